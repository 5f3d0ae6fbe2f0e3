"""Torch-facing wrappers over the CDNA4 radix kernels.

Fail-loud policy: on a CUDA(ROCm)-visible machine these functions REQUIRE
the native extension; there is no silent eager fallback (CPU oracles live
in tests, not here).
"""

from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import load
# op names of reduce_by_key_aos; an op's index is its kernel op code
from ..aggregate import AGGREGATORS as REDUCE_OPS


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def onesweep_passes(start_bit: int, end_bit: int) -> int:
    """Number of 8-bit onesweep passes over key bits [start_bit, end_bit):
    ceil((min(end_bit, 64) - start_bit) / 8), 0 for an empty window. This
    is the count kernels.hip onesweep_sort lays the workspace out for, so
    every ``onesweep_workspace_bytes`` call of a sort wrapper takes it from
    here."""
    bits = min(end_bit, 64) - start_bit
    return -(-bits // 8) if bits > 0 else 0


def sort_records_workspace_bytes(n: int, end_bit: int = 64,
                                 key_bytes: int = 10) -> int:
    """Bytes of ``ws`` that sort_records needs for n records: the native
    figure (kernels.hip), which covers every path the sort can take."""
    return load().sort_records_workspace_bytes(n, min(end_bit, 64), key_bytes)


def _digit_windows(start_bit: int, end_bit: int):
    """The native sort calls, as (start_bit, end_bit) windows run in order,
    that leave the rows ordered by bits [start_bit, end_bit).

    A native call steps 8-bit digits up from its start bit, and every pass
    bins by a full 8-bit digit. That is the window itself when it is a
    whole number of digits, and also when it reaches bit 64: the last pass
    is then clamped to bits [56, 64), which only re-covers bits the pass
    before it ordered. Any other last digit would take in bits ABOVE the
    window and order the rows by those first, so the last pass runs as a
    call of its own over the top 8 bits of the window, re-covering bits
    below it instead. Together the calls make onesweep_passes() passes.

    A window that ends below bit 8 has no 8 bits at or below its top: its
    one pass bins by bits [start_bit, start_bit + 8), which orders the
    rows by the window only when the bits from end_bit up to there are
    equal in all keys (the "shared top bits" case of the readers)."""
    end_bit = min(end_bit, 64)
    bits = end_bit - start_bit
    if bits <= 0:
        return []
    if bits % 8 == 0 or end_bit == 64 or end_bit < 8:
        return [(start_bit, end_bit)]
    whole = start_bit + bits // 8 * 8
    head = [(start_bit, whole)] if whole > start_bit else []
    return head + [(end_bit - 8, end_bit)]


def _check_small_digit(nbits: int, shift: int, func: int) -> None:
    """The kernels bin by at least 4 bits. A narrower digit runs the 4-bit
    kernel, which is the same partition only where the extra mask bits
    read zeros: the digit is the TOP nbits of the (mixed) key."""
    if nbits < 4 and func in (0, 1) and shift != 64 - nbits:
        raise ValueError(f"nbits={nbits} < 4 needs shift == 64 - nbits "
                         f"(the top bits of the key), got shift={shift}")


def digit_counts(src: int, n: int, shift: int, nbits_eff: int, device,
                 func: int = 0, in_stride: int = 1, nparts: int = 0,
                 totals: Optional[torch.Tensor] = None
                 ) -> Tuple[torch.Tensor, torch.Tensor]:
    """radix_hist + radix_scan over the n u64 keys at device address
    ``src`` (``in_stride`` u64 apart). Returns (hist, totals): the scanned
    per-tile histogram for the scatter of the same digit, and the
    int32[2^nbits_eff] digit totals (in ``totals`` when supplied).

    The stream is torch's current one, taken here and not passed in: the
    scan workspace is dropped on return while the scan may still be
    queued, which is safe only because the caching allocator orders reuse
    of a freed block on the current stream — the stream launched on."""
    m = load()
    hist = torch.empty(m.radix_hist_bytes(n, nbits_eff) // 4,
                       dtype=torch.int32, device=device)
    scan_ws = torch.empty(m.radix_scan_ws_bytes(n, nbits_eff) // 4,
                          dtype=torch.int32, device=device)
    if totals is None:
        totals = torch.empty(1 << nbits_eff, dtype=torch.int32, device=device)
    s = _stream()
    m.radix_hist(src, n, shift, nbits_eff, hist.data_ptr(), s, func,
                 in_stride, nparts)
    m.radix_scan(hist.data_ptr(), n, nbits_eff, totals.data_ptr(),
                 scan_ws.data_ptr(), s)
    return hist, totals


def scatter_pairs(pairs: torch.Tensor, n: int, shift: int, nbits_eff: int,
                  hist: torch.Tensor, dst_addr: torch.Tensor,
                  func: int = 0, nparts: int = 0) -> None:
    """Group n interleaved 16-byte (key, aux) pairs by the digit of the
    key into contiguous per-digit runs: digit d's run starts at the device
    byte address ``dst_addr[d]`` (int64[2^nbits_eff] on the device).
    ``hist`` is digit_counts' for the same pairs and digit."""
    val_dst = dst_addr + 8
    load().radix_scatter(pairs.data_ptr(), pairs.data_ptr() + 8, n, shift,
                         nbits_eff, hist.data_ptr(), dst_addr.data_ptr(),
                         val_dst.data_ptr(), _stream(), func, 1, 2, nparts)


def radix_partition(keys: torch.Tensor, vals: Optional[torch.Tensor],
                    nbits: int, shift: Optional[int] = None,
                    key_dst: Optional[torch.Tensor] = None,
                    val_dst: Optional[torch.Tensor] = None,
                    hash_mix: bool = False
                    ) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """One bucket-scatter pass: digit = (key >> shift) & (2^nbits - 1).

    If key_dst/val_dst (u64 device-pointer tables, one per bucket) are
    given, elements scatter straight to those addresses (the map-side
    "write into HBM block buffers" path) and only ``counts`` is returned
    meaningfully. Otherwise contiguous outputs are allocated and per-digit
    bases derived from the counts.

    nbits < 4 is served only as the top nbits of the key (the default
    shift); any other shift raises ValueError.

    Returns (counts u32[2^nbits] on device, keys_out, vals_out).
    """
    n = keys.numel()
    assert keys.dtype in (torch.int64, torch.uint64), "keys must be 64-bit"
    if shift is None:
        shift = 64 - nbits
    # kernel instantiations start at 4 bits; with shift == 64 - nbits the
    # extra mask bits read the zeros the shift brings in above the digit
    nbits_eff = max(nbits, 4)
    nd = 1 << nbits_eff
    dev = keys.device
    if hash_mix and nbits_eff != nbits:
        raise ValueError("hash partitioning requires nbits >= 4")
    _check_small_digit(nbits, shift, int(hash_mix))
    m = load()
    hist, totals = digit_counts(keys.data_ptr(), n, shift, nbits_eff, dev,
                                int(hash_mix))
    keys_out = vals_out = None
    if key_dst is None:
        counts64 = totals.to(torch.int64)
        bases = torch.cumsum(counts64, 0) - counts64
        keys_out = torch.empty_like(keys)
        key_dst = keys_out.data_ptr() + bases * 8   # int64 device addresses
        if vals is not None:
            vals_out = torch.empty_like(vals)
            val_dst = vals_out.data_ptr() + bases * 8
        else:
            val_dst = torch.zeros(nd, dtype=torch.int64, device=dev)
    m.radix_scatter(keys.data_ptr(),
                    vals.data_ptr() if vals is not None else 0,
                    n, shift, nbits_eff, hist.data_ptr(),
                    key_dst.data_ptr(), val_dst.data_ptr(), _stream(),
                    int(hash_mix))
    return totals[:1 << nbits], keys_out, vals_out


def partition_aos(keys: torch.Tensor, vals: torch.Tensor, nbits: int,
                  shift: Optional[int] = None,
                  hash_mix: bool = False):
    """Partition SoA (keys, vals) into ONE interleaved AoS buffer with
    buckets laid out contiguously — the stage-mode (RCCL alltoallv) send
    buffer in a single scatter pass.

    nbits < 4 needs the default shift, as in radix_partition.

    Returns (counts int32[2^nbits] device, pairs int64[2n] device)."""
    n = keys.numel()
    if shift is None:
        shift = 64 - nbits
    _check_small_digit(nbits, shift, int(hash_mix))
    m = load()
    nbits_eff = max(nbits, 4)
    dev = keys.device
    hist, totals = digit_counts(keys.data_ptr(), n, shift, nbits_eff, dev,
                                int(hash_mix))
    pairs = torch.empty(2 * n, dtype=torch.int64, device=dev)
    counts64 = totals.to(torch.int64)
    bases = torch.cumsum(counts64, 0) - counts64
    key_dst = pairs.data_ptr() + bases * 16
    val_dst = key_dst + 8
    m.radix_scatter(keys.data_ptr(), vals.data_ptr(), n, shift, nbits_eff,
                    hist.data_ptr(), key_dst.data_ptr(), val_dst.data_ptr(),
                    _stream(), int(hash_mix), 1)
    return totals[:1 << nbits], pairs


def sort_pairs_aos(pairs: torch.Tensor, start_bit: int = 0,
                   end_bit: int = 64,
                   tmp: Optional[torch.Tensor] = None,
                   ws: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Sort interleaved (key u64, val u64) 16-byte records by key bits
    [start_bit, end_bit). ``pairs`` is an int64 tensor of 2n elements.
    One dwordx4 load + one dwordx4 store per record per pass, and digit
    write bursts twice as long as the SoA path (measured 2x scattered
    write bandwidth at 256 B vs 128 B — profiles/r01_kernel_profile.md).

    Guarantee: the output is ordered by key bits [start_bit, end_bit)
    (end_bit is capped at 64). It is STABLE with respect to that window
    only when the window is a whole number of 8-bit digits that does not
    run past bit 64; otherwise the last pass re-covers bits next to its
    digit (_digit_windows), so rows equal in the window may come out
    ordered by those bits. The result is ``pairs`` itself after an even
    number of passes (onesweep_passes) and ``tmp`` after an odd one.
    ``ws`` needs onesweep_workspace_bytes(n, onesweep_passes(...)) bytes.
    """
    m = load()
    n = pairs.numel() // 2
    if n == 0:
        return pairs
    if tmp is None:
        tmp = torch.empty_like(pairs)
    else:
        assert tmp.numel() >= pairs.numel(), "tmp too small"
        tmp = tmp[:pairs.numel()]
    need_ws = m.onesweep_workspace_bytes(n, onesweep_passes(start_bit,
                                                            end_bit))
    if ws is None:
        ws = torch.empty(need_ws, dtype=torch.uint8, device=pairs.device)
    else:
        assert ws.numel() >= need_ws, "ws too small"
    cur, other = pairs, tmp
    for lo, hi in _digit_windows(start_bit, end_bit):
        if m.onesweep_sort_aos_u64(cur.data_ptr(), other.data_ptr(), n,
                                   lo, hi, ws.data_ptr(), _stream()):
            cur, other = other, cur
    return cur


def reduce_by_key_aos(pairs: torch.Tensor, op: str,
                      out_keys: Optional[torch.Tensor] = None,
                      out_vals: Optional[torch.Tensor] = None,
                      ws: Optional[torch.Tensor] = None
                      ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Segmented reduce over interleaved (key u64, val u64) records whose
    equal keys are adjacent (reduce.hip). ``pairs`` is an int64 tensor of
    2n elements and is left unchanged. Returns SoA (keys, vals), one row
    per run of equal keys in input order; ``vals`` is int64 (sum wraps,
    min/max are signed, count is the run length), float64 for "sum_f64".
    The summation order is fixed, so "sum_f64" is bit-reproducible.

    BLOCKS on the current stream once, to read back the number of runs g.
    ``out_keys``/``out_vals`` (int64, >= g elements) and ``ws`` (uint8,
    >= reduce_by_key_workspace_bytes(n)) may be supplied by the caller; a
    too-small output raises ValueError before anything is written to it.
    """
    if op not in REDUCE_OPS:
        raise ValueError(f"unknown reduce op {op!r}; "
                         f"expected one of {REDUCE_OPS}")
    code = REDUCE_OPS.index(op)
    n = pairs.numel() // 2
    dev = pairs.device
    if n == 0:
        return (torch.empty(0, dtype=torch.int64, device=dev),
                torch.empty(0, dtype=torch.int64, device=dev))
    if n >= 1 << 32:
        raise ValueError("reduce_by_key_aos handles n < 2^32 records")
    m = load()
    nb = -(-n // m.reduce_by_key_tile())
    need_ws = m.reduce_by_key_workspace_bytes(n)
    if ws is None:
        ws = torch.empty(need_ws, dtype=torch.uint8, device=dev)
    elif ws.numel() < need_ws:
        raise ValueError(f"ws too small: {ws.numel()} < {need_ws} bytes")
    s = _stream()
    m.reduce_by_key_count(pairs.data_ptr(), n, code, ws.data_ptr(), s)
    # workspace layout (hipshuffle.h): [lead u64 x nb][base u64 x nb]
    # [heads u32 x nb]; the scan over nb tile counts is plumbing
    heads = ws[16 * nb:20 * nb].view(torch.int32)
    incl = torch.cumsum(heads, 0, dtype=torch.int64)
    ws[8 * nb:16 * nb].view(torch.int64).copy_(incl - heads)
    g = int(incl[-1])                       # syncs the stream
    for name, t in (("out_keys", out_keys), ("out_vals", out_vals)):
        if t is not None and t.numel() < g:
            raise ValueError(f"{name} holds {t.numel()} elements, "
                             f"the input has {g} runs")
    if out_keys is None:
        out_keys = torch.empty(g, dtype=torch.int64, device=dev)
    if out_vals is None:
        out_vals = torch.empty(g, dtype=torch.int64, device=dev)
    m.reduce_by_key_emit(pairs.data_ptr(), n, code, ws.data_ptr(),
                         out_keys.data_ptr(), out_vals.data_ptr(), s)
    keys, vals = out_keys[:g], out_vals[:g]
    if op == "sum_f64":
        vals = vals.view(torch.float64)
    return keys, vals


def extract_pairs(recs: torch.Tensor, rec_bytes: int, key_bytes: int = 8,
                  pairs: Optional[torch.Tensor] = None,
                  bounds: Optional[torch.Tensor] = None,
                  pid: tuple = ()) -> torch.Tensor:
    """records -> interleaved (key-prefix u64, aux u64) pairs, where
    aux = key_lo16 << 48 | record_index (kernels.hip extract_pairs).

    The write path can have pair.x hold the record's partition id instead
    of the prefix: ``bounds`` (int64 device split points, func 4) are
    searched per record (bounds.hip); else ``pid`` = (func, shift, mask,
    nparts) applies that partition function to the prefix."""
    m = load()
    n = recs.numel() // rec_bytes
    if pairs is None:
        pairs = torch.empty(2 * n, dtype=torch.int64, device=recs.device)
    else:
        assert pairs.numel() >= 2 * n
        pairs = pairs[:2 * n]
    if bounds is not None:
        m.extract_pairs_bounds(recs.data_ptr(), n, rec_bytes, key_bytes,
                               pairs.data_ptr(), bounds.data_ptr(),
                               bounds.numel(), _stream())
    else:
        m.extract_pairs(recs.data_ptr(), n, rec_bytes, key_bytes,
                        pairs.data_ptr(), _stream(), *pid)
    return pairs


def _segment_table(segments, n: int, rec_bytes: int, device):
    """``segments`` of sort_records -> (recs pointer, table tensor or None,
    nsegs, checked triples). The table is the device form the kernels search
    (hipshuffle.h): int64 [nsegs, 2] rows of (first_rec, device address).
    One segment needs no table: its address is the contiguous base."""
    segs = sorted((int(a), int(c), int(p)) for a, c, p in segments if c)
    pos = 0
    for first, cnt, ptr in segs:
        if first != pos:
            raise ValueError(f"segments leave a gap or overlap at record "
                             f"{min(first, pos)}")
        if ptr % 4:
            raise ValueError("segment address is not 4-byte aligned")
        pos = first + cnt
    if pos != n:
        raise ValueError(f"segments cover {pos} records, expected {n}")
    if len(segs) == 1:
        return segs[0][2], None, 0, segs
    table = torch.tensor([[first, ptr] for first, _cnt, ptr in segs],
                         dtype=torch.int64, device=device)
    return 0, table, len(segs), segs


def sort_records(recs, rec_bytes: int, key_bytes: int = 8,
                 end_bit: int = 64, out: Optional[torch.Tensor] = None,
                 pairs: Optional[torch.Tensor] = None,
                 tmp: Optional[torch.Tensor] = None,
                 ws: Optional[torch.Tensor] = None,
                 fuse: bool = True,
                 pairs_filled: bool = False,
                 segments=None) -> torch.Tensor:
    """Sort W-byte AoS records by their 80-bit key: u64 LE prefix at
    offset 0 (bits [0, end_bit) significant — callers whose partitions
    share top prefix bits pass end_bit = 64 - shared) then, for
    key_bytes == 10, a u16 LE low word at offset 8.

    Only 16-byte (prefix, aux) pairs flow through the radix passes; one
    gather pass then moves each record once — pair passes cost 16% of
    full-record passes at W = 100 (kernels.hip 'wide-record machinery').
    Returns the sorted records (a fresh tensor, or ``out``).

    ``segments``: the records are not one contiguous buffer but
    ``(first_rec, nrec, device_ptr)`` runs, as a reader's
    ``record_segments()`` returns them: record ``first_rec + i`` is the
    ``i``-th record at ``device_ptr``. The runs must cover every index
    exactly once. ``recs`` then only supplies the extent — a uint8 tensor
    of that many bytes whose contents are never read, or the byte count
    itself — and pair indices are positions in that virtual buffer, so the
    output is the one a contiguous copy would give. The memory behind the
    pointers must stay valid until the sort has run on the stream.

    With ``fuse`` and tie repair on (the default) the call BLOCKS on
    the current stream once: the truncated sort reads back a flag that
    says whether the full pass sequence must run after all. ``ws``, when
    given, needs sort_records_workspace_bytes(n, end_bit, key_bytes) bytes.
    """
    m = load()
    nbytes = recs if isinstance(recs, int) else recs.numel()
    n = nbytes // rec_bytes
    if n == 0:
        return (recs if isinstance(recs, torch.Tensor)
                else torch.empty(0, dtype=torch.uint8, device="cuda"))
    if segments is None:
        dev = recs.device
        recs_ptr, seg_t, nsegs, segs = recs.data_ptr(), None, 0, None
    else:
        dev = (recs.device if isinstance(recs, torch.Tensor)
               else out.device if out is not None
               else torch.device("cuda", torch.cuda.current_device()))
        recs_ptr, seg_t, nsegs, segs = _segment_table(segments, n,
                                                      rec_bytes, dev)
    seg_ptr = seg_t.data_ptr() if seg_t is not None else 0
    if pairs_filled:
        # caller already extracted (e.g. incrementally per fetched chunk,
        # overlapping the fetch phase)
        assert pairs is not None and pairs.numel() >= 2 * n
        prs = pairs[:2 * n]
    elif segments is None:
        prs = extract_pairs(recs, rec_bytes, key_bytes, pairs)
    else:
        if pairs is None:
            pairs = torch.empty(2 * n, dtype=torch.int64, device=dev)
        assert pairs.numel() >= 2 * n
        prs = pairs[:2 * n]
        for first, cnt, ptr in segs:
            m.extract_pairs(ptr, cnt, rec_bytes, key_bytes,
                            prs.data_ptr() + 16 * first, _stream(),
                            idx_base=first)
    if tmp is None:
        tmp = torch.empty_like(prs)
    else:
        assert tmp.numel() >= 2 * n
        tmp = tmp[:2 * n]
    need_ws = sort_records_workspace_bytes(n, end_bit, key_bytes)
    if ws is None:
        ws = torch.empty(need_ws, dtype=torch.uint8, device=dev)
    else:
        assert ws.numel() >= need_ws
    if out is None:
        out = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    else:
        assert out.numel() >= nbytes
        out = out[:nbytes]
    # kernels.hip sort_records_u64: the truncated sort (LSD over the leading
    # key bits only, tied runs repaired in LDS) where it applies, else or
    # after it the full pass sequence. Path: last_sort_path().
    m.sort_records_u64(prs.data_ptr(), tmp.data_ptr(), n, min(end_bit, 64),
                       key_bytes, ws.data_ptr(), _stream(), recs_ptr,
                       out.data_ptr(), rec_bytes, int(fuse), seg_ptr, nsegs)
    return out


def _record_source(recs, rec_bytes: int, segments, device=None):
    """(byte count, n, device, recs pointer, segment table or None, nsegs,
    checked segment triples or None) of a record buffer given the
    sort_records way: a tensor, or an extent plus ``segments``."""
    nbytes = recs if isinstance(recs, int) else recs.numel()
    n = nbytes // rec_bytes
    if segments is None:
        if isinstance(recs, int):
            raise ValueError("recs may be a byte count only with segments")
        return nbytes, n, recs.device, recs.data_ptr(), None, 0, None
    dev = (recs.device if isinstance(recs, torch.Tensor)
           else device if device is not None
           else torch.device("cuda", torch.cuda.current_device()))
    if n == 0:
        return nbytes, 0, dev, 0, None, 0, []
    ptr, table, nsegs, segs = _segment_table(segments, n, rec_bytes, dev)
    return nbytes, n, dev, ptr, table, nsegs, segs


def _empty_columns(cols, dev):
    from ..aggregate import column_is_float
    return (torch.empty(0, dtype=torch.int64, device=dev),
            [torch.empty(0, dtype=torch.float64 if column_is_float(t, o)
                         else torch.int64, device=dev)
             for _off, t, o in cols])


def reduce_records_workspace_bytes(n: int, ncols: int) -> int:
    """Bytes of ``ws`` that reduce_records_by_key needs for n pairs and
    ncols columns: the widened-value scratch and the per-tile tables."""
    return load().reduce_records_workspace_bytes(n, ncols)


def reduce_records_by_key(pairs: torch.Tensor, recs, rec_bytes: int, columns,
                          segments=None,
                          out_keys: Optional[torch.Tensor] = None,
                          out_vals: Optional[torch.Tensor] = None,
                          ws: Optional[torch.Tensor] = None):
    """Reduce up to 8 typed columns of W-byte records per key, without
    moving a record (reduce_records.hip). ``pairs`` is an int64 tensor of
    2n elements, interleaved (key, aux) as extract_pairs writes them with
    equal keys adjacent (all 64 bits; 8-byte keys only); record
    ``aux & (2^48 - 1)`` of ``recs`` belongs to a pair. ``recs`` /
    ``segments`` are sort_records': a uint8 tensor, or an extent (tensor or
    byte count) plus ``(first_rec, nrec, device_ptr)`` runs. Pairs and
    records are left unchanged.

    ``columns`` is a sequence of ``(offset_bytes, dtype, op)``, dtype in
    ("i32", "u32", "i64", "f32", "f64"), op in ("sum", "min", "max",
    "count"); for "count" dtype and offset may be None. The dtype decides
    the accumulator: integers reduce as int64 (i32 sign-, u32 zero-extended;
    sums wrap), floats as float64 in a fixed order, so a float sum is
    bit-reproducible for a given pair order wherever the records lie.

    Returns ``(keys int64[g], [one tensor[g] per column])``, one row per
    run in input order; a column is float64 for f32 / f64 dtypes, int64
    otherwise. The columns are views of one [C, g] buffer.

    BLOCKS on the current stream once, to read back the number of runs g.
    ``out_keys`` (int64, >= g), ``out_vals`` (int64, >= C * g) and ``ws``
    (uint8, >= reduce_records_workspace_bytes(n, C)) may be supplied by the
    caller; one that is too small raises ValueError before anything is
    written to it. With ``segments`` the memory behind the pointers must
    stay valid until the call has run on the stream."""
    from ..aggregate import check_columns, column_is_float
    cols = check_columns(columns, rec_bytes)
    C = len(cols)
    n = pairs.numel() // 2
    if n >= 1 << 32:
        raise ValueError("reduce_records_by_key handles n < 2^32 records")
    _nbytes, nrec, dev, recs_ptr, seg_t, nsegs, _segs = _record_source(
        recs, rec_bytes, segments, pairs.device)
    if n == 0:
        return _empty_columns(cols, pairs.device)
    if nrec == 0:
        raise ValueError("pairs without records")
    m = load()
    nb = -(-n // m.reduce_records_tile())
    need_ws = m.reduce_records_workspace_bytes(n, C)
    if ws is None:
        ws = torch.empty(need_ws, dtype=torch.uint8, device=pairs.device)
    elif ws.numel() < need_ws:
        raise ValueError(f"ws too small: {ws.numel()} < {need_ws} bytes")
    s = _stream()
    words = [off // 4 for off, _t, _o in cols]
    types = [t for _off, t, _o in cols]
    ops = [o for _off, _t, o in cols]
    m.reduce_records_count(pairs.data_ptr(), n, recs_ptr, rec_bytes,
                           seg_t.data_ptr() if seg_t is not None else 0,
                           nsegs, words, types, ops, ws.data_ptr(), s)
    # workspace layout (hipshuffle.h): [scratch u64 x C*n][lead u64 x C*nb]
    # [base u64 x nb][heads u32 x nb]; the scan over nb tile counts is
    # plumbing
    base_off = 8 * C * (n + nb)
    heads = ws[base_off + 8 * nb:base_off + 12 * nb].view(torch.int32)
    incl = torch.cumsum(heads, 0, dtype=torch.int64)
    ws[base_off:base_off + 8 * nb].view(torch.int64).copy_(incl - heads)
    g = int(incl[-1])                       # syncs the stream
    for name, t, need in (("out_keys", out_keys, g),
                          ("out_vals", out_vals, C * g)):
        if t is not None and t.numel() < need:
            raise ValueError(f"{name} holds {t.numel()} elements, the "
                             f"input has {g} runs: {need} needed")
    if out_keys is None:
        out_keys = torch.empty(g, dtype=torch.int64, device=pairs.device)
    if out_vals is None:
        out_vals = torch.empty(C * g, dtype=torch.int64, device=pairs.device)
    m.reduce_records_emit(pairs.data_ptr(), n, types, ops, ws.data_ptr(), g,
                          out_keys.data_ptr(), out_vals.data_ptr(), s)
    vals = []
    for c, (_off, t, o) in enumerate(cols):
        v = out_vals[c * g:(c + 1) * g]
        vals.append(v.view(torch.float64) if column_is_float(t, o) else v)
    return out_keys[:g], vals


def aggregate_records(recs, rec_bytes: int, columns, end_bit: int = 64,
                      segments=None, pairs: Optional[torch.Tensor] = None,
                      tmp: Optional[torch.Tensor] = None,
                      ws: Optional[torch.Tensor] = None):
    """GROUP BY over W-byte AoS records with a u64 LE key at offset 0:
    extract (key, index) pairs, sort them by key bits [0, end_bit)
    (callers whose keys share their top bits pass a smaller end_bit and
    save radix passes), reduce ``columns`` per key with
    reduce_records_by_key. No record is moved or copied; ``recs`` /
    ``segments`` are sort_records'. Returns ``(keys int64[g], [one
    tensor[g] per column])`` with the keys ascending (unsigned).

    ``pairs`` and ``tmp`` (int64, >= 2n) are the pair buffers of the sort;
    ``ws`` (uint8) serves the sort and then the reduction and needs the
    larger of onesweep_workspace_bytes(n, onesweep_passes(0, end_bit)) and
    reduce_records_workspace_bytes(n, C). BLOCKS once, in the reduction."""
    from ..aggregate import check_columns
    cols = check_columns(columns, rec_bytes)
    if not 1 <= end_bit <= 64:
        raise ValueError("end_bit must be in [1, 64]")
    if rec_bytes < 8:
        raise ValueError("records hold a u64 key: rec_bytes >= 8")
    _nbytes, n, dev, _ptr, _seg_t, _nsegs, segs = _record_source(
        recs, rec_bytes, segments)
    if n == 0:
        return _empty_columns(cols, dev)
    if n >= 1 << 32:
        raise ValueError("aggregate_records handles n < 2^32 records")
    m = load()
    need_ws = max(m.onesweep_workspace_bytes(n, onesweep_passes(0, end_bit)),
                  m.reduce_records_workspace_bytes(n, len(cols)))
    if ws is None:
        ws = torch.empty(need_ws, dtype=torch.uint8, device=dev)
    elif ws.numel() < need_ws:
        raise ValueError(f"ws too small: {ws.numel()} < {need_ws} bytes")
    if segments is None:
        prs = extract_pairs(recs, rec_bytes, 8, pairs)
    else:
        if pairs is None:
            pairs = torch.empty(2 * n, dtype=torch.int64, device=dev)
        if pairs.numel() < 2 * n:
            raise ValueError("pairs too small")
        prs = pairs[:2 * n]
        for first, cnt, ptr in segs:
            m.extract_pairs(ptr, cnt, rec_bytes, 8,
                            prs.data_ptr() + 16 * first, _stream(),
                            idx_base=first)
    prs = sort_pairs_aos(prs, 0, end_bit, tmp=tmp, ws=ws)
    return reduce_records_by_key(prs, recs, rec_bytes, columns,
                                 segments=segments, ws=ws)


def gather_grouped(recs: torch.Tensor, pairs_grouped: torch.Tensor, n: int,
                   rec_bytes: int, counts: np.ndarray, dst_addr: np.ndarray,
                   shift: int, mask: int, func: int = 0,
                   nparts: int = 0) -> None:
    """The one gather of the partition path: pairs_grouped[j] names the
    record that moves to dst_addr[d] + (j - start[d]) * rec_bytes, where d
    is the digit of its key under (shift, mask, func, nparts) and start
    the exclusive sum of ``counts``. ``counts`` / ``dst_addr``: int64
    numpy, one entry per digit; dst_addr holds device byte addresses."""
    dev = recs.device
    starts = np.cumsum(counts) - counts
    dstart_t = torch.from_numpy(starts.astype(np.uint32)
                                .view(np.int32)).to(dev)
    dst_addr_t = torch.from_numpy(dst_addr).to(dev)
    load().gather_records(recs.data_ptr(), pairs_grouped.data_ptr(), n,
                          rec_bytes, 1, 0, dst_addr_t.data_ptr(),
                          dstart_t.data_ptr(), shift, mask, func, nparts,
                          _stream())


FUSED_DIGIT_BITS = 8    # widest digit of the fused record partition


class RecordDigits(NamedTuple):
    """What count_record_digits hands to group_records."""
    pairs: torch.Tensor
    n: int
    counts: np.ndarray              # int64[2^nbits_eff] digit totals
    # digits wider than FUSED_DIGIT_BITS only: digit_counts' per-tile
    # matrix and the (shift, nbits_eff, func, nparts) it was counted under
    hist: Optional[torch.Tensor] = None
    digit: tuple = ()


def count_record_digits(recs: torch.Tensor, rec_bytes: int, key_bytes: int,
                        shift: int, nbits_eff: int, func: int = 0,
                        nparts: int = 0,
                        bounds: Optional[torch.Tensor] = None
                        ) -> RecordDigits:
    """First half of a single-pass record partition: extract the pairs and
    count the digit (shift, nbits_eff, func, nparts — or a search of
    ``bounds``) of every record, so that the caller can lay out its
    destinations. BLOCKS on the current stream to read the totals back.

    Digits of at most FUSED_DIGIT_BITS bits: pair.x holds the digit itself,
    whichever partition function produced it, and count_pair_digits totals
    it in one read of the pairs. Wider digits keep the prefix (or the
    searched id) in pair.x and digit_counts' per-tile matrix for the
    scatter of group_records."""
    n = recs.numel() // rec_bytes
    if n >= 1 << 32:
        raise ValueError("a record partition handles n < 2^32 records")
    nd = 1 << nbits_eff
    if nbits_eff <= FUSED_DIGIT_BITS:
        pairs = extract_pairs(recs, rec_bytes, key_bytes, bounds=bounds,
                              pid=(func, shift, nd - 1, nparts))
        totals = torch.empty(1 << FUSED_DIGIT_BITS, dtype=torch.int32,
                             device=recs.device)
        load().count_pair_digits(pairs.data_ptr(), n, totals.data_ptr(),
                                 _stream())
        counts = totals.cpu().numpy().astype(np.int64)  # syncs the stream
        return RecordDigits(pairs, n, counts[:nd])
    pairs = extract_pairs(recs, rec_bytes, key_bytes, bounds=bounds)
    if bounds is not None:
        # hist / scatter / gather read the searched id as plain bits
        func, shift, nparts = 0, 0, 0
    hist, totals = digit_counts(pairs.data_ptr(), n, shift, nbits_eff,
                                recs.device, func, 2, nparts)
    counts = totals.cpu().numpy().astype(np.int64)      # syncs the stream
    return RecordDigits(pairs, n, counts, hist,
                        (shift, nbits_eff, func, nparts))


def group_records(recs: torch.Tensor, rec_bytes: int, digits: RecordDigits,
                  dst_addr: np.ndarray) -> None:
    """Second half, after the caller's layout: move digit d's records, in
    input order, to the device byte address dst_addr[d] onward (int64
    numpy, one entry per digit; entries of empty digits are not used).

    Digits of at most FUSED_DIGIT_BITS bits take ONE pass, the fused pass
    kernel of the sort with the digit bases replaced by ``dst_addr``
    (kernels.hip partition_records_fused): no grouped copy of the pairs,
    no separate gather. Wider digits group the pairs (scatter_pairs) and
    then gather the records (gather_grouped).

    The workspace and the address table are dropped on return while the
    pass may still be queued; see digit_counts for why that is safe."""
    pairs, n = digits.pairs, digits.n
    if digits.hist is None:
        if (np.asarray(dst_addr) % 4).any():
            raise ValueError("destination addresses must be 4-byte aligned")
        m = load()
        table = np.zeros(1 << FUSED_DIGIT_BITS, dtype=np.int64)
        table[:len(dst_addr)] = dst_addr
        table_t = torch.from_numpy(table).to(recs.device)
        ws = torch.empty(m.partition_records_workspace_bytes(n),
                         dtype=torch.uint8, device=recs.device)
        m.partition_records_fused(pairs.data_ptr(), n, recs.data_ptr(),
                                  rec_bytes, table_t.data_ptr(),
                                  ws.data_ptr(), _stream())
        return
    shift, nbits_eff, func, nparts = digits.digit
    pairs_out = torch.empty_like(pairs)
    starts_t = torch.from_numpy(np.cumsum(digits.counts) - digits.counts) \
        .to(recs.device)
    scatter_pairs(pairs, n, shift, nbits_eff, digits.hist,
                  pairs_out.data_ptr() + starts_t * 16, func, nparts)
    gather_grouped(recs, pairs_out, n, rec_bytes, digits.counts, dst_addr,
                   shift, (1 << nbits_eff) - 1, func, nparts)


def partition_records(recs: torch.Tensor, rec_bytes: int,
                      key_bytes: int = 8, nbits: int = 8,
                      shift: Optional[int] = None, func: int = 0,
                      nparts: int = 0):
    """Group W-byte records into 2^nbits contiguous buckets (digit from
    the key prefix) — the stage-mode (RCCL alltoall) send-buffer builder
    for wide records. nbits < 4 with a bit-extraction func (0, 1) needs
    the default shift, as in radix_partition.
    Returns (counts int64 numpy, grouped records)."""
    n = recs.numel() // rec_bytes
    if shift is None:
        shift = 64 - nbits
    _check_small_digit(nbits, shift, func)
    nbits_eff = max(nbits, 4)
    digits = count_record_digits(recs, rec_bytes, key_bytes, shift,
                                 nbits_eff, func, nparts)
    counts = digits.counts
    out = torch.empty_like(recs)
    dst = out.data_ptr() + (np.cumsum(counts) - counts) * rec_bytes
    group_records(recs, rec_bytes, digits, dst)
    return counts[:1 << nbits], out


def sort_pairs(keys: torch.Tensor, vals: Optional[torch.Tensor] = None,
               start_bit: int = 0, end_bit: int = 64,
               onesweep: Optional[bool] = None
               ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """LSD radix sort of u64 keys (and optional u64 payload) on device.

    Sorts by bits [start_bit, end_bit) — callers that range-partitioned by
    the top bits pass end_bit = 64 - log2(R) and save whole passes.
    Uses the decoupled-lookback onesweep path (one kernel per pass) when
    n < 2^30; the 3-kernel hist/scan/scatter path otherwise.

    Guarantee: the output is ordered by key bits [start_bit, end_bit)
    (end_bit is capped at 64). It is STABLE with respect to that window
    only when the window is a whole number of 8-bit digits that does not
    run past bit 64; otherwise the last pass re-covers bits next to its
    digit (_digit_windows), so rows equal in the window may come out
    ordered by those bits. The result is in the input tensors after an
    even number of passes (onesweep_passes) and in fresh ones after an
    odd one.
    """
    m = load()
    n = keys.numel()
    if n == 0:
        return keys, vals
    dev = keys.device
    tmp_k = torch.empty_like(keys)
    tmp_v = torch.empty_like(vals) if vals is not None else None
    if onesweep is None:
        onesweep = n < (1 << 30)
    if onesweep:
        sort = m.onesweep_sort_pairs_u64
        ws_bytes = m.onesweep_workspace_bytes(
            n, onesweep_passes(start_bit, end_bit))
    else:
        sort = m.sort_pairs_u64
        ws_bytes = m.sort_workspace_bytes(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    cur, other = (keys, vals), (tmp_k, tmp_v)
    for lo, hi in _digit_windows(start_bit, end_bit):
        if sort(cur[0].data_ptr(),
                cur[1].data_ptr() if vals is not None else 0,
                other[0].data_ptr(),
                other[1].data_ptr() if vals is not None else 0,
                n, lo, hi, ws.data_ptr(), _stream()):
            cur, other = other, cur
    return cur


class AosSorter:
    """Persistent-buffer AoS sorter: workspace and ping-pong buffer are
    allocated once, so a sort issues ONLY kernel launches and stream
    memsets. (Intended to make the launch sequence hipGraph-capturable;
    torch.cuda.graph capture of the extension's launches SIGABRTs on this
    ROCm/torch build — see ROADMAP.md — so capture is not wired up.)"""

    def __init__(self, n: int, device="cuda", start_bit: int = 0,
                 end_bit: int = 64):
        m = load()
        self.n = n
        self.start_bit = start_bit
        self.end_bit = min(end_bit, 64)
        self.tmp = torch.empty(2 * n, dtype=torch.int64, device=device)
        self.ws = torch.empty(
            m.onesweep_workspace_bytes(n, onesweep_passes(start_bit, end_bit)),
            dtype=torch.uint8, device=device)
        self._m = m

    def sort_(self, pairs: torch.Tensor) -> torch.Tensor:
        """sort_pairs_aos(pairs, start_bit, end_bit) on the held buffers:
        same ordering guarantee, same rule for which buffer comes back."""
        assert pairs.numel() == 2 * self.n
        return sort_pairs_aos(pairs, self.start_bit, self.end_bit,
                              tmp=self.tmp, ws=self.ws)
