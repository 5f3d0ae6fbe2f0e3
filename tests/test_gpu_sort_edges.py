"""Radix partition and sort kernels at tile, wave and digit-window edges,
against the plain numpy checkers of sort_oracle.py (gfx950 only).

The payload of every input is the row index, so an output names the source
of each of its rows: a payload on the wrong one of two equal keys, a tail
lane counted as digit 0, a lost or doubled row and a pass that lands in the
wrong ping-pong buffer all fail an exact integer comparison. There are no
tolerances in this file.

Constants of the kernels under test (kernels.hip): the SoA and AoS tile is
4096 elements, a wave 64 lanes, the sort pass ranks iteration pairs of 128
elements per wave, a wave's chunk is 1024 (SoA) or 512 (AoS) elements, and
the 3-kernel path scans its histogram in chunks of 64 tiles.

The loops run over sizes and patterns inside each test, a few hundred small
launches per test, not one pytest case each."""

import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sort_oracle import check_sorted, expect_partition, window  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = 4096
EDGE_N = [1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025,
          4095, 4096, 4097, 4096 + 64, 8191, 8192, 8193, 3 * 4096 + 1]
# patterns whose keys fit in 16 bits at every size used with them
NARROW = ("zeros", "sawtooth_b0", "sawtooth_b1", "descending",
          "random_narrow")
GUARD = 4096          # bytes (ws) / elements (tmp) either side
U64_MAX = (1 << 64) - 1


@pytest.fixture(scope="module")
def hs():
    from sparkrdma_amd.ops import load
    return load()


def patterns(n, seed, sawtooth_bytes=range(8)):
    """name -> uint64[n] keys; the payload is always the row index."""
    rng = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.uint64)
    a, b, c = rng.integers(0, U64_MAX, 3, dtype=np.uint64, endpoint=True)
    out = {
        "zeros": np.zeros(n, dtype=np.uint64),
        "ones": np.full(n, U64_MAX, dtype=np.uint64),
        "one_digit": np.full(n, c, dtype=np.uint64),
        "two_digits_by_lane": np.where(i & np.uint64(1), a, b),
        "two_digits_by_iteration":
            np.where((i >> np.uint64(6)) & np.uint64(1), a, b),
        "descending": np.uint64(n - 1) - i,
        "random_narrow": rng.integers(0, 500, n, dtype=np.uint64),
        "random_u64": rng.integers(0, U64_MAX, n, dtype=np.uint64,
                                   endpoint=True),
    }
    for byte in sawtooth_bytes:
        out[f"sawtooth_b{byte}"] = (i % np.uint64(256)) << np.uint64(8 * byte)
    return out


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy()


def soa(onesweep):
    """run(keys, start_bit, end_bit) -> (keys, payload, same_buffer) through
    sort_pairs on the chosen path."""
    from sparkrdma_amd.ops.radix import sort_pairs

    def run(k, s, e):
        kd = dev(k)
        vd = torch.arange(k.size, dtype=torch.int64, device="cuda")
        ko, vo = sort_pairs(kd, vd, s, e, onesweep=onesweep)
        assert (ko.data_ptr() == kd.data_ptr()) == \
            (vo.data_ptr() == vd.data_ptr()), "keys and vals in unlike buffers"
        return host(ko), host(vo), ko.data_ptr() == kd.data_ptr()
    return run


def interleave(k):
    n = k.size
    pairs = np.empty(2 * n, dtype=np.uint64)
    pairs[0::2] = k
    pairs[1::2] = np.arange(n, dtype=np.uint64)
    return dev(pairs)


def aos(k, s, e):
    from sparkrdma_amd.ops.radix import sort_pairs_aos
    pairs = interleave(k)
    out = host(sort_pairs_aos(pairs, s, e))
    return out[0::2], out[1::2], None


class Guarded:
    """``size`` elements of ``dtype`` with GUARD patterned elements on
    either side, all in one allocation: a kernel that runs past the end of
    the inner tensor (or before its start) changes a guard, and check()
    turns that into a failed assertion."""

    def __init__(self, size, dtype, fill):
        self.fill = fill
        self.buf = torch.full((GUARD + size + GUARD,), fill, dtype=dtype,
                              device="cuda")
        self.inner = self.buf[GUARD:GUARD + size]

    def check(self, what):
        lo, hi = self.buf[:GUARD], self.buf[GUARD + self.inner.numel():]
        assert bool((lo == self.fill).all()), f"{what}: wrote before start"
        bad = torch.nonzero(hi != self.fill).flatten()
        assert bad.numel() == 0, \
            (f"{what}: wrote {bad.numel()} elements past the end, first at "
             f"+{int(bad[0])}, last at +{int(bad[-1])}")


def aos_guarded(hs, k, s, e):
    """sort_pairs_aos with caller tmp and ws of EXACTLY the documented
    sizes, each between guards."""
    from sparkrdma_amd.ops.radix import onesweep_passes, sort_pairs_aos
    n = k.size
    pairs = interleave(k)
    tmp = Guarded(2 * n, torch.int64, 0x5A5A5A5A5A5A5A5A)
    ws = Guarded(hs.onesweep_workspace_bytes(n, onesweep_passes(s, e)),
                 torch.uint8, 0xA5)
    res = sort_pairs_aos(pairs, s, e, tmp=tmp.inner, ws=ws.inner)
    out = host(res)
    tmp.check(f"tmp, n={n} bits [{s}, {e})")
    ws.check(f"ws, n={n} bits [{s}, {e})")
    assert res.data_ptr() in (pairs.data_ptr(), tmp.inner.data_ptr())
    return out[0::2], out[1::2], res.data_ptr() == pairs.data_ptr()


def checked(run, k, s, e, stable, label):
    gk, gv, same = run(k, s, e)
    try:
        check_sorted(k, np.arange(k.size), gk, gv, s, e, stable)
    except AssertionError as ex:
        raise AssertionError(f"{label} n={k.size} bits [{s}, {e}): {ex}") \
            from None
    return same


def edge_matrix(run, label, sizes=EDGE_N):
    for n in sizes:
        for name, k in patterns(n, seed=n).items():
            checked(run, k, 0, 64, True, f"{label} {name}")
            if name in NARROW:
                checked(run, k, 0, 16, True, f"{label} {name}")


# ---------------------------------------------------------------------------
# partition: LDS attribute of the keys-only and keys+vals kernels

def _partition_check(keys_np, with_vals, nbits, shift=None, label=""):
    from sparkrdma_amd.ops.radix import radix_partition
    n = keys_np.size
    kd = dev(keys_np)
    vd = torch.arange(n, dtype=torch.int64, device="cuda") if with_vals \
        else None
    counts, ko, vo = radix_partition(kd, vd, nbits, shift)
    want_counts, order = expect_partition(
        keys_np, 64 - nbits if shift is None else shift, nbits)
    where = f"{label} n={n} nbits={nbits} shift={shift} vals={with_vals}"
    got_counts = host(counts).astype(np.int64)
    assert got_counts.shape == (1 << nbits,), where
    assert int(got_counts.sum()) == n, where
    assert np.array_equal(got_counts, want_counts), where
    assert np.array_equal(host(ko).view(np.uint64), keys_np[order]), where
    if with_vals:
        assert np.array_equal(host(vo), order), where
    else:
        assert vo is None, where


def test_00_partition_keys_only_before_keys_and_vals(hs):
    """FIRST in this file on purpose. The 12-bit scatter needs 129 KiB of
    dynamic LDS, so each of radix_scatter_kernel<12, false> (keys only) and
    <12, true> (keys + vals) must have had the LDS attribute set on ITSELF
    before its first launch. One shared per-NBITS flag skipped whichever ran
    second in a process. pytest runs a file's tests in the order they are
    written, and the 00 in the name keeps this one first under any plugin
    that sorts by name: before any other 12-bit call of this file, so that
    in a run of this file the keys-only kernel is the first of the two in
    the process and the keys+vals kernel the second. (In a run of the whole
    suite an earlier file may have used the 12-bit keys+vals kernel; then
    the keys-only call here is the second of the two, which is as good.)
    The test below takes the other order for 11 bits."""
    k = patterns(4097, seed=12, sawtooth_bytes=())["random_u64"]
    _partition_check(k, False, 12)
    _partition_check(k, True, 12)
    _partition_check(k, False, 12)


def test_partition_keys_and_vals_before_keys_only(hs):
    """The same for 11 bits (81 KiB of LDS), keys + vals first, and a
    second round for 12 bits now that both kernels have run."""
    for nbits in (11, 12):
        k = patterns(4097, seed=nbits, sawtooth_bytes=())["random_u64"]
        _partition_check(k, True, nbits)
        _partition_check(k, False, nbits)
        _partition_check(k, True, nbits)


# ---------------------------------------------------------------------------
# sorts

def test_onesweep_soa_edges(hs):
    edge_matrix(soa(True), "onesweep")


def test_soa_keys_only(hs):
    from sparkrdma_amd.ops.radix import sort_pairs
    for onesweep in (True, False):
        for n in EDGE_N:
            pats = patterns(n, seed=n, sawtooth_bytes=(3,))
            for name in ("zeros", "random_narrow", "random_u64",
                         "two_digits_by_iteration", "sawtooth_b3"):
                k = pats[name]
                ko, vo = sort_pairs(dev(k), None, onesweep=onesweep)
                assert vo is None
                assert np.array_equal(host(ko).view(np.uint64), np.sort(k)), \
                    f"onesweep={onesweep} {name} n={n}"


def test_three_kernel_soa_edges(hs):
    edge_matrix(soa(False), "3-kernel")


def test_three_kernel_scan_chunk_edges(hs):
    """One scan chunk exactly (64 tiles), a second chunk holding one row,
    and a third: the hierarchical scan's chunk sums and rewrite."""
    run = soa(False)
    for n in (64 * TILE - 1, 64 * TILE, 64 * TILE + 1, 128 * TILE + 1):
        pats = patterns(n, seed=n, sawtooth_bytes=())
        checked(run, pats["random_narrow"], 0, 16, True, "3-kernel narrow")
        checked(run, pats["one_digit"], 0, 64, True, "3-kernel one_digit")


def test_aos_edges(hs):
    edge_matrix(aos, "aos")


def test_aos_caller_buffers_exact_size(hs):
    """tmp and ws supplied by the caller at exactly the documented sizes:
    an overrun of either shows in the guards."""
    def run(k, s, e):
        return aos_guarded(hs, k, s, e)
    for n in (1, 64, 513, 4095, 4096, 4097, 8193, 3 * 4096 + 1):
        pats = patterns(n, seed=n, sawtooth_bytes=(7,))
        for name in ("zeros", "random_narrow", "random_u64", "sawtooth_b7"):
            checked(run, pats[name], 0, 64, True, f"aos guarded {name}")
        checked(run, pats["random_narrow"], 0, 16, True, "aos guarded narrow")


def test_aos_sorter(hs):
    from sparkrdma_amd.ops.radix import AosSorter, onesweep_passes
    for start_bit in (0, 4):
        for n in (1000, 4097, 3 * 4096 + 1):
            sorter = AosSorter(n, start_bit=start_bit)
            assert sorter.ws.numel() == hs.onesweep_workspace_bytes(
                n, onesweep_passes(start_bit, 64))
            assert sorter.tmp.numel() == 2 * n
            for seed in (1, 2):                 # the buffers are reused
                k = patterns(n, seed=seed, sawtooth_bytes=())["random_u64"]

                def run(k, s, e):
                    out = host(sorter.sort_(interleave(k)))
                    return out[0::2], out[1::2], None
                checked(run, k, start_bit, 64, start_bit == 0,
                        f"AosSorter start_bit={start_bit}")


def test_ping_pong_parity(hs):
    """After an even number of passes the result is in the caller's
    buffers, after an odd number in the other ones; correct either way."""
    from sparkrdma_amd.ops.radix import onesweep_passes

    def guarded(k, s, e):
        return aos_guarded(hs, k, s, e)
    paths = (("onesweep", soa(True)), ("3-kernel", soa(False)),
             ("aos", guarded))
    for s, e in ((0, 8), (0, 16), (0, 24), (8, 32)):
        passes = onesweep_passes(s, e)
        assert passes == (e - s) // 8
        for n in (1000, 4097):
            k = patterns(n, seed=n + e, sawtooth_bytes=())["random_u64"]
            for label, run in paths:
                same = checked(run, k, s, e, True, label)
                assert same == (passes % 2 == 0), \
                    (f"{label} n={n} bits [{s}, {e}): {passes} passes, "
                     f"result in the input buffer: {same}")


def test_windows_off_the_digit_grid(hs):
    """Windows that are not whole digits or do not start at bit 0. Every
    one must come out ordered by exactly its own bits; the whole-digit ones
    that end at or below bit 64 stably. (4, 64), (57, 64) and (60, 64) are
    the windows whose workspace the wrappers used to undersize."""
    from sparkrdma_amd.ops.radix import onesweep_passes

    def guarded(k, s, e):
        return aos_guarded(hs, k, s, e)
    paths = (("onesweep", soa(True)), ("3-kernel", soa(False)),
             ("aos", aos), ("aos guarded", guarded))
    want_passes = {(4, 64): 8, (60, 64): 1, (57, 64): 1, (0, 12): 2,
                   (8, 20): 2, (3, 11): 1, (52, 60): 1}
    for (s, e), passes in want_passes.items():
        assert onesweep_passes(s, e) == passes
        stable = (e - s) % 8 == 0 and e <= 64
        for n in (1000, 4097, 3 * 4096 + 1):
            # what the wrappers allocate: the helper's pass count, through
            # the module's own size function (tiles of 4096)
            nb = -(-n // TILE)
            assert hs.onesweep_workspace_bytes(n, onesweep_passes(s, e)) == \
                passes * 1024 + 2 * 256 * 8 + 16 + nb * 256 * 8
            k = patterns(n, seed=n + s, sawtooth_bytes=())["random_u64"]
            for label, run in paths:
                checked(run, k, s, e, False, label)
                if stable:
                    checked(run, k, s, e, True, label)


def test_long_lookback_chains(hs):
    """301 tiles of one digit: tile b's prefix is exactly b * 4096 and
    every tile walks the descriptor chain. One run per path."""
    n = 300 * TILE + 1
    pats = patterns(n, seed=300, sawtooth_bytes=())
    for label, run in (("onesweep", soa(True)), ("aos", aos)):
        for name in ("one_digit", "random_narrow"):
            checked(run, pats[name], 0, 64, True, f"{label} {name}")


def test_sort_word_one(hs):
    """Order by bits [48, 64) of the SECOND word of each pair; the first
    word travels with it."""
    for n in (513, 4097, 8193):
        rng = np.random.default_rng(n)
        x = rng.integers(0, U64_MAX, n, dtype=np.uint64, endpoint=True)
        r16 = rng.integers(0, 1 << 16, n, dtype=np.uint64)
        y = r16 << np.uint64(48) | np.arange(n, dtype=np.uint64)
        pairs_np = np.empty(2 * n, dtype=np.uint64)
        pairs_np[0::2], pairs_np[1::2] = x, y
        pairs = dev(pairs_np)
        tmp = Guarded(2 * n, torch.int64, 0x5A5A5A5A5A5A5A5A)
        ws = Guarded(hs.onesweep_workspace_bytes(n, 2), torch.uint8, 0xA5)
        res = hs.onesweep_sort_aos_u64(
            pairs.data_ptr(), tmp.inner.data_ptr(), n, 48, 64,
            ws.inner.data_ptr(), torch.cuda.current_stream().cuda_stream,
            sort_word=1)
        assert res == 0, "two passes end in the input buffer"
        out = host(pairs).view(np.uint64)
        tmp.check(f"tmp n={n}")
        ws.check(f"ws n={n}")
        order = np.argsort(r16, kind="stable")
        assert np.array_equal(out[1::2], y[order]), f"n={n}: second words"
        assert np.array_equal(out[0::2], x[order]), f"n={n}: first words"


# ---------------------------------------------------------------------------
# partition, every instantiation

PART_N = (1, 64, 65, 4095, 4096, 4097, 64 * TILE + 1)


def _partition_patterns(n, shift, nbits):
    pats = patterns(n, seed=n + nbits, sawtooth_bytes=())
    i = np.arange(n, dtype=np.uint64)
    saw = (i % np.uint64(1 << nbits)) << np.uint64(shift)
    return (("zeros", pats["zeros"]), ("one_digit", pats["one_digit"]),
            ("sawtooth", saw), ("random_u64", pats["random_u64"]))


def test_partition_default_shift_every_nbits(hs):
    """nbits 1..12 as the top bits of the key. 1..3 run the 4-bit kernel,
    whose extra mask bits read the zeros shifted in above bit 63."""
    for nbits in range(1, 13):
        for n in PART_N:
            for name, k in _partition_patterns(n, 64 - nbits, nbits):
                _partition_check(k, True, nbits, label=name)


def test_partition_explicit_shifts(hs):
    for nbits in range(4, 13):
        for shift in (0, 13):
            for n in PART_N:
                for name, k in _partition_patterns(n, shift, nbits):
                    _partition_check(k, True, nbits, shift, label=name)
        # the default written out, once per nbits
        k = _partition_patterns(4097, 64 - nbits, nbits)[3][1]
        _partition_check(k, True, nbits, 64 - nbits, label="random_u64")


PART_SUBSET = ((1, None), (3, None), (4, None), (8, None), (12, None),
               (8, 0), (12, 13), (5, 13))


def test_partition_aos(hs):
    from sparkrdma_amd.ops.radix import partition_aos
    for nbits, shift in PART_SUBSET:
        sh = 64 - nbits if shift is None else shift
        for n in (65, 4097, 2 * TILE + 1):
            for name, k in _partition_patterns(n, sh, nbits)[2:]:
                vd = torch.arange(n, dtype=torch.int64, device="cuda")
                counts, pairs = partition_aos(dev(k), vd, nbits, shift)
                want_counts, order = expect_partition(k, sh, nbits)
                where = f"{name} n={n} nbits={nbits} shift={shift}"
                assert np.array_equal(host(counts).astype(np.int64),
                                      want_counts), where
                out = host(pairs)
                assert np.array_equal(out[0::2].view(np.uint64), k[order]), \
                    where
                assert np.array_equal(out[1::2], order), where


def test_partition_records(hs):
    from sparkrdma_amd.ops.radix import partition_records
    W = 24
    for nbits, shift in PART_SUBSET:
        sh = 64 - nbits if shift is None else shift
        for n in (65, 4097, 2 * TILE + 1):
            for name, k in _partition_patterns(n, sh, nbits)[2:]:
                rec = np.zeros((n, W // 8), dtype="<u8")
                rec[:, 0] = k                       # key prefix, LE
                rec[:, 1] = np.arange(n)            # names the source row
                rec[:, 2] = ~k
                recs = torch.from_numpy(rec.view(np.uint8).reshape(-1)).cuda()
                counts, grouped = partition_records(recs, W, key_bytes=8,
                                                    nbits=nbits, shift=shift)
                want_counts, order = expect_partition(k, sh, nbits)
                where = f"{name} n={n} nbits={nbits} shift={shift}"
                assert counts.shape == (1 << nbits,), where
                assert np.array_equal(counts, want_counts), where
                got = host(grouped).view("<u8").reshape(n, W // 8)
                assert np.array_equal(got, rec[order]), where


def test_small_nbits_with_a_shift_is_rejected(hs, monkeypatch):
    """nbits < 4 anywhere but at the top of the key would be binned by the
    4-bit kernel's 4 bits: ValueError, and nothing is launched."""
    from sparkrdma_amd.ops import radix
    n = 4097
    k = patterns(n, seed=10, sawtooth_bytes=())["random_u64"]
    kd = dev(k)
    vd = torch.arange(n, dtype=torch.int64, device="cuda")
    recs = torch.zeros(n * 24, dtype=torch.uint8, device="cuda")
    # a destination for every digit of the 4-bit kernel, patterned
    arena_k = torch.full((n,), 0x77, dtype=torch.int64, device="cuda")
    arena_v = torch.full((n,), 0x77, dtype=torch.int64, device="cuda")
    key_dst = torch.full((16,), arena_k.data_ptr(), dtype=torch.int64,
                         device="cuda")
    val_dst = torch.full((16,), arena_v.data_ptr(), dtype=torch.int64,
                         device="cuda")
    keys_before, vals_before = kd.clone(), vd.clone()
    torch.cuda.synchronize()

    def no_native_call(*a, **kw):
        raise AssertionError("the native module was reached")
    monkeypatch.setattr(radix, "load", no_native_call)
    for nbits in (1, 2, 3):
        with pytest.raises(ValueError, match="nbits"):
            radix.radix_partition(kd, vd, nbits, shift=10, key_dst=key_dst,
                                  val_dst=val_dst)
        with pytest.raises(ValueError, match="nbits"):
            radix.radix_partition(kd, None, nbits, shift=10)
        with pytest.raises(ValueError, match="nbits"):
            radix.partition_aos(kd, vd, nbits, shift=10)
        with pytest.raises(ValueError, match="nbits"):
            radix.partition_records(recs, 24, nbits=nbits, shift=10)
    torch.cuda.synchronize()
    assert bool((arena_k == 0x77).all()) and bool((arena_v == 0x77).all())
    assert torch.equal(kd, keys_before) and torch.equal(vd, vals_before)
