"""Wire format of the variable-length record lane, shared by the CPU and
GPU write and read paths.

A row is a u64 key plus a payload of any length, zero included. Batches of
rows travel as ``(keys, offsets, data)`` in the CSR / Arrow binary layout:
``offsets`` has ``n + 1`` int64 entries, ``offsets[0] == 0``, and row ``r``
is ``data[offsets[r]:offsets[r + 1]]``.

One (map, partition) segment with ``n > 0`` rows and ``H`` payload bytes::

    [u64 n][u64 H]                    16-byte header
    n x [u64 key][u64 end]            end = exclusive end offset of the row's
                                      payload inside this segment's heap
                                      (row r starts at end[r-1], row 0 at 0)
    H payload bytes, back to back     no per-row padding
    zero padding to a multiple of 16 bytes

All words are little-endian. A partition without rows is a zero-length
location-table entry, as on every other lane; ``pack_varlen_segment`` of no
rows is ``b""``. Segment lengths are multiples of 16, pool blocks are
16 KiB-aligned and the groups of ``writer.group_partitions`` are packed back
to back, so every segment starts 16-byte aligned; a partition is never
split across blocks, so a fetched block is exactly one segment.

The functions here are numpy only: they are the CPU lane, and the oracle of
the GPU lane's tests (ops/csrc/varlen.hip moves the same bytes on the GPU).
"""

from __future__ import annotations

from typing import List, Tuple

import numpy as np

HEADER_BYTES = 16
INDEX_ENTRY_BYTES = 16
ALIGN = 16


def segment_bytes(n: int, heap_bytes: int) -> int:
    """Length of a segment of ``n`` rows and ``heap_bytes`` payload bytes."""
    if n == 0:
        return 0
    raw = HEADER_BYTES + INDEX_ENTRY_BYTES * n + heap_bytes
    return -(-raw // ALIGN) * ALIGN


def check_offsets(offsets: np.ndarray, n: int, data_len: int) -> None:
    """Raise ValueError unless ``offsets`` describes n rows inside
    ``data_len`` bytes."""
    if len(offsets) != n + 1:
        raise ValueError(f"offsets has {len(offsets)} entries for {n} keys, "
                         f"expected {n + 1}")
    if offsets[0] != 0:
        raise ValueError("offsets[0] must be 0")
    if n and bool(np.any(offsets[1:] < offsets[:-1])):
        raise ValueError("offsets must be non-decreasing")
    if offsets[-1] > data_len:
        raise ValueError(f"offsets[-1] = {int(offsets[-1])} exceeds the "
                         f"{data_len} data bytes")


def _as_rows(keys, offsets, data) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    keys = np.ascontiguousarray(keys).astype("<u8", copy=False).reshape(-1)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
    data = np.ascontiguousarray(data, dtype=np.uint8).reshape(-1)
    check_offsets(offsets, len(keys), len(data))
    return keys, offsets, data


def pack_varlen_segment(keys, offsets, data) -> bytes:
    """The segment of rows ``(keys, offsets, data)``; ``b""`` for no rows.
    Only ``data[:offsets[-1]]`` is payload."""
    keys, offsets, data = _as_rows(keys, offsets, data)
    n = len(keys)
    if n == 0:
        return b""
    heap = int(offsets[-1])
    out = np.zeros(segment_bytes(n, heap), dtype=np.uint8)
    words = out[:HEADER_BYTES + INDEX_ENTRY_BYTES * n].view("<u8")
    words[0] = n
    words[1] = heap
    words[2::2] = keys
    words[3::2] = offsets[1:].astype("<u8")
    out[HEADER_BYTES + INDEX_ENTRY_BYTES * n:][:heap] = data[:heap]
    return out.tobytes()


def unpack_varlen_segment(buf) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """``(keys u64[n], offsets int64[n + 1], data uint8[H])`` of one
    segment; the arrays are copies. A zero-length buffer has no rows.
    Raises ValueError for a buffer that is not a well-formed segment."""
    raw = np.frombuffer(buf, dtype=np.uint8)
    if len(raw) == 0:
        return (np.empty(0, dtype=np.uint64), np.zeros(1, dtype=np.int64),
                np.empty(0, dtype=np.uint8))
    if len(raw) < HEADER_BYTES or len(raw) % ALIGN:
        raise ValueError(f"a segment of {len(raw)} bytes is not a multiple "
                         f"of {ALIGN}")
    n, heap = (int(x) for x in raw[:HEADER_BYTES].view("<u8"))
    if n == 0 or segment_bytes(n, heap) != len(raw):
        raise ValueError(f"segment header (n={n}, H={heap}) does not match "
                         f"its length {len(raw)}")
    index = raw[HEADER_BYTES:HEADER_BYTES + INDEX_ENTRY_BYTES * n].view("<u8")
    keys = index[0::2].astype(np.uint64)
    offsets = np.zeros(n + 1, dtype=np.int64)
    offsets[1:] = index[1::2].astype(np.int64)
    if offsets[-1] != heap or bool(np.any(offsets[1:] < offsets[:-1])):
        raise ValueError("segment index is not a non-decreasing scan that "
                         "ends at H")
    start = HEADER_BYTES + INDEX_ENTRY_BYTES * n
    return keys, offsets, raw[start:start + heap].copy()


def take_rows(offsets: np.ndarray, data: np.ndarray, order: np.ndarray
              ) -> Tuple[np.ndarray, np.ndarray]:
    """Rows ``order`` of ``(offsets, data)`` as a fresh ``(offsets, data)``
    with the payloads back to back in that order."""
    lens = (offsets[1:] - offsets[:-1])[order]
    out_off = np.zeros(len(order) + 1, dtype=np.int64)
    np.cumsum(lens, out=out_off[1:])
    total = int(out_off[-1])
    # byte j of the output lies in output row searchsorted(out_off, j) - 1
    row = np.repeat(np.arange(len(order)), lens)
    src = offsets[:-1][order][row] + (np.arange(total) - out_off[:-1][row])
    return out_off, data[src]


def partition_varlen_np(keys, offsets, data, pids, R: int) -> List[bytes]:
    """Stable numpy mirror of the GPU write path: the R segments of rows
    ``(keys, offsets, data)`` whose partition ids are ``pids``; rows keep
    their input order inside a partition."""
    keys, offsets, data = _as_rows(keys, offsets, data)
    pids = np.asarray(pids).astype(np.int64).reshape(-1)
    if len(pids) != len(keys):
        raise ValueError("pids/keys length mismatch")
    if len(pids) and (pids.min() < 0 or pids.max() >= R):
        raise ValueError(f"partition id outside [0, {R})")
    order = np.argsort(pids, kind="stable")
    g_off, g_data = take_rows(offsets, data, order)
    g_keys = keys[order]
    counts = np.bincount(pids, minlength=R)
    ends = np.cumsum(counts)
    out = []
    for p in range(R):
        a, b = int(ends[p] - counts[p]), int(ends[p])
        out.append(pack_varlen_segment(
            g_keys[a:b], g_off[a:b + 1] - g_off[a],
            g_data[int(g_off[a]):int(g_off[b])]))
    return out


def concat_rows(parts) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Concatenate ``(keys, offsets, data)`` triples into one."""
    parts = [p for p in parts if len(p[0])]
    if not parts:
        return (np.empty(0, dtype=np.uint64), np.zeros(1, dtype=np.int64),
                np.empty(0, dtype=np.uint8))
    keys = np.concatenate([p[0] for p in parts])
    data = np.concatenate([p[2][:int(p[1][-1])] for p in parts])
    offsets = np.zeros(len(keys) + 1, dtype=np.int64)
    np.cumsum(np.concatenate([np.diff(p[1]) for p in parts]),
              out=offsets[1:])
    return keys, offsets, data
