"""Named keyed reductions shared by both sides of the shuffle.

The reference reader has two aggregation branches
(RdmaShuffleReader.scala:83-96): ``combineValuesByKey`` over raw rows and
``combineCombinersByKey`` when the map side already combined. A map-side
combine collapses each map task's rows to one per key; the reduce side then
MERGES those partial results, which for ``count`` is a sum and for every
other aggregator is the aggregator itself.
"""

from __future__ import annotations

import numpy as np

#: ShuffleReader.AGGREGATORS; the index is the reduce_by_key kernel's op code
AGGREGATORS = ("sum", "sum_f64", "count", "min", "max")

#: aggregator -> the reduction that merges its partial results
MERGE_OF = {"sum": "sum", "sum_f64": "sum_f64", "count": "sum",
            "min": "min", "max": "max"}


def check_aggregator(name: str, what: str = "aggregator") -> None:
    if name not in AGGREGATORS:
        raise ValueError(f"unknown {what} {name!r}; "
                         f"expected one of {AGGREGATORS}")


def reduce_sorted_np(k: np.ndarray, v: np.ndarray, op: str):
    """CPU mirror of the reduce_by_key kernel: ``k`` (u64) has equal keys
    adjacent, ``v`` (u64) rides along. Returns (run keys, reductions) in
    input order. min/max compare the u64 payload as the CPU lane of
    read_aos always has."""
    if len(k) == 0:
        return k, v
    start = np.flatnonzero(np.concatenate(([True], k[1:] != k[:-1])))
    uk = k[start]
    if op == "count":
        return uk, np.diff(np.append(start, len(k)))
    if op == "sum":
        return uk, np.add.reduceat(v, start)
    if op == "sum_f64":
        return uk, np.add.reduceat(v.view(np.float64), start)
    fn = np.minimum if op == "min" else np.maximum
    return uk, fn.reduceat(v, start)


# ---------------------------------------------------------------------------
# Several typed columns of wide records reduced per key (the GROUP BY of the
# record lane): ops/csrc/reduce_records.hip on the GPU, reduce_records_np here.

#: column dtypes; the index is the kernel's type code
COLUMN_DTYPES = ("i32", "u32", "i64", "f32", "f64")
#: column ops; the index is the kernel's op code
COLUMN_OPS = ("sum", "min", "max", "count")
#: most columns one call reduces (reduce_records_max_columns())
MAX_COLUMNS = 8

_COLUMN_NP = {"i32": "<i4", "u32": "<u4", "i64": "<i8", "f32": "<f4",
              "f64": "<f8"}


def check_columns(columns, rec_bytes: int):
    """Validate ``columns`` = a sequence of ``(offset_bytes, dtype, op)``
    against ``rec_bytes``-byte records; return them as a list of
    ``(offset_bytes, type code, op code)``. dtype is one of COLUMN_DTYPES,
    op one of COLUMN_OPS; "count" ignores offset and dtype (both may be
    None) and comes back as ``(0, code of "i64", code of "count")``.

    The dtype decides the accumulator: integer columns reduce as int64
    (i32 sign-, u32 zero-extended), float columns as float64."""
    if rec_bytes <= 0 or rec_bytes % 4:
        raise ValueError(f"rec_bytes must be a positive multiple of 4, "
                         f"got {rec_bytes}")
    columns = list(columns)
    if not 1 <= len(columns) <= MAX_COLUMNS:
        raise ValueError(f"{len(columns)} columns; one call reduces 1 to "
                         f"{MAX_COLUMNS}")
    out = []
    for i, col in enumerate(columns):
        try:
            off, dtype, op = col
        except (TypeError, ValueError):
            raise ValueError(f"column {i}: expected (offset_bytes, dtype, "
                             f"op), got {col!r}") from None
        if op not in COLUMN_OPS:
            raise ValueError(f"column {i}: unknown op {op!r}; expected one "
                             f"of {COLUMN_OPS}")
        if op == "count":
            out.append((0, COLUMN_DTYPES.index("i64"),
                        COLUMN_OPS.index("count")))
            continue
        if dtype not in COLUMN_DTYPES:
            raise ValueError(f"column {i}: unknown dtype {dtype!r}; "
                             f"expected one of {COLUMN_DTYPES}")
        if not isinstance(off, (int, np.integer)) or off < 0 or off % 4:
            raise ValueError(f"column {i}: offset {off!r} is not a "
                             f"non-negative multiple of 4")
        size = np.dtype(_COLUMN_NP[dtype]).itemsize
        if off + size > rec_bytes:
            raise ValueError(f"column {i}: bytes [{off}, {off + size}) reach "
                             f"past the {rec_bytes}-byte record")
        out.append((int(off), COLUMN_DTYPES.index(dtype),
                    COLUMN_OPS.index(op)))
    return out


def column_is_float(type_code: int, op_code: int) -> bool:
    """Does a checked column come back as float64 (else int64)?"""
    return (COLUMN_OPS[op_code] != "count"
            and COLUMN_DTYPES[type_code] in ("f32", "f64"))


def reduce_records_np(recs: np.ndarray, columns, end_bit: int = 64):
    """CPU mirror of ops.radix.aggregate_records. ``recs`` is uint8 [n, W]:
    AoS records with a u64 LE key at offset 0. Stable argsort by the key
    bits [0, end_bit), then one reduceat per column with the kernel's
    widening. Returns ``(keys int64[g], [one array[g] per column])``, keys
    ascending, a column float64 for f32 / f64 dtypes and int64 otherwise
    (sums wrap mod 2^64). Rows whose keys agree in the window must agree
    everywhere, as for every ``end_bit`` of this package."""
    recs = np.ascontiguousarray(recs, dtype=np.uint8)
    if recs.ndim != 2:
        raise ValueError("recs must be uint8 [n, W]")
    n, W = recs.shape
    if W < 8:
        raise ValueError("records hold a u64 key: W >= 8")
    cols = check_columns(columns, W)
    if not 1 <= end_bit <= 64:
        raise ValueError("end_bit must be in [1, 64]")
    if n == 0:
        return (np.empty(0, np.int64),
                [np.empty(0, np.float64 if column_is_float(t, o)
                          else np.int64) for _off, t, o in cols])
    k = recs[:, :8].copy().view("<u8").reshape(n)
    mask = np.uint64((1 << end_bit) - 1)
    order = np.argsort(k & mask, kind="stable")
    k = k[order]
    start = np.flatnonzero(np.concatenate(([True], k[1:] != k[:-1])))
    vals = []
    for off, t, o in cols:
        op = COLUMN_OPS[o]
        if op == "count":
            vals.append(np.diff(np.append(start, n)).astype(np.int64))
            continue
        nd = np.dtype(_COLUMN_NP[COLUMN_DTYPES[t]])
        v = recs[:, off:off + nd.itemsize].copy().view(nd).reshape(n)[order]
        v = v.astype(np.float64 if column_is_float(t, o) else np.int64)
        fn = {"sum": np.add, "min": np.minimum, "max": np.maximum}[op]
        with np.errstate(over="ignore"):
            vals.append(fn.reduceat(v, start))
    return k[start].view(np.int64), vals
