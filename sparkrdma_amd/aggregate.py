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
