"""Join types of the sort-merge join family and their numpy mirror.

Spark's sort-merge join, which the reference plugin's reducers serve, runs
inner, left / right / full outer, left semi and left anti joins. The device
path is ``ops/join.py::merge_join`` (ops/csrc/join.hip); ``merge_join_np``
computes the same rows in the same order on the host: the CPU lane of the
sql_join workload, and the oracle the device path is tested against.

Semantics shared by both:

* keys compare as unsigned 64-bit; both sides are sorted by key
* rows come in order of the driving side's row number (A, or B for
  ``right_outer``), and within one driving row in order of the other side's
  row number; ``full_outer`` appends the rows only B has, in B order
* a null slot has validity False, value 0 and index -1; the key of a row
  only B has is B's key
* ``left_semi`` / ``left_anti`` return rows of A only: every ``b_*`` field
  is None
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Optional

import numpy as np

JOIN_TYPES = ("inner", "left_outer", "right_outer", "full_outer",
              "left_semi", "left_anti")


def check_join_type(how: str) -> None:
    if how not in JOIN_TYPES:
        raise ValueError(f"unknown join type {how!r}; "
                         f"expected one of {JOIN_TYPES}")


@dataclass
class JoinOutput:
    """SoA join result. ``*_vals`` is None when the input payload was None,
    ``*_idx`` (int64 input row numbers) unless ``indices=True``."""
    keys: Any
    a_vals: Optional[Any]
    b_vals: Optional[Any]
    a_valid: Any
    b_valid: Optional[Any]
    a_idx: Optional[Any] = None
    b_idx: Optional[Any] = None


def row_counts(m, how: str):
    """Output rows of each driving row from its match count ``m`` (numpy
    array or torch tensor); ``full_outer`` counts its left-outer part."""
    if how == "inner":
        return m
    if how in ("left_outer", "right_outer", "full_outer"):
        return m.clip(1)
    if how == "left_semi":
        return m > 0
    return m == 0


def _as_u64(k: np.ndarray, what: str) -> np.ndarray:
    k = np.asarray(k)
    if k.ndim != 1 or k.dtype not in (np.uint64, np.int64):
        raise ValueError(f"{what} must be a 1-D uint64 or int64 array")
    return k.view(np.uint64)


def _expand_np(pk, qk, how):
    """(p_idx, q_idx) of the rows P drives; q_idx is -1 in null slots."""
    lo = np.searchsorted(qk, pk, side="left").astype(np.int64)
    m = np.searchsorted(qk, pk, side="right").astype(np.int64) - lo
    cnt = np.asarray(row_counts(m, how), dtype=np.int64)
    offsets = np.cumsum(cnt) - cnt
    p_idx = np.repeat(np.arange(len(pk), dtype=np.int64), cnt)
    j = np.arange(len(p_idx), dtype=np.int64) - offsets[p_idx]
    q_idx = np.where(m[p_idx] > 0, lo[p_idx] + j, -1)
    return p_idx, q_idx


def _take(vals, idx):
    """vals[idx] with 0 where idx == -1; None stays None."""
    if vals is None:
        return None
    vals = np.asarray(vals)
    out = np.zeros(len(idx), dtype=vals.dtype)
    ok = idx >= 0
    out[ok] = vals[idx[ok]]
    return out


def merge_join_np(a_keys, a_vals, b_keys, b_vals, how: str = "inner",
                  indices: bool = False) -> JoinOutput:
    """Numpy mirror of ``ops.join.merge_join``: the same rows in the same
    order. Keys are 1-D uint64 (or int64 holding the same bits), sorted as
    unsigned; payloads are 1-D arrays of the keys' length or None."""
    check_join_type(how)
    ak, bk = _as_u64(a_keys, "a_keys"), _as_u64(b_keys, "b_keys")
    for v, k, what in ((a_vals, ak, "a_vals"), (b_vals, bk, "b_vals")):
        if v is not None and np.shape(v) != k.shape:
            raise ValueError(f"{what} must match its keys' shape")
    if how == "right_outer":
        b_idx, a_idx = _expand_np(bk, ak, how)
    elif how == "full_outer":
        a_idx, b_idx = _expand_np(ak, bk, how)
        only_b, _ = _expand_np(bk, ak, "left_anti")
        a_idx = np.concatenate((a_idx, np.full(len(only_b), -1, np.int64)))
        b_idx = np.concatenate((b_idx, only_b))
    else:
        a_idx, b_idx = _expand_np(ak, bk, how)
    a_valid = a_idx >= 0
    keys = np.where(a_valid, _take(ak, a_idx), _take(bk, b_idx))
    keys = keys.astype(np.uint64).view(np.asarray(a_keys).dtype)
    if how in ("left_semi", "left_anti"):
        return JoinOutput(keys, _take(a_vals, a_idx), None, a_valid, None,
                          a_idx if indices else None, None)
    return JoinOutput(keys, _take(a_vals, a_idx), _take(b_vals, b_idx),
                      a_valid, b_idx >= 0,
                      a_idx if indices else None,
                      b_idx if indices else None)
