"""Sorted-merge join on device (u64 keys, u64 payloads).

Both inputs must be sorted by key (use radix.sort_pairs).

``merge_join_sorted`` is the inner join of the join_count / join_emit
kernels: returns (keys, a_payloads, b_payloads) of all matching pairs.

``merge_join`` is the join family of ops/csrc/join.hip: the six join types
of ``joins.JOIN_TYPES``, validity masks for null-extended rows, and
optionally the input row numbers of every output row, so that tables wider
than one payload word can be gathered by the caller.
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import load
from ..joins import JOIN_TYPES, JoinOutput, check_join_type, row_counts

__all__ = ["EXPAND_TILE", "EXPAND_LDS_ROWS", "PROBE_LDS_KEYS", "JOIN_TYPES",
           "JoinOutput", "merge_join", "merge_join_sorted"]

#: output rows per block of join_expand_kernel, and the longest range of
#: driving rows whose offsets a block searches in LDS (longer: global)
EXPAND_TILE = 2048
EXPAND_LDS_ROWS = 4096
#: longest window of the searched side that a block of 256 probing rows
#: stages in LDS (longer: searched in global memory)
PROBE_LDS_KEYS = 2048


def merge_join_sorted(a_keys: torch.Tensor, a_vals: Optional[torch.Tensor],
                      b_keys: torch.Tensor, b_vals: torch.Tensor
                      ) -> Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor]:
    m = load()
    na, nb = a_keys.numel(), b_keys.numel()
    dev = a_keys.device
    s = torch.cuda.current_stream().cuda_stream
    if na == 0 or nb == 0:
        empty = torch.empty(0, dtype=torch.int64, device=dev)
        return empty, (empty if a_vals is not None else None), empty.clone()
    counts = torch.empty(na, dtype=torch.int32, device=dev)
    lo_idx = torch.empty(na, dtype=torch.int32, device=dev)
    m.join_count(a_keys.data_ptr(), na, b_keys.data_ptr(), nb,
                 counts.data_ptr(), lo_idx.data_ptr(), s)
    counts64 = counts.to(torch.int64)
    offsets = torch.cumsum(counts64, 0) - counts64
    total = int(offsets[-1].item() + counts64[-1].item())
    out_key = torch.empty(total, dtype=torch.int64, device=dev)
    out_a = (torch.empty(total, dtype=torch.int64, device=dev)
             if a_vals is not None else None)
    out_b = torch.empty(total, dtype=torch.int64, device=dev)
    m.join_emit(a_keys.data_ptr(),
                a_vals.data_ptr() if a_vals is not None else 0, na,
                b_vals.data_ptr(), counts.data_ptr(), lo_idx.data_ptr(),
                offsets.data_ptr(), out_key.data_ptr(),
                out_a.data_ptr() if out_a is not None else 0,
                out_b.data_ptr(), s)
    return out_key, out_a, out_b


def _check_side(keys, vals, what: str) -> None:
    for t, name in ((keys, f"{what}_keys"), (vals, f"{what}_vals")):
        if t is None and name.endswith("_vals"):
            continue
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name} must be a torch.Tensor")
        if t.dtype != torch.int64 or t.dim() != 1:
            raise ValueError(f"{name} must be a 1-D int64 tensor "
                             "(u64 bits)")
        if not t.is_cuda:
            raise ValueError(f"{name} must be on the GPU")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
    if keys.numel() >= 1 << 31:
        raise ValueError(f"{what}_keys has 2^31 rows or more")
    if vals is not None and (vals.numel() != keys.numel()
                             or vals.device != keys.device):
        raise ValueError(f"{what}_vals must match {what}_keys in length "
                         "and device")


def _ptr(t: Optional[torch.Tensor]) -> int:
    return t.data_ptr() if t is not None and t.numel() else 0


class _Probe:
    """One side probing the other: lo / m from join_probe_kernel, then the
    per-row output count for ``how`` and its scan, all left on the device.
    ``incl[-1]`` is the side's output total."""

    def __init__(self, mod, pk, qk, how, stream):
        n = pk.numel()
        self.n = n
        self.lo = torch.empty(n, dtype=torch.int32, device=pk.device)
        self.m = torch.empty(n, dtype=torch.int32, device=pk.device)
        mod.join_probe(_ptr(pk), n, _ptr(qk), qk.numel(), _ptr(self.lo),
                       _ptr(self.m), stream)
        cnt = row_counts(self.m, how).to(torch.int64)
        self.incl = torch.cumsum(cnt, 0)
        self.offsets = self.incl - cnt


def merge_join(a_keys: torch.Tensor, a_vals: Optional[torch.Tensor],
               b_keys: torch.Tensor, b_vals: Optional[torch.Tensor],
               how: str = "inner", indices: bool = False) -> JoinOutput:
    """Join two key-sorted tables on the GPU (ops/csrc/join.hip).

    Keys and payloads are contiguous 1-D int64 CUDA tensors holding u64
    bits, fewer than 2^31 rows a side; either payload may be None.
    Sortedness (unsigned) is the caller's contract. Row order, null slots
    and the fields of the result are those of ``joins.merge_join_np``;
    ``a_valid`` / ``b_valid`` are torch.bool. One host synchronisation per
    call, to size the outputs.
    """
    check_join_type(how)
    _check_side(a_keys, a_vals, "a")
    _check_side(b_keys, b_vals, "b")
    if a_keys.device != b_keys.device:
        raise ValueError("a_keys and b_keys must be on the same device")
    if how == "right_outer":
        r = merge_join(b_keys, b_vals, a_keys, a_vals, "left_outer", indices)
        return JoinOutput(r.keys, r.b_vals, r.a_vals, r.b_valid, r.a_valid,
                          r.b_idx, r.a_idx)
    mod = load()
    dev = a_keys.device
    s = torch.cuda.current_stream().cuda_stream
    one_sided = how in ("left_semi", "left_anti")

    # both probes first, then ONE readback of both totals
    pa = _Probe(mod, a_keys, b_keys, how, s) if a_keys.numel() else None
    pb = (_Probe(mod, b_keys, a_keys, "left_anti", s)
          if how == "full_outer" and b_keys.numel() else None)
    live = [p for p in (pa, pb) if p is not None]
    totals = (torch.stack([p.incl[-1] for p in live]).tolist()
              if live else [])
    t1 = totals[0] if pa is not None else 0
    t2 = totals[-1] if pb is not None else 0
    total = t1 + t2

    def i64():
        return torch.empty(total, dtype=torch.int64, device=dev)

    out = JoinOutput(
        keys=i64(),
        a_vals=i64() if a_vals is not None else None,
        b_vals=i64() if b_vals is not None and not one_sided else None,
        a_valid=torch.ones(total, dtype=torch.bool, device=dev),
        b_valid=None if one_sided else
        torch.ones(total, dtype=torch.bool, device=dev),
        a_idx=i64() if indices else None,
        b_idx=i64() if indices and not one_sided else None)
    if t1:
        # inner has no null slot: b_valid stays all true, unwritten
        bvalid = out.b_valid if how in ("left_outer", "full_outer") else None
        bvals_out = out.b_vals
        if bvals_out is not None and b_keys.numel() == 0:
            bvals_out.zero_()       # no B row to read: every slot is null
            bvals_out = None
        mod.join_expand(
            _ptr(a_keys), _ptr(a_vals), _ptr(b_vals), _ptr(pa.lo),
            _ptr(pa.m), _ptr(pa.offsets), pa.n, t1, _ptr(out.keys),
            _ptr(out.a_vals), _ptr(bvals_out),
            _ptr(bvalid.view(torch.uint8)) if bvalid is not None else 0,
            _ptr(out.a_idx), _ptr(out.b_idx), s)
    if t2:
        # rows only B has: B drives an anti expansion into out[t1:], whose
        # A slots are null
        mod.join_expand(
            _ptr(b_keys), _ptr(b_vals), 0, 0, 0, _ptr(pb.offsets), pb.n, t2,
            _ptr(out.keys[t1:]),
            _ptr(out.b_vals[t1:]) if out.b_vals is not None else 0, 0, 0,
            _ptr(out.b_idx[t1:]) if indices else 0, 0, s)
        out.a_valid[t1:] = False
        if out.a_vals is not None:
            out.a_vals[t1:] = 0
        if indices:
            out.a_idx[t1:] = -1
    return out
