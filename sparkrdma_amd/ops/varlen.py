"""Torch-facing wrapper over the variable-length row copy
(ops/csrc/varlen.hip) and the small helpers the write and the read side of
the variable-length lane share. Scans are ``torch.cumsum``: plumbing.

As in ops/radix.py there is no eager fallback: the native extension is
required.
"""

from __future__ import annotations

from typing import Optional

import torch

from . import load

__all__ = ["TILE_BYTES", "LDS_ROWS", "exclusive_scan", "varlen_copy"]

#: destination bytes per block of varlen_copy_kernel, and the most rows of a
#: block's window whose offsets it searches in LDS (more: global memory)
TILE_BYTES = 16384
LDS_ROWS = 4096


def exclusive_scan(lengths: torch.Tensor) -> torch.Tensor:
    """int64[n + 1] with out[0] == 0 and out[r + 1] = sum(lengths[:r + 1])."""
    out = torch.zeros(lengths.numel() + 1, dtype=torch.int64,
                      device=lengths.device)
    torch.cumsum(lengths, 0, out=out[1:])
    return out


def _check(t, name: str, numel: Optional[int] = None) -> None:
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 \
            or t.dim() != 1:
        raise ValueError(f"{name} must be a 1-D int64 tensor")
    if not t.is_cuda:
        raise ValueError(f"{name} must be on the GPU")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if numel is not None and t.numel() != numel:
        raise ValueError(f"{name} has {t.numel()} entries, expected {numel}")


def varlen_copy(cum: torch.Tensor, src_addr: torch.Tensor,
                seg_first_row: torch.Tensor, seg_dst: torch.Tensor,
                total: Optional[int] = None, wide_loads: bool = True) -> int:
    """Copy n rows of different lengths; the work is split by bytes.

    ``cum``: int64[n + 1], exclusive scan of the row lengths in destination
    order (``cum[0] == 0``). ``src_addr``: int64[n], device byte address of
    every row's first byte, any alignment. The destination is S contiguous
    ranges: range s holds rows ``[seg_first_row[s], seg_first_row[s + 1])``
    back to back from device byte address ``seg_dst[s]``
    (``seg_first_row``: int64[S + 1], non-decreasing from 0 to n;
    ``seg_dst``: int64[S], any alignment). No byte outside a range is
    written. Rows of length 0 and empty ranges are allowed; their addresses
    are never used.

    ``total`` is ``cum[n]``; a caller that knows it saves the host
    synchronisation that reads it back. Returns the bytes copied. The
    kernel runs on torch's current stream; the tables must stay alive until
    it has run, which the caching allocator guarantees for tensors freed on
    that stream.
    """
    n = src_addr.numel() if isinstance(src_addr, torch.Tensor) else 0
    _check(src_addr, "src_addr")
    _check(cum, "cum", n + 1)
    _check(seg_first_row, "seg_first_row")
    nseg = seg_first_row.numel() - 1
    if nseg < 0:
        raise ValueError("seg_first_row needs at least one entry")
    _check(seg_dst, "seg_dst", nseg)
    if total is None:
        total = int(cum[-1])                # syncs the stream
    if total == 0:
        return 0
    seg_off = cum[seg_first_row]            # range s takes these bytes
    load().varlen_copy(cum.data_ptr(), src_addr.data_ptr(), n,
                       seg_off.data_ptr(), seg_dst.data_ptr(), nseg, total,
                       torch.cuda.current_stream().cuda_stream,
                       int(wide_loads))
    return total
