"""SQL sort-merge join — BASELINE config 5 (1B x 1B rows on 8 GPUs).

Two synthetic tables of (key u64, payload u64) rows. One step:

  1. shuffle table A by key range into R global partitions (GPU radix
     partition straight into HBM blocks)
  2. shuffle table B likewise (second shuffle)
  3. per owned partition: radix-sort both sides over the low bits, then
     the hand-written merge kernel (join_count/join_emit) produces the
     matched pairs

Keys are drawn from a shared space so a controllable fraction matches;
validation checks the exact match count against a CPU oracle.

``how`` picks the join type (joins.JOIN_TYPES). The default inner join runs
the join_count/join_emit pair above; every other type, and inner when
``kernel="family"`` asks for it, runs the join family (ops/join.py
merge_join on the GPU lane, joins.merge_join_np on the CPU lane) and also
counts the rows only one side has.
"""

from __future__ import annotations

import time
from dataclasses import dataclass
from typing import Optional

import numpy as np

from ..engine import Engine
from ..joins import check_join_type
from ..partitioner import RangePartitioner


@dataclass
class JoinResult:
    seconds: float
    rows_a: int
    rows_b: int
    matches: int            # matched rows; left_semi: rows emitted
    shuffle_bytes: int
    how: str = "inner"
    left_only: int = 0      # rows of A null-extended (left_anti: emitted)
    right_only: int = 0     # rows of B null-extended


class SortMergeJoin:
    KERNELS = ("sorted", "family")

    def __init__(self, engine: Engine, rows_per_executor: int,
                 partitions_per_executor: int = 64, device: str = "cpu",
                 key_space_bits: int = 32, validate: bool = False,
                 seed: int = 0, how: str = "inner",
                 kernel: Optional[str] = None):
        check_join_type(how)
        if kernel is None:
            kernel = "sorted" if how == "inner" else "family"
        if kernel not in self.KERNELS:
            raise ValueError(f"unknown kernel {kernel!r}; "
                             f"expected one of {self.KERNELS}")
        if kernel == "sorted" and how != "inner":
            raise ValueError("kernel='sorted' joins inner only")
        self.how = how
        self.kernel = kernel
        self.engine = engine
        self.n = rows_per_executor
        self.device = device
        self.validate = validate
        W = engine.world_size
        R = W * partitions_per_executor
        if R & (R - 1):
            raise ValueError("total partitions must be pow2")
        self.R = R
        self.ppe = partitions_per_executor
        self.key_bits = key_space_bits
        self.part = RangePartitioner.uniform(
            R, key_min=0, key_max=(1 << key_space_bits) - 1)
        self.low_bits = key_space_bits - (R - 1).bit_length()
        rank = engine.rank
        rng = np.random.default_rng(seed * 31 + rank)
        ka = rng.integers(0, 1 << key_space_bits, self.n, dtype=np.uint64)
        kb = rng.integers(0, 1 << key_space_bits, self.n, dtype=np.uint64)
        if device == "cuda":
            import torch
            self.a_keys = torch.from_numpy(ka.view(np.int64)).cuda()
            self.b_keys = torch.from_numpy(kb.view(np.int64)).cuda()
            self.a_vals = self.a_keys.clone()   # payload := key (checkable)
            self.b_vals = self.b_keys.clone()
        else:
            self.a_keys, self.b_keys = ka, kb
            self.a_vals = ka.view(np.uint8).reshape(-1, 8).copy()
            self.b_vals = kb.view(np.uint8).reshape(-1, 8).copy()

    def _shuffle_sorted(self, keys, vals):
        """One table's shuffle, consumed through the reader's GENERIC
        ordering hookup (read_aos(ordering=True) — the shared
        deserialize->sort path, RdmaShuffleReader.scala:61-114 role):
        returns (handle, sorted keys, sorted vals, metrics)."""
        eng = self.engine
        handle = eng.register_shuffle(eng.world_size, self.R)
        w = eng.manager.get_writer(handle, eng.rank)
        if self.device == "cuda":
            w.write_device_batch(keys, vals)
        else:
            w.write_batch(keys, vals)
        w.stop(True, partitioner=self.part)
        eng.barrier()
        lo, hi = eng.rank * self.ppe, (eng.rank + 1) * self.ppe - 1
        arena_hint = None
        if self.device == "cuda":
            import torch
            cap = int(self.n * 16 * 1.25) + (64 << 10)
            self._arena_pool = getattr(self, "_arena_pool", [])
            for t in self._arena_pool:
                if not getattr(t, "_in_use", False) and t.numel() >= cap:
                    arena_hint = t
                    break
            if arena_hint is None:
                arena_hint = torch.empty(cap, dtype=torch.uint8,
                                         device="cuda")
                self._arena_pool.append(arena_hint)
            # table A's data must survive table B's shuffle
            arena_hint._in_use = True
        reader = eng.manager.get_reader(handle, lo, hi, arena=arena_hint)
        # the owned partition range shares its top log2(W) key bits, so
        # ONE batched sort over the low bits fully orders each side
        wbits = (eng.world_size - 1).bit_length()
        k, v = reader.read_aos(ordering=True,
                               end_bit=self.key_bits - wbits)
        return handle, k, v, reader.metrics

    def _join_family(self, ak, av, bk, bv):
        """(matches, left_only, right_only) of the family join of the two
        sorted sides. Payload equals key in this workload, so validation
        also checks every payload slot: the key where valid, 0 where null."""
        if self.device == "cuda":
            from ..ops.join import merge_join
            out = merge_join(ak.contiguous(), av.contiguous(),
                             bk.contiguous(), bv.contiguous(), how=self.how)
        else:
            from ..joins import merge_join_np
            out = merge_join_np(ak, av, bk, bv, self.how)
        rows = len(out.keys)
        if out.b_valid is None:
            counts = (rows, 0, 0) if self.how == "left_semi" else (0, rows, 0)
        else:
            a_ok, b_ok = out.a_valid, out.b_valid
            counts = (int((a_ok & b_ok).sum()), int((a_ok & ~b_ok).sum()),
                      int((~a_ok & b_ok).sum()))
            assert sum(counts) == rows, "a row with both sides null"
        if self.validate:
            for vals, ok, side in ((out.a_vals, out.a_valid, "a"),
                                   (out.b_vals, out.b_valid, "b")):
                if vals is None:
                    continue
                assert bool((vals[ok] == out.keys[ok]).all()), \
                    f"joined {side} payloads must equal keys"
                assert bool((vals[~ok] == 0).all()), \
                    f"null {side} payloads must be 0"
        return counts

    def run_step(self) -> JoinResult:
        if self.kernel == "family":
            return self._run_step_family()
        eng = self.engine
        t0 = time.perf_counter()
        ha, ak, av, ma = self._shuffle_sorted(self.a_keys, self.a_vals)
        hb, bk, bv, mb = self._shuffle_sorted(self.b_keys, self.b_vals)
        matches = 0
        if self.device == "cuda":
            import torch
            from ..ops.join import merge_join_sorted
            if ak.numel() and bk.numel():
                jk, ja, jb = merge_join_sorted(
                    ak.contiguous(), av.contiguous(),
                    bk.contiguous(), bv.contiguous())
                matches += jk.numel()
                if self.validate and jk.numel():
                    assert torch.equal(jk, ja) and torch.equal(jk, jb), \
                        "joined payloads must equal keys"
            torch.cuda.synchronize()
        elif len(ak) and len(bk):
            lo = np.searchsorted(bk, ak, side="left")
            hi = np.searchsorted(bk, ak, side="right")
            matches += int((hi - lo).sum())
        eng.unregister_shuffle(ha)
        eng.unregister_shuffle(hb)
        for t in getattr(self, "_arena_pool", []):
            t._in_use = False
        dt = time.perf_counter() - t0
        if self.validate:
            self._validate_counts(matches)
        return JoinResult(dt, self.n, self.n, matches,
                          ma.remote_bytes_read + mb.remote_bytes_read)

    def _run_step_family(self) -> JoinResult:
        eng = self.engine
        t0 = time.perf_counter()
        ha, ak, av, ma = self._shuffle_sorted(self.a_keys, self.a_vals)
        hb, bk, bv, mb = self._shuffle_sorted(self.b_keys, self.b_vals)
        counts = self._join_family(ak, av, bk, bv)
        if self.device == "cuda":
            import torch
            torch.cuda.synchronize()
        eng.unregister_shuffle(ha)
        eng.unregister_shuffle(hb)
        for t in getattr(self, "_arena_pool", []):
            t._in_use = False
        dt = time.perf_counter() - t0
        if self.validate:
            self._validate_family(counts)
        return JoinResult(dt, self.n, self.n, counts[0],
                          ma.remote_bytes_read + mb.remote_bytes_read,
                          self.how, counts[1], counts[2])

    def _validate_family(self, counts) -> None:
        """(matches, left_only, right_only) against a searchsorted oracle
        over the original inputs; single-process only, as below."""
        if self.engine.world_size != 1:
            return
        if self.device == "cuda":
            ka = self.a_keys.cpu().numpy().view(np.uint64)
            kb = self.b_keys.cpu().numpy().view(np.uint64)
        else:
            ka, kb = self.a_keys, self.b_keys
        sa, sb = np.sort(ka), np.sort(kb)
        m_a = np.searchsorted(sb, ka, "right") - np.searchsorted(sb, ka, "left")
        m_b = np.searchsorted(sa, kb, "right") - np.searchsorted(sa, kb, "left")
        pairs, a_only, b_only = (int(m_a.sum()), int((m_a == 0).sum()),
                                 int((m_b == 0).sum()))
        want = {"inner": (pairs, 0, 0),
                "left_outer": (pairs, a_only, 0),
                "right_outer": (pairs, 0, b_only),
                "full_outer": (pairs, a_only, b_only),
                "left_semi": (int((m_a > 0).sum()), 0, 0),
                "left_anti": (0, a_only, 0)}[self.how]
        assert tuple(counts) == want, \
            f"{self.how} join counts {tuple(counts)} != oracle {want}"

    def _validate_counts(self, matches: int) -> None:
        """Local-count oracle only works single-process; multi-rank runs
        validate via all-rank sum equality in the caller."""
        if self.engine.world_size != 1:
            return
        if self.device == "cuda":
            ka = self.a_keys.cpu().numpy().view(np.uint64)
            kb = self.b_keys.cpu().numpy().view(np.uint64)
        else:
            ka, kb = self.a_keys, self.b_keys
        bs = np.sort(kb)
        want = int((np.searchsorted(bs, ka, "right")
                    - np.searchsorted(bs, ka, "left")).sum())
        assert matches == want, f"join matches {matches} != oracle {want}"
