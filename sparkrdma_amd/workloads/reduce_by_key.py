"""reduceByKey — the aggregation role of the shuffle reader
(reference RdmaShuffleReader.scala:61-114: deserialize → aggregate),
realized on GPU.

Synthetic (key u64, value u64) pairs with a bounded key space; one step:
hash-partition by splitmix64 (the kernel's hash_mix digit — bit-identical
to HashPartitioner), one-sided shuffle, then per-rank: AoS sort by key
and segmented sum over equal-key runs. Validated against a CPU
dictionary oracle.
"""

from __future__ import annotations

import time
from dataclasses import dataclass

import numpy as np

from ..engine import Engine
from ..partitioner import HashPartitioner


@dataclass
class ReduceByKeyResult:
    seconds: float
    rows: int
    groups: int
    shuffle_bytes: int


class ReduceByKey:
    def __init__(self, engine: Engine, rows_per_executor: int,
                 num_keys: int = 1 << 20, partitions_per_executor: int = 32,
                 device: str = "cpu", validate: bool = False, seed: int = 0,
                 aggregator: str = "sum", map_side_combine: bool = False):
        from ..aggregate import check_aggregator
        check_aggregator(aggregator)
        self.aggregator = aggregator
        self.map_side_combine = map_side_combine
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
        self.part = HashPartitioner(R)
        self.seed = seed
        self.num_keys = num_keys
        rng = np.random.default_rng(seed * 101 + engine.rank)
        k = rng.integers(0, num_keys, self.n, dtype=np.uint64)
        v = rng.integers(0, 1 << 20, self.n, dtype=np.uint64)
        self._k_np, self._v_np = k, v
        if device == "cuda":
            import torch
            self.keys = torch.from_numpy(k.view(np.int64)).cuda()
            self.vals = torch.from_numpy(v.view(np.int64)).cuda()
        else:
            self.keys = k
            self.vals = v.view(np.uint8).reshape(-1, 8).copy()

    def run_step(self) -> ReduceByKeyResult:
        eng = self.engine
        t0 = time.perf_counter()
        handle = eng.register_shuffle(eng.world_size, self.R)
        w = eng.manager.get_writer(handle, eng.rank)
        if self.device == "cuda":
            w.write_device_batch(self.keys, self.vals)
        else:
            w.write_batch(self.keys, self.vals)
        # map-side combine ships one row per distinct key of this map task
        # (Spark's reduceByKey default); the reader then merges
        w.stop(True, partitioner=self.part,
               combiner=self.aggregator if self.map_side_combine else None)
        eng.barrier()
        lo, hi = eng.rank * self.ppe, (eng.rank + 1) * self.ppe - 1
        reader = eng.manager.get_reader(handle, lo, hi)
        # the reader's GENERIC aggregate hookup (RdmaShuffleReader.scala:
        # 61-114 role): sort by key + segmented reduction, device-side on
        # GPU (ops/csrc/reduce.hip)
        uk, sums = reader.read_aos(aggregator=self.aggregator,
                                   map_side_combined=self.map_side_combine)
        if self.device == "cuda":
            import torch
            torch.cuda.synchronize()
            groups = int(uk.numel())
        else:
            groups = len(uk)
        if self.validate:
            self._validate(uk, sums)
        eng.unregister_shuffle(handle)
        return ReduceByKeyResult(
            time.perf_counter() - t0, self.n, groups,
            reader.metrics.remote_bytes_read + reader.metrics.local_bytes_read)

    def _validate(self, uk, sums) -> None:
        """Single-rank oracle: this rank's groups must equal the dict-based
        reduction of every rank's rows hashing to this rank's partitions.
        Integer aggregators match exactly (payloads are below 2^20, so the
        signed and unsigned readings of min/max agree); sum_f64 reads the
        payload bits as doubles and is compared to math.fsum within the
        any-order summation bound."""
        import math
        eng = self.engine
        agg = self.aggregator
        rows: dict = {}
        for r in range(eng.world_size):
            # regenerate rank r's rows deterministically
            rng = np.random.default_rng(self.seed * 101 + r)
            k = rng.integers(0, self.num_keys, self.n, dtype=np.uint64)
            v = rng.integers(0, 1 << 20, self.n, dtype=np.uint64)
            pids = self.part.partition_ids(k)
            mine = (pids >= eng.rank * self.ppe) & \
                   (pids < (eng.rank + 1) * self.ppe)
            if agg == "sum_f64":
                v = v.view(np.float64)
            for kk, vv in zip(k[mine].tolist(), v[mine].tolist()):
                rows.setdefault(kk, []).append(vv)
        if self.device == "cuda":
            uk = uk.cpu().numpy().view(np.uint64)
            sums = sums.cpu().numpy()
        uk = np.asarray(uk)
        sums = np.asarray(sums)
        if agg == "sum_f64":
            got = dict(zip(uk.tolist(), sums.view(np.float64).tolist()))
            assert got.keys() == rows.keys(), (len(got), len(rows))
            for kk, vs in rows.items():
                bound = 2 * (len(vs) - 1) * 2.0 ** -53 * math.fsum(
                    abs(x) for x in vs)
                assert abs(got[kk] - math.fsum(vs)) <= bound, kk
            return
        fold = {"sum": lambda vs: sum(vs) & (2 ** 64 - 1), "count": len,
                "min": min, "max": max}[agg]
        want = {kk: fold(vs) for kk, vs in rows.items()}
        got = dict(zip(uk.tolist(), sums.view(np.uint64).tolist()))
        assert got == want, (len(got), len(want))
