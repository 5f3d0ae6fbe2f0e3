"""groupByKey over arbitrary pickled records — BASELINE config 1
(Spark local-cluster[2,1,1024] groupByKey on 1M synthetic rows; the
plumbing path, no GPU required).

Exercises the bytes-record write path, hash partitioning by pickled key,
and stream deserialization on the reduce side — the closest analog of the
reference's production validation workload shape.

``device="cuda"`` is the same workload on the GPU variable-length lane: u64
keys with byte-string values of random length go through
``write_device_varlen`` -> ``stop(partitioner=HashPartitioner(R))`` ->
``read_varlen(ordering=True)``, and the groups are the runs of equal keys.
"""

from __future__ import annotations

import time
from dataclasses import dataclass

import numpy as np

from ..engine import Engine
from ..partitioner import HashPartitioner


@dataclass
class GroupByResult:
    seconds: float
    rows: int
    groups: int


class GroupByKey:
    #: longest value of the device="cuda" rows, bytes
    MAX_VALUE_BYTES = 64

    def __init__(self, engine: Engine, rows_per_executor: int,
                 num_keys: int = 1000, num_partitions: int = 0, seed: int = 0,
                 device: str = "cpu", validate: bool = False):
        if device not in ("cpu", "cuda"):
            raise ValueError(f"unknown device {device!r}")
        self.engine = engine
        self.n = rows_per_executor
        self.num_keys = num_keys
        self.R = num_partitions or engine.world_size * 4
        self.seed = seed
        self.device = device
        self.validate = validate
        if device == "cuda":
            import torch
            self.part = HashPartitioner(self.R)
            k, off, data = self._rows(engine.rank)
            self.keys = torch.from_numpy(k.view(np.int64)).cuda()
            self.offsets = torch.from_numpy(off).cuda()
            self.data = torch.from_numpy(data).cuda()
            return
        rng = np.random.default_rng(seed + engine.rank)
        self.keys = rng.integers(0, num_keys, rows_per_executor)

    def _rows(self, rank: int):
        """Rank ``rank``'s variable-length rows, deterministically:
        (keys u64, offsets int64[n + 1], data uint8)."""
        rng = np.random.default_rng(self.seed * 101 + rank)
        keys = rng.integers(0, self.num_keys, self.n, dtype=np.uint64)
        offsets = np.zeros(self.n + 1, dtype=np.int64)
        np.cumsum(rng.integers(0, self.MAX_VALUE_BYTES + 1, self.n),
                  out=offsets[1:])
        data = rng.integers(0, 256, int(offsets[-1]), dtype=np.uint8)
        return keys, offsets, data

    def _run_step_varlen(self) -> GroupByResult:
        import torch
        eng = self.engine
        t0 = time.perf_counter()
        handle = eng.register_shuffle(eng.world_size, self.R)
        w = eng.manager.get_writer(handle, eng.rank)
        w.write_device_varlen(self.keys, self.offsets, self.data)
        w.stop(True, partitioner=self.part)
        eng.barrier()
        per = self.R // eng.world_size
        lo, hi = eng.rank * per, (eng.rank + 1) * per - 1
        reader = eng.manager.get_reader(handle, lo, hi)
        keys, offsets, data = reader.read_varlen(ordering=True)
        # a group is a run of equal keys
        groups = (1 + int((keys[1:] != keys[:-1]).sum())
                  if keys.numel() else 0)
        torch.cuda.synchronize()
        if self.validate:
            self._validate_varlen(keys, offsets, data, lo, hi)
        eng.unregister_shuffle(handle)
        return GroupByResult(time.perf_counter() - t0, self.n, groups)

    def _validate_varlen(self, keys, offsets, data, lo: int, hi: int) -> None:
        """Numpy oracle: the per-key multisets of values this rank read
        equal those of every rank's rows that hash to its partitions, and
        the keys come back ascending."""
        def groups_of(k, off, buf):
            out: dict = {}
            for r, key in enumerate(k.tolist()):
                out.setdefault(key, []).append(buf[off[r]:off[r + 1]])
            return {key: sorted(v) for key, v in out.items()}

        want: dict = {}
        for rank in range(self.engine.world_size):
            k, off, d = self._rows(rank)
            pids = self.part.partition_ids(k)
            buf = d.tobytes()
            for r in np.nonzero((pids >= lo) & (pids <= hi))[0].tolist():
                want.setdefault(int(k[r]), []).append(buf[off[r]:off[r + 1]])
        want = {key: sorted(v) for key, v in want.items()}
        k = keys.cpu().numpy().view(np.uint64)
        assert np.all(k[1:] >= k[:-1]), "keys are not ascending"
        got = groups_of(k, offsets.cpu().numpy(), data.cpu().numpy().tobytes())
        assert got.keys() == want.keys(), (len(got), len(want))
        assert got == want, "per-key value multisets differ"

    def run_step(self) -> GroupByResult:
        if self.device == "cuda":
            return self._run_step_varlen()
        eng = self.engine
        t0 = time.perf_counter()
        handle = eng.register_shuffle(eng.world_size, self.R)
        w = eng.manager.get_writer(handle, eng.rank)
        w.write_records(((f"key{k}", (eng.rank, int(k))) for k in self.keys),
                        None)
        w.stop(True)
        eng.barrier()
        per = self.R // eng.world_size
        lo, hi = eng.rank * per, (eng.rank + 1) * per - 1
        reader = eng.manager.get_reader(handle, lo, hi)
        groups = {}
        # reader-side generic deserialize (read_records) + group-by
        for k, v in reader.read_records():
            groups.setdefault(k, []).append(v)
        eng.unregister_shuffle(handle)
        return GroupByResult(time.perf_counter() - t0, self.n, len(groups))
