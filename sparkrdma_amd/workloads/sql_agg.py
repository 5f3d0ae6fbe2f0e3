"""SELECT k, sum(qty), sum(price), min(discount), max(flag), count(*)
GROUP BY k over a shuffled table of wide rows — the aggregation half of the
SQL workload (BASELINE config 5), and reduceByKey over tuple values.

Synthetic W-byte rows, little-endian:

    u64 key | i64 qty | f64 price | f32 discount | i32 flag | padding

One step: hash-partition the rows by key through the record lane
(write_device_records, or write_batch on the CPU lane), one-sided shuffle,
then ``reader.read_records_agg``: on the GPU the (key, index) pairs are
sorted and ops/csrc/reduce_records.hip reduces the five columns per key
without moving a row — with ``in_place`` not even out of the blocks this
executor wrote. Validated against a per-key dict oracle.
"""

from __future__ import annotations

import time
from dataclasses import dataclass

import numpy as np

from ..engine import Engine
from ..partitioner import HashPartitioner

OFF_QTY, OFF_PRICE, OFF_DISCOUNT, OFF_FLAG, ROW_MIN_BYTES = 8, 16, 24, 28, 40

#: the query: (offset_bytes, dtype, op) per output column
COLUMNS = ((OFF_QTY, "i64", "sum"), (OFF_PRICE, "f64", "sum"),
           (OFF_DISCOUNT, "f32", "min"), (OFF_FLAG, "i32", "max"),
           (None, None, "count"))


@dataclass
class GroupByAggregateResult:
    seconds: float
    rows: int
    groups: int
    shuffle_bytes: int


def make_rows(rng, n: int, num_keys: int, W: int) -> np.ndarray:
    """n synthetic rows as uint8 [n, W]. Prices are multiples of 1/4 below
    2^18 and discounts multiples of 1/64, so every float partial sum is
    exact and the oracle can compare with ==."""
    rows = np.zeros((n, W), dtype=np.uint8)
    rows[:, 0:8] = rng.integers(0, num_keys, n, dtype=np.uint64) \
        .astype("<u8").view(np.uint8).reshape(n, 8)
    rows[:, OFF_QTY:OFF_QTY + 8] = rng.integers(-1000, 1000, n) \
        .astype("<i8").view(np.uint8).reshape(n, 8)
    rows[:, OFF_PRICE:OFF_PRICE + 8] = \
        (rng.integers(0, 1 << 20, n) / 4.0).astype("<f8") \
        .view(np.uint8).reshape(n, 8)
    rows[:, OFF_DISCOUNT:OFF_DISCOUNT + 4] = \
        (rng.integers(0, 64, n) / 64.0).astype("<f4") \
        .view(np.uint8).reshape(n, 4)
    rows[:, OFF_FLAG:OFF_FLAG + 4] = rng.integers(-(1 << 31), 1 << 31, n) \
        .astype("<i4").view(np.uint8).reshape(n, 4)
    rows[:, 32:] = rng.integers(0, 256, (n, W - 32), dtype=np.uint8)
    return rows


class GroupByAggregate:
    def __init__(self, engine: Engine, rows_per_executor: int,
                 num_keys: int = 1 << 16, partitions_per_executor: int = 32,
                 device: str = "cpu", validate: bool = False, seed: int = 0,
                 record_bytes: int = 64, in_place: bool = False):
        if record_bytes % 4 or record_bytes < ROW_MIN_BYTES:
            raise ValueError(f"record_bytes must be a multiple of 4, "
                             f">= {ROW_MIN_BYTES}")
        if in_place and device != "cuda":
            raise ValueError("in_place is a GPU-lane option")
        self.engine = engine
        self.n = rows_per_executor
        self.W = record_bytes
        self.device = device
        self.validate = validate
        self.in_place = in_place
        R = engine.world_size * partitions_per_executor
        if R & (R - 1):
            raise ValueError("total partitions must be pow2")
        self.R = R
        self.ppe = partitions_per_executor
        self.part = HashPartitioner(R)
        self.seed = seed
        self.num_keys = num_keys
        self._rows_np = self._rows_of(engine.rank)
        if device == "cuda":
            import torch
            self.recs = torch.from_numpy(self._rows_np.reshape(-1)).cuda()

    def _rows_of(self, rank: int) -> np.ndarray:
        rng = np.random.default_rng(self.seed * 101 + rank)
        return make_rows(rng, self.n, self.num_keys, self.W)

    def run_step(self) -> GroupByAggregateResult:
        eng = self.engine
        W = self.W
        t0 = time.perf_counter()
        handle = eng.register_shuffle(eng.world_size, self.R)
        w = eng.manager.get_writer(handle, eng.rank)
        if self.device == "cuda":
            w.write_device_records(self.recs, W, key_bytes=8)
        else:
            rows = self._rows_np
            w.write_batch(rows[:, :8].copy().view("<u8").reshape(-1),
                          rows[:, 8:])
        w.stop(True, partitioner=self.part)
        eng.barrier()
        lo, hi = eng.rank * self.ppe, (eng.rank + 1) * self.ppe - 1
        if self.in_place:
            # the record spec plus an arena hint turn the fused lane on;
            # blocks this executor owns then stay where they are (conf
            # fusedRecordFetch=inplace) and only their column bytes are read
            import torch
            cap = eng.world_size * self.n * W + 4096
            arena = torch.empty(cap, dtype=torch.uint8, device="cuda")
            pairs = torch.empty(2 * (cap // W) + 16, dtype=torch.int64,
                                device="cuda")
            reader = eng.manager.get_reader(handle, lo, hi, arena=arena,
                                            records=(W, 8, pairs),
                                            in_place=True)
        else:
            reader = eng.manager.get_reader(handle, lo, hi)
        keys, cols = reader.read_records_agg(W, COLUMNS)
        if self.device == "cuda":
            import torch
            # the in-place segments die with unregister_shuffle below
            torch.cuda.synchronize()
            groups = int(keys.numel())
        else:
            groups = len(keys)
        if self.validate:
            self._validate(keys, cols)
        eng.unregister_shuffle(handle)
        return GroupByAggregateResult(
            time.perf_counter() - t0, self.n, groups,
            reader.metrics.remote_bytes_read + reader.metrics.local_bytes_read)

    def _validate(self, keys, cols) -> None:
        """Single-rank oracle: this rank's groups must equal the dict-based
        reduction of every rank's rows hashing to this rank's partitions.
        Everything compares exactly: make_rows keeps the float sums exact."""
        eng = self.engine
        want: dict = {}
        for r in range(eng.world_size):
            rows = self._rows_of(r)
            k = rows[:, :8].copy().view("<u8").reshape(-1)
            pids = self.part.partition_ids(k)
            mine = (pids >= eng.rank * self.ppe) & \
                   (pids < (eng.rank + 1) * self.ppe)
            rows, k = rows[mine], k[mine]

            def col(off, dt):
                size = np.dtype(dt).itemsize
                return rows[:, off:off + size].copy().view(dt).reshape(-1)
            for kk, q, p, d, f in zip(
                    k.tolist(), col(OFF_QTY, "<i8").tolist(),
                    col(OFF_PRICE, "<f8").tolist(),
                    col(OFF_DISCOUNT, "<f4").tolist(),
                    col(OFF_FLAG, "<i4").tolist()):
                a = want.get(kk)
                want[kk] = ((q, p, d, f, 1) if a is None else
                            (a[0] + q, a[1] + p, min(a[2], d), max(a[3], f),
                             a[4] + 1))
        if self.device == "cuda":
            keys = keys.cpu().numpy()
            cols = [c.cpu().numpy() for c in cols]
        keys = np.asarray(keys).view(np.uint64)
        assert np.all(keys[1:] > keys[:-1]), "keys not ascending"
        got = {kk: tuple(vs) for kk, *vs in zip(
            keys.tolist(), *(np.asarray(c).tolist() for c in cols))}
        assert got == want, (len(got), len(want))
