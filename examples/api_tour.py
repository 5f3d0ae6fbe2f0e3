#!/usr/bin/env python3
"""API tour — the ShuffleManager surface in one runnable file (CPU-only).

For a user coming from the reference plugin (Mellanox/SparkRDMA): the same
lifecycle Spark drives through `spark.shuffle.manager` —
registerShuffle → getWriter/write/stop(commit) → getReader/read →
unregisterShuffle — driven directly here. Run:

    python examples/api_tour.py

Everything below works without a GPU (host-shm segments); on an MI355X
box the same code serves map output from HBM and fetches it over xGMI —
the transport is picked per-executor by `transport=auto`.
"""

import os
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np

from sparkrdma_amd.conf import ShuffleConf
from sparkrdma_amd.engine import Engine
from sparkrdma_amd.partitioner import HashPartitioner, RangePartitioner
from sparkrdma_amd.writer import unpack_partition_segment


def main():
    tmp = tempfile.mkdtemp(prefix="sparkrdma_tour_")
    # --- configuration: the reference's spark.shuffle.rdma.* namespace ---
    conf = ShuffleConf.from_dict({
        "spark.shuffle.rdma.maxBytesInFlight": "48m",
        "spark.shuffle.rdma.shuffleReadBlockSize": "256k",
        "spark.shuffle.rdma.shmDir": tmp,
    })

    # --- an Engine is one executor process; rank 0 hosts the registry ---
    # (multi-process: launch N of these under torchrun, one per GPU)
    with Engine(conf, rank=0, world_size=1, driver_port=0) as eng:
        mgr = eng.manager

        # 1) fixed-width records: u64 keys, hash-partitioned -------------
        handle = eng.register_shuffle(num_maps=1, num_partitions=4)
        writer = mgr.get_writer(handle, map_id=0)
        keys = np.arange(100_000, dtype=np.uint64)
        writer.write_batch(keys)                       # stage rows
        writer.stop(True, partitioner=HashPartitioner(4))   # commit+publish
        reader = mgr.get_reader(handle, start_partition=0, end_partition=3)
        got = 0
        for pid, chunks in reader.collect_partitions().items():
            for chunk in chunks:                       # packed segments
                k, _v = unpack_partition_segment(chunk, 0)
                got += len(k)
        assert got == len(keys)
        eng.unregister_shuffle(handle)
        print(f"fixed-width: shuffled {got} u64 keys across 4 partitions")

        # 2) arbitrary Python records: the pickled lane ------------------
        handle = eng.register_shuffle(num_maps=1, num_partitions=2)
        writer = mgr.get_writer(handle, map_id=0)
        writer.write_records([(f"word{i % 10}", 1) for i in range(1000)],
                             partitioner=None)          # default: hash(key)
        writer.stop(True)
        reader = mgr.get_reader(handle, 0, 1)
        counts = {}
        for word, one in reader.read_records():
            counts[word] = counts.get(word, 0) + one
        assert sum(counts.values()) == 1000
        eng.unregister_shuffle(handle)
        print(f"pickled lane: word-counted 1000 records -> {len(counts)} keys")

        # 3) range partitioning (TeraSort-style total order) -------------
        handle = eng.register_shuffle(num_maps=1, num_partitions=8)
        writer = mgr.get_writer(handle, map_id=0)
        rng = np.random.default_rng(0)
        # uniform bounds split the FULL u64 key space (TeraSort convention)
        writer.write_batch(rng.integers(0, 2**64, 50_000, dtype=np.uint64))
        writer.stop(True, partitioner=RangePartitioner.uniform(8))
        reader = mgr.get_reader(handle, 0, 7)
        parts = reader.collect_partitions()            # {pid: [chunks]}
        sizes = [sum(len(unpack_partition_segment(c, 0)[0]) for c in parts[p])
                 for p in sorted(parts)]
        assert all(s > 0 for s in sizes)
        eng.unregister_shuffle(handle)
        print(f"range-partitioned: keys per partition = {sizes}")

        # 4) reduceByKey with map-side combine ---------------------------
        # stop(combiner=...) ships one row per distinct key of the map
        # task; the reader merges those partial results
        handle = eng.register_shuffle(num_maps=1, num_partitions=4)
        writer = mgr.get_writer(handle, map_id=0)
        k = rng.integers(0, 100, 50_000, dtype=np.uint64)
        ones = np.ones(50_000, dtype=np.uint64)
        writer.write_batch(k, ones.view(np.uint8).reshape(-1, 8))
        writer.stop(True, partitioner=HashPartitioner(4), combiner="sum")
        reader = mgr.get_reader(handle, 0, 3)
        uk, sums = reader.read_aos(aggregator="sum", map_side_combined=True)
        assert int(np.sum(sums)) == 50_000 and len(uk) == 100
        shipped = writer.metrics.records_written
        eng.unregister_shuffle(handle)
        print(f"map-side combine: 50000 rows in, {shipped} rows shipped, "
              f"{len(uk)} keys out")

        # 5) sampled range partitioning: split points from the data ------
        # skewed keys (most of them small) overload the first partitions
        # of uniform(8); bounds taken from a sample balance them. On an
        # MI355X box the write is the GPU lane: the split points are
        # searched by the extract_pairs_bounds kernel (func 4).
        skewed = (rng.random(50_000) ** 4 * 2.0**64).astype(np.uint64)
        part = RangePartitioner.from_sample(rng.choice(skewed, 4096), 8)
        assert part.gpu_params() == (4, 0, 8)
        handle = eng.register_shuffle(num_maps=1, num_partitions=8)
        writer = mgr.get_writer(handle, map_id=0)
        if mgr.gpu is not None:
            import torch
            writer.write_device_batch(
                torch.from_numpy(skewed.view(np.int64)).cuda())
        else:
            writer.write_batch(skewed)
        writer.stop(True, partitioner=part)
        want = np.bincount(part.partition_ids(skewed), minlength=8)
        parts = mgr.get_reader(handle, 0, 7).collect_partitions()
        sizes = [sum((c.numel() if hasattr(c, "numel") else len(c)) // 8
                     for c in parts[p]) for p in sorted(parts)]
        assert sizes == want.tolist()
        uni = np.bincount(RangePartitioner.uniform(8).partition_ids(skewed),
                          minlength=8)
        eng.unregister_shuffle(handle)
        print(f"sampled bounds: keys per partition = {sizes} "
              f"(uniform bounds: {uni.tolist()})")

        # 6) variable-length rows: u64 key + a payload of any length ------
        # CSR layout (keys, offsets, data): row r is
        # data[offsets[r]:offsets[r + 1]]. write_varlen is the CPU lane;
        # write_device_varlen takes the same three as CUDA tensors.
        words = [f"value-{i}".encode() * (i % 4) for i in range(1000)]
        k = rng.integers(0, 20, len(words), dtype=np.uint64)
        offsets = np.concatenate([[0], np.cumsum([len(w) for w in words])])
        handle = eng.register_shuffle(num_maps=1, num_partitions=4)
        writer = mgr.get_writer(handle, map_id=0)
        writer.write_varlen(k, offsets, np.frombuffer(b"".join(words),
                                                      dtype=np.uint8))
        writer.stop(True, partitioner=HashPartitioner(4))
        gk, goff, gdata = mgr.get_reader(handle, 0, 3).read_varlen(
            ordering=True)                 # grouped: equal keys adjacent
        if hasattr(gk, "cpu"):             # GPU data plane: device tensors
            gk, goff, gdata = (t.cpu().numpy() for t in (gk, goff, gdata))
        buf = gdata.tobytes()
        assert sorted(buf[goff[r]:goff[r + 1]] for r in range(len(gk))) \
            == sorted(words)
        gk = gk.view(np.uint64)
        assert np.all(gk[1:] >= gk[:-1])
        eng.unregister_shuffle(handle)
        print(f"variable-length: {len(gk)} rows, {len(buf)} payload bytes, "
              f"{len(np.unique(gk))} groups")

        # 7) GROUP BY over wide rows: several aggregates per key ----------
        # 24-byte rows: u64 key | i64 qty | f32 price | i32 flag. A column
        # is (offset_bytes, dtype, op); integers reduce as int64, floats
        # as float64. This is the numpy lane; on the GPU lane the rows
        # are written with write_device_records(recs, 24, key_bytes=8),
        # the results are device tensors and the rows are reduced where
        # they lie (ops/csrc/reduce_records.hip).
        n = 20_000
        rows = np.zeros((n, 24), dtype=np.uint8)
        rows[:, 0:8] = rng.integers(0, 50, n, dtype=np.uint64) \
            .view(np.uint8).reshape(n, 8)
        rows[:, 8:16] = rng.integers(1, 10, n).astype("<i8") \
            .view(np.uint8).reshape(n, 8)
        rows[:, 16:20] = rng.integers(1, 100, n).astype("<f4") \
            .view(np.uint8).reshape(n, 4)
        handle = eng.register_shuffle(num_maps=1, num_partitions=4)
        writer = mgr.get_writer(handle, map_id=0)
        writer.write_batch(rows[:, :8].copy().view(np.uint64).ravel(),
                           rows[:, 8:])
        writer.stop(True, partitioner=HashPartitioner(4))
        gk, (qty, price_min, cnt) = mgr.get_reader(handle, 0, 3) \
            .read_records_agg(24, [(8, "i64", "sum"), (16, "f32", "min"),
                                   (None, None, "count")])
        assert len(gk) == 50 and int(cnt.sum()) == n
        assert int(qty.sum()) == int(rows[:, 8:16].copy().view("<i8").sum())
        eng.unregister_shuffle(handle)
        print(f"group by: {n} rows -> {len(gk)} keys, sum(qty) = "
              f"{int(qty.sum())}, min(price) over all = {price_min.min():.0f}")

        # 8) metrics: the task/executor counters the reference feeds Spark
        print("lifetime:", mgr.lifetime_metrics.format())


if __name__ == "__main__":
    main()
