"""Map-side write with split-point (bounds) partitioning on one MI355X.

Run on a GPU box:
  python scripts/bench_range_partition.py wide  [log2_n] [rounds] [log2_R]
  python scripts/bench_range_partition.py pairs [log2_n] [rounds] [log2_R]

Times ShuffleWriter.stop() — partition, lay out, publish — for n records
into R partitions (default 512), uniform u64 keys in every arm:

wide   100-byte records. RangePartitioner.uniform(R) (func 0, top bits)
       against bounds sampled from the keys (func 4). The two lanes
       differ in the extract kernel only (extract_pairs against
       extract_pairs_bounds) and, at 257 <= R <= 4096, in the digit of
       hist / scatter / gather (top key bits against the stored pid).
       R <= 256 takes the fused route in both lanes (ids counted, one
       fused pass); R > 4096 adds the two-level pid radix to both alike.
pairs  16-byte (key, value) records. uniform(R) takes the direct
       scatter; bounds take the record lane (pairs + gather).

Every round runs uniform, bounds, uniform again: the spread between the
two uniform arms bounds what counts as a difference.
"""

import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from sparkrdma_amd.conf import ShuffleConf
from sparkrdma_amd.engine import Engine
from sparkrdma_amd.partitioner import RangePartitioner


def _write_once(eng, part, feed, R):
    handle = eng.register_shuffle(1, R)
    w = eng.manager.get_writer(handle, 0)
    feed(w)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    w.stop(True, partitioner=part)      # ends in a device synchronise
    dt = (time.perf_counter() - t0) * 1e3
    eng.unregister_shuffle(handle)
    return dt


def _fmt(ts):
    return f"{statistics.median(ts):8.2f} [{min(ts):.2f}..{max(ts):.2f}]"


def main(shape="wide", log2_n=26, rounds=5, log2_R=9):
    n = 1 << log2_n
    R = 1 << log2_R
    W = 100 if shape == "wide" else 16
    conf = ShuffleConf(transport="ipc")
    conf.hbm_pool_size = n * W + (2 << 30)
    conf.shuffle_write_block_size = 512 << 20
    eng = Engine(conf, rank=0, world_size=1, driver_port=0)
    try:
        g = torch.Generator(device="cuda").manual_seed(1)
        keys = torch.randint(-2**63, 2**63 - 1, (n,), dtype=torch.int64,
                             device="cuda", generator=g)
        if shape == "wide":
            recs = torch.randint(-128, 128, (n, W), dtype=torch.int8,
                                 device="cuda", generator=g)
            recs[:, :8] = keys.view(torch.int8).reshape(n, 8)
            recs = recs.view(torch.uint8).reshape(-1)

            def feed(w):
                w.write_device_records(recs, W, 10)
        else:
            vals = keys.clone()

            def feed(w):
                w.write_device_batch(keys, vals)
        sample = keys[torch.randint(0, n, (1 << 16,), device="cuda",
                                    generator=g)]
        arms = [("uniform-a", RangePartitioner.uniform(R)),
                ("bounds", RangePartitioner.from_sample(sample, R)),
                ("uniform-b", RangePartitioner.uniform(R))]
        assert arms[0][1].gpu_params()[0] == 0
        assert arms[1][1].gpu_params()[0] == 4
        for _name, part in arms[:2]:                 # warm-up, both lanes
            for _ in range(2):
                _write_once(eng, part, feed, R)
        times = {name: [] for name, _ in arms}
        for _ in range(rounds):
            for name, part in arms:
                times[name].append(_write_once(eng, part, feed, R))
        print(f"{shape}: n = 2^{log2_n} x {W} B, R = {R}, {rounds} rounds, "
              "stop() ms median [min..max]")
        for name, _ in arms:
            print(f"  {name:>9}: {_fmt(times[name])}")
        ua = statistics.median(times["uniform-a"])
        ub = statistics.median(times["uniform-b"])
        b = statistics.median(times["bounds"])
        print(f"  bounds / uniform-a = {b / ua:.3f}   "
              f"uniform-b / uniform-a = {ub / ua:.3f}", flush=True)
    finally:
        eng.shutdown()


if __name__ == "__main__":
    a = sys.argv[1:]
    main(a[0] if a else "wide", *(int(x) for x in a[1:4]))
