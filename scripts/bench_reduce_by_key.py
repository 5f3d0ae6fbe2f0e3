"""Bench of the reduce_by_key kernel and of map-side combine on one MI355X.

Run on a GPU box:
  python scripts/bench_reduce_by_key.py op [log2_n] [runs]
  python scripts/bench_reduce_by_key.py workload [gb_per_gpu] [steps]

op        reduce_by_key_aos against the torch chain read_aos used before
          the kernel existed (unique_consecutive + index_add_ /
          scatter_reduce_), on the same sorted pairs, alternating the two
          in one process; median and range per distinct-key ratio.
workload  the reducebykey workload at bench.py's single-GPU configuration
          with and without map-side combine: step time and shuffle bytes.
"""

import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from sparkrdma_amd.ops import load
from sparkrdma_amd.ops.radix import REDUCE_OPS, reduce_by_key_aos


def torch_chain(pairs, aggregator):
    k = pairs[0::2].contiguous()
    v = pairs[1::2].contiguous()
    uk, inverse, cnt = torch.unique_consecutive(
        k, return_inverse=True, return_counts=True)
    if aggregator == "count":
        return uk, cnt
    if aggregator in ("sum", "sum_f64"):
        dt = torch.int64 if aggregator == "sum" else torch.float64
        out = torch.zeros(uk.numel(), dtype=dt, device=k.device)
        out.index_add_(0, inverse, v.view(dt))
        return uk, out
    red = "amin" if aggregator == "min" else "amax"
    out = torch.empty(uk.numel(), dtype=torch.int64, device=k.device)
    out.scatter_reduce_(0, inverse, v, reduce=red, include_self=False)
    return uk, out


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def bench_op(log2_n=26, runs=10):
    load()
    n = 1 << log2_n
    torch.manual_seed(0)
    vals = torch.randint(0, 1 << 20, (n,), dtype=torch.int64, device="cuda")
    idx = torch.arange(n, dtype=torch.int64, device="cuda")
    print(f"n = 2^{log2_n} sorted pairs, {runs} alternating runs, ms "
          "median [min..max]")
    for label, shift in (("1", 0), ("1/16", 4), ("1/4096", 12),
                         ("all-equal", 63)):
        pairs = torch.empty(2 * n, dtype=torch.int64, device="cuda")
        pairs[0::2] = idx >> shift
        for op in REDUCE_OPS:
            pairs[1::2] = vals.double().view(torch.int64) \
                if op == "sum_f64" else vals
            for _ in range(2):                       # warm-up
                reduce_by_key_aos(pairs, op)
                torch_chain(pairs, op)
            a, b = [], []
            for _ in range(runs):
                a.append(timed(lambda: reduce_by_key_aos(pairs, op)))
                b.append(timed(lambda: torch_chain(pairs, op)))
            ma, mb = statistics.median(a), statistics.median(b)
            print(f"ratio {label:>9} {op:>7}: kernel {ma:7.2f} "
                  f"[{min(a):.2f}..{max(a):.2f}]  torch {mb:7.2f} "
                  f"[{min(b):.2f}..{max(b):.2f}]  "
                  f"{'kernel' if ma <= mb else 'TORCH'} x{mb / ma:.2f}",
                  flush=True)
        del pairs


def bench_workload(gb_per_gpu=4.0, steps=3):
    from sparkrdma_amd.conf import ShuffleConf
    from sparkrdma_amd.engine import Engine
    from sparkrdma_amd.workloads.reduce_by_key import ReduceByKey
    # bench.py's single-GPU configuration for --workload reducebykey
    conf = ShuffleConf(transport="ipc")
    conf.hbm_pool_size = int((gb_per_gpu * 2.0 + 2) * (1 << 30))
    conf.shuffle_write_block_size = 512 << 20
    conf.shuffle_read_block_size = 512 << 20
    conf.max_bytes_in_flight = 8 << 30
    eng = Engine(conf, rank=0, world_size=1)
    try:
        rows = int(gb_per_gpu * (1 << 30) / 16)
        wl = ReduceByKey(eng, rows_per_executor=rows,
                         partitions_per_executor=256, device="cuda")
        for combine in (False, True, False, True):
            wl.map_side_combine = combine
            wl.run_step()                            # warm-up
            res = [wl.run_step() for _ in range(steps)]
            ts = [r.seconds for r in res]
            print(f"rows {rows} combine={combine}: step "
                  f"{statistics.median(ts):.3f}s [{min(ts):.3f}.."
                  f"{max(ts):.3f}]  groups {res[0].groups}  shuffle_bytes "
                  f"{res[0].shuffle_bytes}", flush=True)
    finally:
        eng.shutdown()


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "op"
    if what == "op":
        bench_op(*(int(a) for a in sys.argv[2:4]))
    else:
        args = sys.argv[2:4]
        bench_workload(*([float(args[0])] + [int(a) for a in args[1:]]
                         if args else []))
