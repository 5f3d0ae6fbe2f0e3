"""Bench of the variable-length row copy (ops/csrc/varlen.hip) and of the
group-by step built on it, on one MI355X.

Run on a GPU box:
  python scripts/bench_varlen.py [log2_bytes] [runs] [groupby_rows]

Part 1 copies about 2^log2_bytes payload bytes (default 30) with
varlen_copy into one contiguous destination, rows taken from a contiguous
source in a random order (what a partition or a sort leaves behind):

  fixed100   every row 100 B; next to gather_records at W = 100 on the same
             rows in the same order, outputs compared equal
  u16        row lengths uniform in 0..16
  u200       row lengths uniform in 0..200
  zipf       floor(8 / u) bytes for u uniform in (0, 1], capped at 4 MiB:
             mostly short rows, a few long ones hold most bytes
  one        ONE row of all the bytes; next to a plain device-to-device
             copy_ of the same bytes, outputs compared equal

fixed100 and u200 also run with wide_loads=False (byte loads only), the
alternative to two aligned 16-byte loads and a shift. Times are device
events around the call alone (tables built before), median [min..max] over
the runs after one warm-up; neighbours alternate inside one loop. GB/s is
payload bytes copied per second — each byte is read once and written once,
and the per-row tables (16 B a row) come on top, so it is a call rate and
not a share of peak.

Part 2 runs the GroupByKey workload step (host clock, whole step:
register, write, publish, fetch, sort, copy) on the device lane and on the
pickled lane at the same row count.
"""

import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from sparkrdma_amd.ops import load
from sparkrdma_amd.ops.varlen import exclusive_scan, varlen_copy


def event_ms(fn):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def fmt(ts):
    return f"{statistics.median(ts):.3f} [{min(ts):.3f}..{max(ts):.3f}]"


def row(name, what, n, nbytes, ts):
    med = statistics.median(ts)
    print(f"| {name} | {what} | {n} | {nbytes} | {fmt(ts)} | "
          f"{nbytes / med / 1e6:.1f} |", flush=True)


def lengths(kind, total, gen):
    """Row lengths (int64, device) whose sum is just above ``total``."""
    mean = {"fixed100": 100, "u16": 8, "u200": 100, "zipf": 8}[kind]
    n = total // mean + 1024
    if kind == "fixed100":
        return torch.full((total // 100,), 100, dtype=torch.int64,
                          device="cuda")
    if kind == "zipf":
        u = torch.rand(n, device="cuda", generator=gen).clamp_(min=1e-9)
        lens = torch.clamp((8.0 / u).to(torch.int64), max=4 << 20)
    else:
        hi = 16 if kind == "u16" else 200
        lens = torch.randint(0, hi + 1, (n,), dtype=torch.int64,
                             device="cuda", generator=gen)
    cum = torch.cumsum(lens, 0)
    keep = int(torch.searchsorted(cum, torch.tensor([total], device="cuda")
                                  )[0]) + 1
    return lens[:keep].contiguous()


class Case:
    """Source rows back to back in ``src``; destination row r is source row
    perm[r]."""

    def __init__(self, kind, total, gen):
        lens = lengths(kind, total, gen)
        self.n = lens.numel()
        self.perm = torch.randperm(self.n, device="cuda", generator=gen)
        src_off = exclusive_scan(lens)
        self.bytes = int(src_off[-1])
        self.src = torch.randint(0, 256, (self.bytes,), dtype=torch.uint8,
                                 device="cuda", generator=gen)
        self.dst = torch.empty(self.bytes, dtype=torch.uint8, device="cuda")
        self.cum = exclusive_scan(lens[self.perm])
        self.addr = (src_off[:-1][self.perm] + self.src.data_ptr()) \
            .contiguous()
        self.first = torch.tensor([0, self.n], dtype=torch.int64,
                                  device="cuda")
        self.seg_dst = torch.tensor([self.dst.data_ptr()], dtype=torch.int64,
                                    device="cuda")
        del lens, src_off

    def copy(self, wide=True):
        varlen_copy(self.cum, self.addr, self.first, self.seg_dst,
                    total=self.bytes, wide_loads=wide)


def bench_copy(log2_bytes, runs):
    m = load()
    total = 1 << log2_bytes
    gen = torch.Generator(device="cuda")
    gen.manual_seed(12)
    stream = torch.cuda.current_stream().cuda_stream
    print(f"payload 2^{log2_bytes} bytes, {runs} runs, ms median "
          "[min..max]\n", flush=True)
    print("| case | path | rows | payload bytes | ms | payload GB/s |")
    print("|---|---|---|---|---|---|", flush=True)
    for kind in ("fixed100", "u16", "u200", "zipf"):
        c = Case(kind, total, gen)
        paths = [("varlen_copy", lambda: c.copy(True))]
        if kind in ("fixed100", "u200"):
            paths.append(("varlen_copy, byte loads", lambda: c.copy(False)))
        if kind == "fixed100":
            pairs = torch.zeros(2 * c.n, dtype=torch.int64, device="cuda")
            pairs[1::2] = c.perm
            out = torch.empty_like(c.dst)
            paths.append(("gather_records W=100", lambda: m.gather_records(
                c.src.data_ptr(), pairs.data_ptr(), c.n, 100, 0,
                out.data_ptr(), 0, 0, 0, 0, 0, 0, stream)))
        for _name, fn in paths:                          # warm-up
            fn()
        torch.cuda.synchronize()
        if kind == "fixed100" and not torch.equal(out, c.dst):
            raise SystemExit("varlen_copy and gather_records disagree")
        ts = {name: [] for name, _fn in paths}
        for _ in range(runs):
            for name, fn in paths:
                ts[name].append(event_ms(fn))
        for name, _fn in paths:
            row(kind, name, c.n, c.bytes, ts[name])
        # spot check: 64 destination rows against their sources
        c.copy(True)
        cum = c.cum.cpu()
        for r in torch.randint(0, c.n, (64,)).tolist():
            a, b = int(cum[r]), int(cum[r + 1])
            s = int(c.addr[r]) - c.src.data_ptr()
            if not torch.equal(c.dst[a:b], c.src[s:s + b - a]):
                raise SystemExit(f"{kind}: row {r} differs")
        del c, paths
        torch.cuda.empty_cache()
    # one row of all the bytes, against copy_
    src = torch.randint(0, 256, (total,), dtype=torch.uint8, device="cuda",
                        generator=gen)
    dst = torch.empty_like(src)
    ref = torch.empty_like(src)
    cum = torch.tensor([0, total], dtype=torch.int64, device="cuda")
    addr = torch.tensor([src.data_ptr()], dtype=torch.int64, device="cuda")
    first = torch.tensor([0, 1], dtype=torch.int64, device="cuda")
    seg = torch.tensor([dst.data_ptr()], dtype=torch.int64, device="cuda")
    paths = [("varlen_copy", lambda: varlen_copy(cum, addr, first, seg,
                                                 total=total)),
             ("copy_", lambda: ref.copy_(src))]
    for _name, fn in paths:
        fn()
    torch.cuda.synchronize()
    if not torch.equal(dst, ref):
        raise SystemExit("one row: varlen_copy and copy_ disagree")
    ts = {name: [] for name, _fn in paths}
    for _ in range(runs):
        for name, fn in paths:
            ts[name].append(event_ms(fn))
    for name, _fn in paths:
        row("one", name, 1, total, ts[name])


def bench_groupby(rows, runs):
    from sparkrdma_amd.conf import ShuffleConf
    from sparkrdma_amd.engine import Engine
    from sparkrdma_amd.workloads.groupby import GroupByKey
    print(f"\nGroupByKey step, {rows} rows, 1000 keys, 4 partitions, host "
          "clock, s\n", flush=True)
    print("| lane | runs | s median [min..max] | groups |")
    print("|---|---|---|---|", flush=True)
    eng = Engine(ShuffleConf(transport="ipc", hbm_pool_size=2 << 30),
                 rank=0, world_size=1, driver_port=0)
    try:
        g = GroupByKey(eng, rows_per_executor=rows, device="cuda")
        g.run_step()                                     # warm-up
        res = [g.run_step() for _ in range(runs)]
        ts = [r.seconds for r in res]
        print(f"| write_device_varlen / read_varlen | {runs} | {fmt(ts)} | "
              f"{res[0].groups} |", flush=True)
        g = GroupByKey(eng, rows_per_executor=rows)
        r = g.run_step()
        ts = [r.seconds]
        print(f"| write_records / read_records (pickled) | 1 | {fmt(ts)} | "
              f"{r.groups} |", flush=True)
    finally:
        eng.shutdown()


if __name__ == "__main__":
    args = [int(a) for a in sys.argv[1:4]]
    log2_bytes = args[0] if len(args) > 0 else 30
    runs = args[1] if len(args) > 1 else 10
    gb_rows = args[2] if len(args) > 2 else 1_000_000
    if not torch.cuda.is_available():
        raise SystemExit("bench_varlen.py measures on a GPU; none is visible")
    bench_copy(log2_bytes, runs)
    bench_groupby(gb_rows, max(runs // 3, 3))
