"""Micro-bench of the record-moving kernels on one MI355X.

Run on a GPU box:  python scripts/bench_record_movement.py [--gb 4]
Times, for 100-byte and 256-byte records:
  * gather_records dst_mode 0 (records -> sorted output, random permutation)
  * gather_records dst_mode 1 (records -> 256 per-digit destinations)
  * the map-side record move into 256 partitions: gather_records mode 1
    over grouped pairs against partition_records_fused over pairs in input
    order (--only-partition runs these alone)
  * sort_records(fuse=True)   (pair extract + radix passes + fused gather)
  * sort_records with the tie repair on and off, on random keys and on
    all-equal keys (the input that forces the fallback to the full passes)
  * the reduce-side fetch of the records: read_batch (hipMemcpyAsync) +
    extract_pairs against read_records_batch (the fused copy + pair-extract
    kernel), source and destination at 4-byte-only alignment
with device events, median of --launches launches, at a size far past the
256 MB Infinity Cache. GB/s counts each record's bytes ONCE (n * W / time):
the kernels read and write every record once, so memory traffic is at
least twice that figure.
"""

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from sparkrdma_amd.ops import load
from sparkrdma_amd.ops.radix import sort_records


def timed_ms(fn, launches, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(launches):
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        ms.append(t0.elapsed_time(t1))
    ms.sort()
    return ms[len(ms) // 2]


def report(name, W, n, ms):
    print(f"W={W:4d} n={n:10d} {name:28s} {ms:9.3f} ms  "
          f"{n * W / ms / 1e6:8.1f} GB/s of record bytes", flush=True)


def bench_width(hs, W, total_bytes, launches):
    n = (total_bytes // W) & ~1     # even: n * W is a whole number of u64
    dev = "cuda"
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev)
    g.manual_seed(W)
    recs = torch.randint(-2**63, 2**63 - 1, (n * W // 8,), dtype=torch.int64,
                         device=dev, generator=g).view(torch.uint8)
    out = torch.empty(n * W, dtype=torch.uint8, device=dev)

    # (key, aux) pairs: key = the record's own prefix, aux = random record
    # index with key-low bits in the high 16 (masked off by the kernels)
    perm = torch.randperm(n, device=dev, generator=g)
    pairs = torch.empty(n, 2, dtype=torch.int64, device=dev)
    keyw = recs.view(n, W)[:, :8].contiguous().view(torch.int64).view(n)
    pairs[:, 0] = keyw[perm]
    pairs[:, 1] = perm | (0x5A5A << 48)
    del keyw
    ms = timed_ms(lambda: hs.gather_records(
        recs.data_ptr(), pairs.data_ptr(), n, W, 0, out.data_ptr(),
        0, 0, 0, 0, 0, 0, s), launches)
    report("gather_records mode 0", W, n, ms)

    # mode 1: pairs grouped by the top 8 key bits, one destination per digit
    digit = (pairs[:, 0] >> 56) & 255
    order = torch.argsort(digit, stable=True)
    grouped = pairs[order].contiguous()
    counts = torch.bincount(digit, minlength=256)
    del digit, order, perm, pairs
    starts = torch.cumsum(counts, 0) - counts
    dst_addr = out.data_ptr() + starts * W
    dstart = starts.to(torch.int32)
    ms = timed_ms(lambda: hs.gather_records(
        recs.data_ptr(), grouped.data_ptr(), n, W, 1, 0,
        dst_addr.data_ptr(), dstart.data_ptr(), 56, 255, 0, 0, s), launches)
    report("gather_records mode 1", W, n, ms)
    del grouped

    prs = torch.empty(2 * n, dtype=torch.int64, device=dev)
    tmp = torch.empty(2 * n, dtype=torch.int64, device=dev)
    ms = timed_ms(lambda: sort_records(recs, W, key_bytes=10, out=out,
                                       pairs=prs, tmp=tmp, fuse=True),
                  launches)
    report("sort_records(fuse=True)", W, n, ms)
    ms = timed_ms(lambda: sort_records(recs, W, key_bytes=10, out=out,
                                       pairs=prs, tmp=tmp, fuse=False),
                  launches)
    report("sort_records(fuse=False)", W, n, ms)

    # truncated sort + tie repair against the full LSD sequence, on random
    # keys (path 1) and on all-equal keys, which force the fallback (path
    # 2: truncated attempt, then the full sequence). A build without the
    # switch times its only path.
    def sort_case(name, mode):
        if hasattr(hs, "set_tie_repair"):
            hs.set_tie_repair(mode)
        elif mode == 0:
            return
        try:
            ms = timed_ms(lambda: sort_records(recs, W, key_bytes=10,
                                               out=out, pairs=prs, tmp=tmp),
                          launches)
        finally:
            if hasattr(hs, "set_tie_repair"):
                hs.set_tie_repair(1)
        path = hs.last_sort_path() if hasattr(hs, "last_sort_path") else 0
        report(f"{name} repair={mode} path={path}", W, n, ms)

    sort_case("sort random", 1)
    sort_case("sort random", 0)
    recs.view(n, W)[:, :10] = 0x5A
    sort_case("sort equal keys", 1)
    sort_case("sort equal keys", 0)


def bench_partition(hs, W, total_bytes, launches):
    """The record move of the map-side write into 256 partitions (top 8 key
    bits): gather_records mode 1 over pairs already grouped by partition
    (the last of the three kernels of that route; random record reads)
    against partition_records_fused over the pairs in input order (the
    whole route after the counts; a tile's reads are one contiguous span).
    Both write the same bytes to the same places. A build without the fused
    entry times the gather only."""
    n = (total_bytes // W) & ~1
    dev = "cuda"
    s = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device=dev)
    g.manual_seed(W + 2)
    recs = torch.randint(-2**63, 2**63 - 1, (n * W // 8,), dtype=torch.int64,
                         device=dev, generator=g).view(torch.uint8)
    out = torch.empty(n * W, dtype=torch.uint8, device=dev)
    keyw = recs.view(n, W)[:, :8].contiguous().view(torch.int64).view(n)
    digit = (keyw >> 56) & 255
    idx = torch.arange(n, dtype=torch.int64, device=dev)
    counts = torch.bincount(digit, minlength=256)
    starts = torch.cumsum(counts, 0) - counts
    dst_addr = out.data_ptr() + starts * W

    order = torch.argsort(digit, stable=True)
    grouped = torch.stack([keyw[order], idx[order] | (0x5A5A << 48)], 1) \
        .contiguous()
    del order
    dstart = starts.to(torch.int32)
    ms = timed_ms(lambda: hs.gather_records(
        recs.data_ptr(), grouped.data_ptr(), n, W, 1, 0,
        dst_addr.data_ptr(), dstart.data_ptr(), 56, 255, 0, 0, s), launches)
    report("partition: gather mode 1", W, n, ms)
    del grouped
    if not hasattr(hs, "partition_records_fused"):
        return
    want = out[:min(n * W, 1 << 28)].clone()
    out.zero_()
    pairs = torch.stack([digit, idx | (0x5A5A << 48)], 1).contiguous()
    del digit, idx, keyw
    ws = torch.empty(hs.partition_records_workspace_bytes(n),
                     dtype=torch.uint8, device=dev)
    totals = torch.empty(256, dtype=torch.int32, device=dev)
    ms = timed_ms(lambda: hs.count_pair_digits(
        pairs.data_ptr(), n, totals.data_ptr(), s), launches)
    report("partition: count_pair_digits", W, n, ms)
    assert torch.equal(totals.to(torch.int64), counts)
    ms = timed_ms(lambda: hs.partition_records_fused(
        pairs.data_ptr(), n, recs.data_ptr(), W, dst_addr.data_ptr(),
        ws.data_ptr(), s), launches)
    report("partition: fused pass", W, n, ms)
    assert torch.equal(out[:want.numel()], want), "fused pass != gather"


def bench_fetch(hs, W, total_bytes, launches):
    """Fetch n W-byte records into an arena and produce their pairs: plain
    copy + extract_pairs against the fused kernel. src sits 4 and dst 12
    bytes into their buffers (mutually 8 mod 16). TB/s counts each byte
    once: records read + records written + pairs written."""
    n = total_bytes // W
    dev = "cuda"
    g = torch.Generator(device=dev)
    g.manual_seed(W + 1)
    src_buf = torch.randint(-2**63, 2**63 - 1, (n * W // 8 + 4,),
                            dtype=torch.int64, device=dev,
                            generator=g).view(torch.uint8)
    dst_buf = torch.empty(n * W + 32, dtype=torch.uint8, device=dev)
    pairs = torch.empty(2 * n, dtype=torch.int64, device=dev)
    src, dst = src_buf.data_ptr() + 4, dst_buf.data_ptr() + 12
    s = torch.cuda.current_stream().cuda_stream
    moved = 2 * n * W + 16 * n

    # the copy engine runs on its own streams: fence them with the events
    # of the current stream by waiting for the engine's completion event
    def plain():
        hs.wait_event(hs.read_batch(0, [dst], [src], [n * W]))
        hs.extract_pairs(dst, n, W, 10, pairs.data_ptr(), s)

    def copy_only():
        hs.wait_event(hs.read_batch(0, [dst], [src], [n * W]))

    def fused():
        hs.wait_event(hs.read_records_batch(
            0, [dst], [src], [n * W], W, 10, [pairs.data_ptr()], [0]))

    for name, fn, nbytes in (("read_batch alone", copy_only, 2 * n * W),
                             ("read_batch + extract_pairs", plain, moved),
                             ("read_records_batch (fused)", fused, moved)):
        ms = timed_ms(fn, launches)
        print(f"W={W:4d} n={n:10d} fetch: {name:28s} {ms:9.3f} ms  "
              f"{nbytes / ms / 1e9:6.2f} TB/s of bytes moved", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gb", type=float, default=4.0,
                    help="record bytes per case (default 4 GB)")
    ap.add_argument("--launches", type=int, default=11)
    ap.add_argument("--only-fetch", action="store_true",
                    help="run only the reduce-side fetch cases")
    ap.add_argument("--only-partition", action="store_true",
                    help="run only the map-side partition cases at 100 "
                         "bytes (the run to collect counters over)")
    args = ap.parse_args()
    if args.launches < 10:
        ap.error("--launches must be at least 10")
    if not torch.cuda.is_available():
        sys.exit("bench_record_movement needs a GPU")
    hs = load()
    if args.only_partition:
        bench_partition(hs, 100, int(args.gb * 1e9), args.launches)
        return
    for W in (100, 256):
        if not args.only_fetch:
            bench_width(hs, W, int(args.gb * 1e9), args.launches)
            torch.cuda.empty_cache()
            bench_partition(hs, W, int(args.gb * 1e9), args.launches)
            torch.cuda.empty_cache()
        bench_fetch(hs, W, int(args.gb * 1e9), args.launches)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
