"""Bench of the keyed aggregation of wide records on one MI355X.

Run on a GPU box:
  python scripts/bench_records_agg.py [--log2-n 26] [--runs 10]
         [--widths 16,100,256] [--columns 1,4,8] [--log2-keys 26,20,0]

Two arms on the same unsorted records, alternating inside one loop, device
events around each (both arms block once inside to read a count back; the
events still bracket all their device work):

new          ops.radix.aggregate_records — extract (key, index) pairs, sort
             them, reduce_records.hip gathers and reduces the columns where
             the records lie. No record is moved.
composition  what a user had before it: sort_records moves every whole
             record, then per column a strided slice of the sorted records,
             widened, interleaved with the keys, and reduce_by_key_aos.

The columns use only what the composition can express (integer sum / min /
max, float sum, count). Outputs are compared at the timed size before the
timing. Bytes per record are printed from the shapes: the pairs the sort
moves, the 64-byte lines a record's column fields touch, the scratch.
"""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from sparkrdma_amd.ops import load
from sparkrdma_amd.ops.radix import (aggregate_records, onesweep_passes,
                                     reduce_by_key_aos, sort_records)

TORCH_OF = {"i32": torch.int32, "u32": torch.int32, "i64": torch.int64,
            "f32": torch.float32, "f64": torch.float64}
SIZE_OF = {"i32": 4, "u32": 4, "i64": 8, "f32": 4, "f64": 8}


def columns_for(W, C):
    """The first C of a fixed list per layout. W = 16: i32 at 8, f32 at 12.
    W >= 40: i64 at 8, f64 at 16, f32 at 24, i32 at 28, and the record's
    last 8 bytes as an i64 / its last 4 as a u32."""
    if W == 16:
        cols = [(8, "i32", "sum"), (12, "f32", "sum"), (8, "i32", "min"),
                (None, None, "count"), (8, "i32", "max"), (8, "u32", "sum"),
                (8, "u32", "max"), (8, "u32", "min")]
    else:
        cols = [(8, "i64", "sum"), (16, "f64", "sum"), (24, "f32", "sum"),
                (None, None, "count"), (28, "i32", "max"),
                (W - 8, "i64", "min"), (W - 4, "u32", "sum"),
                (28, "i32", "min")]
    return cols[:C]


def make_records(n, W, log2_keys, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    recs = torch.randint(0, 256, (n, W), dtype=torch.uint8, device="cuda",
                         generator=g)
    keys = torch.randint(0, 1 << log2_keys, (n,), dtype=torch.int64,
                         device="cuda", generator=g) if log2_keys else \
        torch.full((n,), 0x1234567, dtype=torch.int64, device="cuda")
    recs[:, 0:8] = keys.view(torch.uint8).view(n, 8)
    small = torch.randint(0, 1 << 20, (n,), dtype=torch.int64, device="cuda",
                          generator=g)
    # float fields hold small integers: sums are exact, the arms must agree
    if W == 16:
        recs[:, 12:16] = small.float().view(torch.uint8).view(n, 4)
    else:
        recs[:, 16:24] = small.double().view(torch.uint8).view(n, 8)
        recs[:, 24:28] = small.float().view(torch.uint8).view(n, 4)
    return recs.view(-1)


def composition(recs, W, cols):
    n = recs.numel() // W
    srt = sort_records(recs, W, key_bytes=8).view(n, W)
    keys = srt[:, 0:8].contiguous().view(torch.int64).view(n)
    pairs = torch.empty(2 * n, dtype=torch.int64, device=recs.device)
    pairs[0::2] = keys
    out_keys, out = None, []
    for off, dtype, op in cols:
        if op == "count":
            out_keys, v = reduce_by_key_aos(pairs, "count")
            out.append(v)
            continue
        f = srt[:, off:off + SIZE_OF[dtype]].contiguous() \
            .view(TORCH_OF[dtype]).view(n)
        if dtype in ("f32", "f64"):
            pairs[1::2] = f.double().view(torch.int64)
            rop = "sum_f64"
            assert op == "sum"
        else:
            w = f.long()
            if dtype == "u32":
                w = w & 0xFFFFFFFF
            pairs[1::2] = w
            rop = op
        out_keys, v = reduce_by_key_aos(pairs, rop)
        out.append(v)
    return out_keys, out


def lines_per_record(W, cols, line=64):
    """Mean number of distinct `line`-byte lines one record's column fields
    touch, over the record start offsets a dense array of W-byte records
    takes (the key is read by the pair extraction, not here)."""
    starts = sorted({(i * W) % line for i in range(line)})
    tot = 0
    for s in starts:
        touched = set()
        for off, dtype, op in cols:
            if op == "count":
                continue
            a = s + off
            touched.update(range(a // line, (a + SIZE_OF[dtype] - 1) // line + 1))
        tot += len(touched)
    return tot / len(starts)


def device_ms(fn):
    a = torch.cuda.Event(enable_timing=True)
    b = torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def fmt(ts):
    return f"{statistics.median(ts):8.2f} [{min(ts):.2f}..{max(ts):.2f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2-n", type=int, default=26)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--widths", default="16,100,256")
    ap.add_argument("--columns", default="1,4,8")
    ap.add_argument("--log2-keys", default="26,20,0")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_records_agg needs a GPU: nothing is measured without")
    m = load()
    n = 1 << a.log2_n
    T = m.reduce_records_tile()
    print(f"n = 2^{a.log2_n} records, {a.runs} alternating runs after one "
          f"warm-up, device-event ms median [min..max]; tile {T}")
    for W in (int(x) for x in a.widths.split(",")):
        for lk in (int(x) for x in a.log2_keys.split(",")):
            recs = make_records(n, W, lk)
            for C in (int(x) for x in a.columns.split(",")):
                cols = columns_for(W, C)
                nread = sum(op != "count" for _o, _d, op in cols)
                passes = onesweep_passes(0, 64)
                print(f"W {W:3d} C {C} keys 2^{lk:<2d} bytes/record: extract "
                      f"{min(W, 64 * lines_per_record(W, [(0, 'i64', 'sum')])):.0f}"
                      f" read (streamed) + 16 written, sort {passes} x 32 pair bytes, "
                      f"reduce 16 pair + "
                      f"{64 * lines_per_record(W, cols):.0f} record-line + "
                      f"{8 * nread} scratch written + 8 pair-key + "
                      f"{8 * nread} scratch read; composition: "
                      f"sort_records' own extract and pair passes, "
                      f"{2 * W} record bytes in its gather, then per column "
                      f"a strided slice and 32 pair bytes", flush=True)
                k1, v1 = aggregate_records(recs, W, cols)       # warm-up
                k2, v2 = composition(recs, W, cols)
                same = torch.equal(k1, k2) and all(
                    x.dtype == y.dtype and torch.equal(x, y)
                    for x, y in zip(v1, v2))
                groups = k1.numel()
                del k1, v1, k2, v2
                ta, tb = [], []
                for _ in range(a.runs):
                    ta.append(device_ms(
                        lambda: aggregate_records(recs, W, cols)))
                    tb.append(device_ms(lambda: composition(recs, W, cols)))
                ma, mb = statistics.median(ta), statistics.median(tb)
                overlap = not (max(ta) < min(tb) or max(tb) < min(ta))
                print(f"W {W:3d} C {C} keys 2^{lk:<2d} groups {groups:9d} "
                      f"outputs {'equal' if same else 'DIFFER'}: new "
                      f"{fmt(ta)}  composition {fmt(tb)}  x{mb / ma:.2f}"
                      f"{' (ranges overlap)' if overlap else ''}",
                      flush=True)
                if not same:
                    sys.exit("the two arms disagree")
            del recs
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
