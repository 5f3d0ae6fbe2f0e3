"""Bench of the join family against the inner-only merge join on one MI355X.

Run on a GPU box:
  python scripts/bench_join.py [log2_n] [runs]

Two key-sorted tables of 2^log2_n (key u64, payload u64) rows a side
(default 24), three key distributions:

  a  keys from a 32-bit space, near-unique: the sql_join workload's shape
  b  keys from a 20-bit space: about 2^(log2_n - 20) duplicates a side
  c  shape a plus one hot key of 2^14 rows on each side

On every shape merge_join_sorted (join_count / join_emit) and
merge_join(how="inner") (join.hip) alternate in one process after warm-up,
their outputs are compared equal, and median and range over the runs are
printed; the other five join types are timed on a and b. Times are host
clock around the whole call, synchronised before and after: the probe,
the scan, the readback of the total, the output allocation and the
expansion. Bytes are those a call must move — every input word read once,
every output word written once — so GB/s is a call rate, not a kernel's
share of peak.
"""

import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from sparkrdma_amd.joins import JOIN_TYPES
from sparkrdma_amd.ops import load
from sparkrdma_amd.ops.join import merge_join, merge_join_sorted

HOT_ROWS = 1 << 14


def make_side(n, bits, seed, hot=False):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    k = torch.randint(0, 1 << bits, (n,), dtype=torch.int64, device="cuda",
                      generator=g)
    if hot:
        k[:HOT_ROWS] = 1 << (bits - 1)
    k = torch.sort(k).values.contiguous()
    return k, k.clone()                 # payload := key, as in the workload


def must_move_bytes(na, nb, rows, how):
    """Inputs read once (keys and payloads of both sides), outputs written
    once: key + A payload (+ B payload unless semi / anti) per row, and
    the two validity bytes where a join type can produce nulls."""
    two_sided = how not in ("left_semi", "left_anti")
    per_row = 16 + (8 if two_sided else 0)
    if how.endswith("_outer"):
        per_row += 2
    return 16 * (na + nb) + per_row * rows


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def fmt(ts):
    return f"{statistics.median(ts):8.2f} [{min(ts):.2f}..{max(ts):.2f}]"


def bench(log2_n=24, runs=10):
    load()
    n = 1 << log2_n
    print(f"n = 2^{log2_n} rows a side, {runs} alternating runs, ms median "
          "[min..max], GB/s from the bytes a call must move", flush=True)
    for shape, bits, hot in (("a", 32, False), ("b", 20, False),
                             ("c", 32, True)):
        ak, av = make_side(n, bits, 1, hot)
        bk, bv = make_side(n, bits, 2, hot)

        def old():
            return merge_join_sorted(ak, av, bk, bv)

        def new(how="inner"):
            return merge_join(ak, av, bk, bv, how=how)

        for _ in range(2):                               # warm-up
            o = old()
            f = new()
        rows = f.keys.numel()
        same = (torch.equal(o[0], f.keys) and torch.equal(o[1], f.a_vals)
                and torch.equal(o[2], f.b_vals))
        del o, f
        t_old, t_new = [], []
        for _ in range(runs):
            t_old.append(timed(old)[0])
            t_new.append(timed(new)[0])
        gb = must_move_bytes(n, n, rows, "inner") / 1e9
        m_old, m_new = statistics.median(t_old), statistics.median(t_new)
        print(f"shape {shape} inner rows {rows}: sorted {fmt(t_old)} "
              f"{gb / m_old * 1e3:7.1f} GB/s | family {fmt(t_new)} "
              f"{gb / m_new * 1e3:7.1f} GB/s | sorted/family "
              f"x{m_old / m_new:.2f} | outputs equal: {same}", flush=True)
        if not same:
            raise SystemExit("the two inner paths disagree")
        if shape == "c":
            continue
        for how in JOIN_TYPES[1:]:
            for _ in range(2):
                rows = new(how).keys.numel()
            ts = [timed(lambda: new(how))[0] for _ in range(runs)]
            gb = must_move_bytes(n, n, rows, how) / 1e9
            print(f"shape {shape} {how} rows {rows}: family {fmt(ts)} "
                  f"{gb / statistics.median(ts) * 1e3:7.1f} GB/s",
                  flush=True)
        del ak, av, bk, bv
        torch.cuda.empty_cache()


if __name__ == "__main__":
    bench(*(int(a) for a in sys.argv[1:3]))
