"""reduce_by_key over key-sorted AoS pairs (ops/csrc/reduce.hip) vs a numpy
oracle. T = reduce_by_key_tile(); the shapes sit on the tile boundaries, on
runs that cross tiles holding no head, and on the forward walk beyond one
64-tile step.

Every call writes into outputs of EXACTLY g elements and a workspace of
exactly reduce_by_key_workspace_bytes(n), each between canary guards; all
guards must come back untouched and the input pairs unchanged."""

import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CANARY = 0xA5
PAD = 256           # guard bytes on each side (keeps 16-byte alignment)
OPS = ("sum", "sum_f64", "count", "min", "max")
GOLDEN = np.uint64(0x9E3779B97F4A7C15)   # odd: run id -> distinct 64-bit key


@pytest.fixture(scope="module")
def hs():
    from sparkrdma_amd.ops import load
    m = load()
    m.set_device(0)
    return m


@pytest.fixture(scope="module")
def T(hs):
    return hs.reduce_by_key_tile()


def _guarded(nbytes):
    import torch
    buf = torch.full((PAD + nbytes + PAD,), CANARY, dtype=torch.uint8,
                     device="cuda")
    return buf, buf[PAD:PAD + nbytes]


def _check_guards(buf, what):
    got = buf.cpu().numpy()
    assert np.all(got[:PAD] == CANARY), what + ": written before"
    assert np.all(got[-PAD:] == CANARY), what + ": written past the end"


def _heads(k):
    return np.flatnonzero(np.concatenate(([True], k[1:] != k[:-1])))


def _oracle(k, v, op):
    """(run keys u64, reductions as u64 bits); sum_f64 sums left to right
    in float64, exact for the integer-valued inputs it is used with."""
    st = _heads(k)
    if op == "count":
        red = np.diff(np.append(st, len(k))).astype(np.uint64)
    elif op == "sum":
        red = np.add.reduceat(v, st)                     # wraps mod 2^64
    elif op == "sum_f64":
        red = np.add.reduceat(v.view(np.float64), st).view(np.uint64)
    else:
        fn = np.minimum if op == "min" else np.maximum
        red = fn.reduceat(v.view(np.int64), st).view(np.uint64)
    return k[st], red


def _run(hs, k, v, op):
    """reduce_by_key_aos with every buffer between canaries; returns
    (keys u64, value bits u64)."""
    import torch
    from sparkrdma_amd.ops.radix import reduce_by_key_aos
    n = len(k)
    g = len(_heads(k))
    inter = np.empty(2 * n, dtype=np.uint64)
    inter[0::2], inter[1::2] = k, v
    pairs_buf, pairs = _guarded(16 * n)
    pairs.copy_(torch.from_numpy(inter.view(np.uint8)).cuda())
    ok_buf, ok = _guarded(8 * g)
    ov_buf, ov = _guarded(8 * g)
    ws_buf, ws = _guarded(hs.reduce_by_key_workspace_bytes(n))
    keys, vals = reduce_by_key_aos(pairs.view(torch.int64), op,
                                   out_keys=ok.view(torch.int64),
                                   out_vals=ov.view(torch.int64), ws=ws)
    torch.cuda.synchronize()
    assert keys.numel() == g and vals.numel() == g
    assert keys.data_ptr() == ok.data_ptr()
    assert vals.data_ptr() == ov.data_ptr()
    assert vals.dtype == (torch.float64 if op == "sum_f64" else torch.int64)
    for buf, what in ((pairs_buf, "pairs"), (ok_buf, "out_keys"),
                      (ov_buf, "out_vals"), (ws_buf, "ws")):
        _check_guards(buf, what)
    assert np.array_equal(pairs.cpu().numpy().view(np.uint64), inter), \
        "input pairs modified"
    return (keys.cpu().numpy().view(np.uint64),
            vals.cpu().numpy().view(np.uint64))


def _values(rng, n, op):
    if op == "sum":                   # up to 2^62: run sums wrap
        return rng.integers(0, 1 << 62, n, dtype=np.uint64)
    if op == "sum_f64":               # integer-valued: every order is exact
        return rng.integers(0, 1 << 20, n).astype(np.float64).view(np.uint64)
    if op == "count":
        return rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    return rng.integers(-2 ** 63, 2 ** 63 - 1, n, dtype=np.int64) \
        .view(np.uint64)


def _keys_from_heads(h):
    h = h.copy()
    h[0] = True
    return np.cumsum(h).astype(np.uint64) * GOLDEN


def _keys(rng, n, pattern):
    if pattern == "equal":
        return np.full(n, 0xDEADBEEF12345678, dtype=np.uint64)
    if pattern == "distinct":
        # records 2j and 2j+1 differ in bit 63 ONLY: a 32-bit compare or a
        # compare that drops the top bit would merge them
        i = np.arange(n, dtype=np.uint64)
        return (i >> np.uint64(1)) ^ ((i & np.uint64(1)) << np.uint64(63))
    return _keys_from_heads(rng.random(n) < 0.3)


def _check(hs, k, v, op):
    gk, gv = _run(hs, k, v, op)
    wk, wv = _oracle(k, v, op)
    assert np.array_equal(gk, wk), op
    assert np.array_equal(gv, wv), op


@pytest.mark.parametrize("pattern", ["equal", "distinct", "random"])
@pytest.mark.parametrize("op", OPS)
def test_sizes_and_patterns(hs, T, op, pattern):
    rng = np.random.default_rng(OPS.index(op) * 7 + len(pattern))
    for n in (1, 2, T - 1, T, T + 1, 2 * T + 3):
        k = _keys(rng, n, pattern)
        if pattern == "distinct":
            assert len(_heads(k)) == n
        _check(hs, k, _values(rng, n, op), op)


def _boundary_cases(rng, T):
    n = 4 * T
    # A: all heads, but a run of 2 on [T-1, T] and no head in the last tile
    a = np.ones(n, dtype=bool)
    a[T] = False
    a[3 * T - 3 + 1:] = False
    # B: a run ends exactly at T-1, a new one starts at T (tile 1's lead is
    # the identity); random elsewhere
    b = rng.random(n) < 0.3
    b[T - 1] = False
    b[T] = True
    # C: one run on [T-1, 3T+1): tiles 1 and 2 hold no head
    c = rng.random(n) < 0.3
    c[T - 1] = True
    c[T:3 * T + 1] = False
    c[3 * T + 1] = True
    # D: C's long run AND a last tile without a head
    d = c.copy()
    d[3 * T + 1:] = False
    d[3 * T - 7] = True
    d[T:3 * T - 7] = False
    return {"A": a, "B": b, "C": c, "D": d}


@pytest.mark.parametrize("case", ["A", "B", "C", "D"])
def test_tile_boundaries(hs, T, case):
    rng = np.random.default_rng(ord(case))
    h = _boundary_cases(rng, T)[case]
    k = _keys_from_heads(h)
    for op in OPS:
        _check(hs, k, _values(rng, len(k), op), op)


@pytest.mark.parametrize("op", OPS)
def test_walk_beyond_one_step(hs, T, op):
    """first and last keys distinct, one run between: its owner in tile 0
    walks 129 tiles, more than two 64-tile steps."""
    n = 130 * T + 7
    h = np.zeros(n, dtype=bool)
    h[[0, 1, n - 1]] = True
    rng = np.random.default_rng(130)
    _check(hs, _keys_from_heads(h), _values(rng, n, op), op)


def test_sum_f64_fractions(hs, T):
    """random fractions: bit-identical across calls, and each run of
    length L within 2(L-1) 2^-53 sum|v| of math.fsum — the bound for any
    summation order, doubled for the oracle's own rounding."""
    n = 5 * T + 1
    rng = np.random.default_rng(53)
    h = rng.random(n) < 0.01
    h[2 * T - 9:4 * T + 5] = False         # one run across whole tiles
    k = _keys_from_heads(h)
    f = rng.random(n) * 2.0 - 1.0
    v = f.view(np.uint64)
    k1, r1 = _run(hs, k, v, "sum_f64")
    k2, r2 = _run(hs, k, v, "sum_f64")
    assert np.array_equal(k1, k2) and np.array_equal(r1, r2)
    st = _heads(k)
    assert np.array_equal(k1, k[st])
    got = r1.view(np.float64)
    ends = np.append(st[1:], n)
    for g, (a, b) in enumerate(zip(st.tolist(), ends.tolist())):
        run = f[a:b].tolist()
        bound = 2 * (len(run) - 1) * 2.0 ** -53 * math.fsum(map(abs, run))
        assert abs(got[g] - math.fsum(run)) <= bound, (g, a, b)


def _torch_chain(pairs, aggregator):
    """The keyed reduction read_aos ran before the kernel existed."""
    import torch
    k = pairs[0::2].contiguous()
    v = pairs[1::2].contiguous()
    uk, inverse, cnt = torch.unique_consecutive(
        k, return_inverse=True, return_counts=True)
    if aggregator == "count":
        return uk, cnt
    if aggregator == "sum":
        out = torch.zeros(uk.numel(), dtype=torch.int64, device=k.device)
        out.index_add_(0, inverse, v)
        return uk, out
    red = "amin" if aggregator == "min" else "amax"
    out = torch.empty(uk.numel(), dtype=torch.int64, device=k.device)
    out.scatter_reduce_(0, inverse, v, reduce=red, include_self=False)
    return uk, out


def test_integer_ops_match_torch_chain(hs, T):
    import torch
    from sparkrdma_amd.ops.radix import reduce_by_key_aos
    n = 5 * T + 1
    rng = np.random.default_rng(5)
    k = np.sort(rng.integers(0, n // 3, n, dtype=np.uint64))
    for op in ("sum", "count", "min", "max"):
        v = _values(rng, n, "min" if op == "count" else op)
        inter = np.empty(2 * n, dtype=np.uint64)
        inter[0::2], inter[1::2] = k, v
        pairs = torch.from_numpy(inter.view(np.int64)).cuda()
        gk, gv = reduce_by_key_aos(pairs, op)
        wk, wv = _torch_chain(pairs, op)
        assert gk.dtype == wk.dtype and gv.dtype == wv.dtype
        assert torch.equal(gk, wk), op
        assert torch.equal(gv, wv), op


def test_small_outputs_and_empty_input(hs, T):
    import torch
    from sparkrdma_amd.ops.radix import reduce_by_key_aos
    k, v = reduce_by_key_aos(torch.empty(0, dtype=torch.int64, device="cuda"),
                             "sum")
    assert k.numel() == 0 and v.numel() == 0
    assert k.dtype == torch.int64 and v.dtype == torch.int64
    pairs = torch.arange(2 * 10, dtype=torch.int64, device="cuda")  # 10 runs
    small = torch.empty(9, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError):
        reduce_by_key_aos(pairs, "sum", out_keys=small)
    with pytest.raises(ValueError):
        reduce_by_key_aos(pairs, "sum", out_vals=small)
    with pytest.raises(ValueError):
        reduce_by_key_aos(pairs, "median")
