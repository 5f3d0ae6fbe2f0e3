"""Keyed aggregation of wide records on the GPU (ops/csrc/reduce_records.hip
through ops.radix.reduce_records_by_key / aggregate_records and
ShuffleReader.read_records_agg) against numpy oracles.

T = reduce_records_tile(). Every output, workspace and pair buffer of the
kernel-level tests sits between canary guards: outputs are sized exactly g
(keys) and C * g (values), the workspace exactly
reduce_records_workspace_bytes(n, C); guards must come back intact, records
and pairs unchanged. The pairs address the records through a random
permutation and carry junk in the aux word's top 16 bits, which the kernel
must mask off. Float inputs are integer-valued with magnitude < 2^20, so
every f64 partial sum is exact and order-free: everything compares with ==.
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CANARY = 0xA5
PAD = 256           # guard bytes on each side (keeps 16-byte alignment)
GOLDEN = np.uint64(0x9E3779B97F4A7C15)   # odd: run id -> distinct 64-bit key
NP_OF = {"i32": "<i4", "u32": "<u4", "i64": "<i8", "f32": "<f4", "f64": "<f8"}

# W = 100: i64 at 12 (8-byte fields at addresses 4 mod 8 for odd records),
# f64 at 92 (the last 8 bytes), i32 at 96, a column over the key's low half
COLS_100 = ((12, "i64", "sum"), (92, "f64", "sum"), (96, "i32", "min"),
            (20, "u32", "max"), (24, "i32", "sum"), (28, "f32", "max"),
            (0, "u32", "min"), (None, None, "count"))
COLS_16 = ((8, "i64", "sum"), (8, "i64", "min"), (8, "i64", "max"),
           (12, "i32", "sum"), (8, "u32", "sum"), (4, "u32", "max"),
           (None, None, "count"))
COLS_256 = ((248, "f64", "min"), (8, "f64", "max"), (8, "f64", "sum"),
            (128, "f32", "sum"), (132, "f32", "min"), (252, "u32", "sum"),
            (64, "i64", "max"), (252, "i32", "sum"))


@pytest.fixture(scope="module")
def hs():
    from sparkrdma_amd.ops import load
    m = load()
    m.set_device(0)
    return m


@pytest.fixture(scope="module")
def T(hs):
    return hs.reduce_records_tile()


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


def _keys_from_heads(h):
    h = h.copy()
    h[0] = True
    return np.cumsum(h).astype(np.uint64) * GOLDEN


def _keys(rng, n, T, structure):
    if structure == "equal":
        return np.full(n, 0xDEADBEEF12345678, dtype=np.uint64)
    if structure == "distinct":
        # records 2j and 2j+1 differ in bit 63 ONLY, 2j+1 and 2j+2 in the
        # low bits only
        i = np.arange(n, dtype=np.uint64)
        return (i >> np.uint64(1)) ^ ((i & np.uint64(1)) << np.uint64(63))
    if structure == "half_tile":
        # runs of T/2 + 1: tiles alternate between one head and none
        return _keys_from_heads(np.arange(n) % (T // 2 + 1) == 0)
    h = np.zeros(n, dtype=bool)                       # run lengths 1..300
    starts = np.cumsum(rng.integers(1, 301, n))
    h[starts[starts < n]] = True
    return _keys_from_heads(h)


def _put(rows, off, a):
    rows[:, off:off + a.dtype.itemsize] = \
        a.view(np.uint8).reshape(len(rows), a.dtype.itemsize)


def _field(rows, off, dtype):
    nd = np.dtype(NP_OF[dtype])
    return rows[:, off:off + nd.itemsize].copy().view(nd).reshape(-1)


def _records(rng, keys_sorted, W, columns, fractions=False):
    """(rows uint8 [n, W], perm): row perm[i] holds the i-th sorted key.
    Bytes are random; every non-count column's field is then overwritten
    with a small integer value of its dtype (or a fraction), later columns
    winning where fields overlap; the key goes in last."""
    n = len(keys_sorted)
    rows = rng.integers(0, 256, (n, W), dtype=np.uint8)
    for off, dtype, op in columns:
        if op == "count" or off < 8:
            continue
        if dtype in ("f32", "f64"):
            v = rng.integers(-(1 << 20) + 1, 1 << 20, n).astype(np.float64)
            if fractions:
                v = v + rng.random(n)
            _put(rows, off, v.astype(NP_OF[dtype]))
        elif dtype == "i64":
            _put(rows, off, rng.integers(-(1 << 40), 1 << 40, n).astype("<i8"))
        # i32 / u32: the random bytes are the values, all 32 bits in play
    perm = rng.permutation(n)
    if W >= 8:
        k = np.empty(n, dtype=np.uint64)
        k[perm] = keys_sorted
        _put(rows, 0, k.astype("<u8"))
    return rows, perm


def _oracle(rows, perm, keys_sorted, columns):
    st = _heads(keys_sorted)
    n = len(keys_sorted)
    out = []
    for off, dtype, op in columns:
        if op == "count":
            out.append(np.diff(np.append(st, n)).astype(np.int64))
            continue
        v = _field(rows, off, dtype)[perm]
        v = v.astype(np.float64 if dtype in ("f32", "f64") else np.int64)
        fn = {"sum": np.add, "min": np.minimum, "max": np.maximum}[op]
        out.append(fn.reduceat(v, st))
    return keys_sorted[st], out


def _pairs_np(keys_sorted, perm, idx_base=0):
    inter = np.empty(2 * len(perm), dtype=np.uint64)
    inter[0::2] = keys_sorted
    inter[1::2] = (perm.astype(np.uint64) + np.uint64(idx_base)) \
        | (np.uint64(0xBEEF) << np.uint64(48))
    return inter


def _run(hs, rows, perm, keys_sorted, columns, split=None):
    """reduce_records_by_key with every buffer between canaries. ``split``:
    record counts of separately allocated segments. Returns (keys u64,
    [column arrays])."""
    import torch
    from sparkrdma_amd.ops.radix import reduce_records_by_key
    n, W = rows.shape
    C = len(columns)
    g = len(_heads(keys_sorted))
    inter = _pairs_np(keys_sorted, perm)
    pairs_buf, pairs = _guarded(16 * n)
    pairs.copy_(torch.from_numpy(inter.view(np.uint8)).cuda())
    bounds = np.cumsum([0] + list(split or [n]))
    assert bounds[-1] == n
    rec_bufs, segments = [], []
    for a, b in zip(bounds[:-1], bounds[1:]):
        buf, rec = _guarded(int(b - a) * W)
        rec.copy_(torch.from_numpy(rows[a:b].reshape(-1)).cuda())
        rec_bufs.append((buf, rec, int(a), int(b)))
        segments.append((int(a), int(b - a), rec.data_ptr()))
    ok_buf, ok = _guarded(8 * g)
    ov_buf, ov = _guarded(8 * g * C)
    ws_buf, ws = _guarded(hs.reduce_records_workspace_bytes(n, C))
    if split is None:
        keys, vals = reduce_records_by_key(
            pairs.view(torch.int64), rec_bufs[0][1], W, columns,
            out_keys=ok.view(torch.int64), out_vals=ov.view(torch.int64),
            ws=ws)
    else:
        keys, vals = reduce_records_by_key(
            pairs.view(torch.int64), n * W, W, columns, segments=segments,
            out_keys=ok.view(torch.int64), out_vals=ov.view(torch.int64),
            ws=ws)
    torch.cuda.synchronize()
    assert keys.numel() == g and len(vals) == C
    assert keys.data_ptr() == ok.data_ptr()
    for c, ((_off, dtype, op), v) in enumerate(zip(columns, vals)):
        assert v.numel() == g
        assert v.data_ptr() == ov.data_ptr() + 8 * g * c
        isfloat = op != "count" and dtype in ("f32", "f64")
        assert v.dtype == (torch.float64 if isfloat else torch.int64)
    for buf, what in ((pairs_buf, "pairs"), (ok_buf, "out_keys"),
                      (ov_buf, "out_vals"), (ws_buf, "ws")):
        _check_guards(buf, what)
    for buf, rec, a, b in rec_bufs:
        _check_guards(buf, "records")
        assert np.array_equal(rec.cpu().numpy(), rows[a:b].reshape(-1)), \
            "records modified"
    assert np.array_equal(pairs.cpu().numpy().view(np.uint64), inter), \
        "input pairs modified"
    return (keys.cpu().numpy().view(np.uint64),
            [v.cpu().numpy() for v in vals])


def _check(hs, rows, perm, keys_sorted, columns, split=None):
    gk, gv = _run(hs, rows, perm, keys_sorted, columns, split)
    wk, wv = _oracle(rows, perm, keys_sorted, columns)
    assert np.array_equal(gk, wk)
    for col, g, w in zip(columns, gv, wv):
        assert g.dtype == w.dtype, col
        assert np.array_equal(g, w), col
    return gk, gv


def _records_100(rng, keys_sorted):
    # (96, i32) reads the high dword of the f64 at 92: plain bits, and any
    # bits are a valid integer column
    return _records(rng, keys_sorted, 100, COLS_100)


@pytest.mark.parametrize("structure", ["distinct", "equal", "half_tile",
                                       "random"])
def test_edge_sizes_w100(hs, T, structure):
    rng = np.random.default_rng(len(structure))
    for n in (1, T - 1, T, T + 1, 2 * T + 3, 65 * T + 5):
        k = _keys(rng, n, T, structure)
        if structure == "distinct":
            assert len(_heads(k)) == n
        if structure == "half_tile" and n > T:
            assert len(_heads(k)) == -(-n // (T // 2 + 1))
        rows, perm = _records_100(rng, k)
        _check(hs, rows, perm, k, COLS_100)


def test_keys_differ_in_one_bit(hs):
    a = 0x0123456789ABCDEE
    k = np.array([a, a, a ^ 1, a ^ 1, (a ^ 1) ^ (1 << 63), (a ^ 1) ^ (1 << 63),
                  a ^ (1 << 63) ^ (1 << 32), a ^ (1 << 63)], dtype=np.uint64)
    rng = np.random.default_rng(1)
    rows, perm = _records_100(rng, k)
    gk, gv = _check(hs, rows, perm, k, COLS_100)
    assert len(gk) == 5 and gv[-1].tolist() == [2, 2, 2, 1, 1]


def test_w8_count_only(hs, T):
    rng = np.random.default_rng(8)
    for n in (1, T + 1, 3 * T + 9):
        k = _keys(rng, n, T, "random")
        rows, perm = _records(rng, k, 8, ())
        _check(hs, rows, perm, k, [(None, None, "count")])
        _check(hs, rows, perm, k, [(4, "u32", "max"), (0, "i64", "min"),
                                   (None, None, "count")])


def test_w16(hs, T):
    rng = np.random.default_rng(16)
    for n in (T - 1, 2 * T + 3):
        k = _keys(rng, n, T, "random")
        rows, perm = _records(rng, k, 16, ())      # all 64 value bits random
        _check(hs, rows, perm, k, COLS_16)
    # f64 at 8: the whole payload is one double
    k = _keys(rng, 2 * T + 3, T, "half_tile")
    cols = [(8, "f64", "sum"), (8, "f64", "min"), (8, "f64", "max")]
    rows, perm = _records(rng, k, 16, cols)
    _check(hs, rows, perm, k, cols)


def test_w256_eight_columns(hs, T):
    rng = np.random.default_rng(256)
    for n, structure in ((T + 1, "random"), (5 * T + 77, "random"),
                         (3 * T, "equal")):
        k = _keys(rng, n, T, structure)
        # (252, u32/i32) read the high dword of the f64 at 248: plain bits
        rows, perm = _records(rng, k, 256, COLS_256)
        _check(hs, rows, perm, k, COLS_256)


def test_sign_and_zero_extension(hs, T):
    """u32 0xFFFFFFFF and i32 -1 are the same bits: the sums tell the
    extensions apart."""
    n = 2 * T + 3
    rng = np.random.default_rng(32)
    k = _keys(rng, n, T, "half_tile")
    rows, perm = _records(rng, k, 100, ())
    rows[:, 20:24] = 0xFF
    cols = [(20, "u32", "sum"), (20, "i32", "sum"), (20, "u32", "min"),
            (20, "i32", "max"), (None, None, "count")]
    _gk, gv = _check(hs, rows, perm, k, cols)
    assert np.array_equal(gv[0], gv[4] * 0xFFFFFFFF)
    assert np.array_equal(gv[1], -gv[4])
    assert set(gv[2].tolist()) == {0xFFFFFFFF} and set(gv[3].tolist()) == {-1}


def test_i64_sum_wraps(hs, T):
    n = 3 * T + 1
    rng = np.random.default_rng(63)
    k = _keys(rng, n, T, "random")
    rows, perm = _records(rng, k, 100, ())
    v = rng.integers((1 << 63) - (1 << 40), (1 << 63) - 1, n).astype("<i8")
    _put(rows, 12, v)
    cols = [(12, "i64", "sum"), (12, "i64", "max"), (12, "i64", "min")]
    _gk, gv = _check(hs, rows, perm, k, cols)
    assert (gv[0] < 0).any(), "no run sum wrapped: the case tests nothing"


def _fraction_case(T):
    n = 5 * T + 1
    rng = np.random.default_rng(53)
    h = rng.random(n) < 0.01
    h[2 * T - 9:4 * T + 5] = False         # one run across whole tiles
    k = _keys_from_heads(h)
    cols = [(12, "f64", "sum"), (92, "f64", "sum"), (28, "f32", "sum"),
            (28, "f32", "min"), (None, None, "count")]
    rows, perm = _records(rng, k, 100, cols, fractions=True)
    return k, cols, rows, perm


def test_three_segments_bit_identical(hs, T):
    """Three separately allocated segments, one of them a single record:
    bit-identical to the contiguous call, non-integer f64 sums included
    (same order, same bits)."""
    k, cols, rows, perm = _fraction_case(T)
    n = len(k)
    bk, bv = _run(hs, rows, perm, k, cols)
    for split in ([2 * T + 7, 1, n - 2 * T - 8], [1, n - 2, 1]):
        gk, gv = _run(hs, rows, perm, k, cols, split=split)
        assert np.array_equal(gk, bk)
        for a, b in zip(gv, bv):
            assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    # and the integer-valued layout against the oracle
    rng = np.random.default_rng(3)
    k = _keys(rng, 2 * T + 3, T, "random")
    rows, perm = _records_100(rng, k)
    _check(hs, rows, perm, k, COLS_100, split=[T, 1, T + 2])


def test_f64_sum_reproducible_and_close(hs, T):
    import math
    k, cols, rows, perm = _fraction_case(T)
    k1, v1 = _run(hs, rows, perm, k, cols)
    k2, v2 = _run(hs, rows, perm, k, cols)
    assert np.array_equal(k1, k2)
    for a, b in zip(v1, v2):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    # any summation order is within 2(L-1) 2^-53 sum|v| of math.fsum
    # (doubled for the oracle's own rounding)
    f = _field(rows, 12, "f64")[perm]
    st = _heads(k)
    ends = np.append(st[1:], len(k))
    for g, (a, b) in enumerate(zip(st.tolist(), ends.tolist())):
        run = f[a:b].tolist()
        bound = 2 * (len(run) - 1) * 2.0 ** -53 * math.fsum(map(abs, run))
        assert abs(v1[0][g] - math.fsum(run)) <= bound, (g, a, b)


def _sorted_case(rng, n, nkeys, W, columns):
    """Unsorted rows with random keys, for aggregate_records."""
    k = np.sort(rng.integers(0, nkeys, n, dtype=np.uint64)) * GOLDEN
    rows, _perm = _records(rng, np.sort(k), W, columns)
    return rows


def test_aggregate_records_matches_mirror(hs, T):
    import torch
    from sparkrdma_amd.aggregate import reduce_records_np
    from sparkrdma_amd.ops.radix import aggregate_records
    rng = np.random.default_rng(77)
    n = 3 * T + 11
    rows = _sorted_case(rng, n, 500, 100, COLS_100)
    wk, wv = reduce_records_np(rows, COLS_100)
    assert len(wk) > 400
    recs = torch.from_numpy(rows.reshape(-1)).cuda()
    keep = recs.clone()
    for segmented in (False, True):
        if segmented:
            cuts = [0, T + 5, T + 6, n]
            parts = [torch.from_numpy(rows[a:b].reshape(-1)).cuda()
                     for a, b in zip(cuts[:-1], cuts[1:])]
            segs = [(a, b - a, p.data_ptr())
                    for a, b, p in zip(cuts[:-1], cuts[1:], parts)]
            keys, vals = aggregate_records(n * 100, 100, COLS_100,
                                           segments=segs)
        else:
            keys, vals = aggregate_records(recs, 100, COLS_100)
        torch.cuda.synchronize()
        assert np.array_equal(keys.cpu().numpy(), wk)
        for col, g, w in zip(COLS_100, vals, wv):
            g = g.cpu().numpy()
            assert g.dtype == w.dtype and np.array_equal(g, w), col
    assert torch.equal(recs, keep)
    # keys below 2^16 sorted by 16 bits only
    rows[:, 2:8] = 0
    wk, wv = reduce_records_np(rows, COLS_100, end_bit=16)
    keys, vals = aggregate_records(
        torch.from_numpy(rows.reshape(-1)).cuda(), 100, COLS_100, end_bit=16)
    assert np.array_equal(keys.cpu().numpy(), wk)
    assert all(np.array_equal(g.cpu().numpy(), w) for g, w in zip(vals, wv))
    # empty input: empty tensors of the right dtypes
    keys, vals = aggregate_records(
        torch.empty(0, dtype=torch.uint8, device="cuda"), 100, COLS_100)
    assert keys.numel() == 0 and keys.dtype == torch.int64
    assert [v.dtype for v in vals] == [
        torch.float64 if (op != "count" and dt in ("f32", "f64"))
        else torch.int64 for _o, dt, op in COLS_100]


def test_small_buffers_raise_before_any_write(hs, T):
    import torch
    from sparkrdma_amd.ops.radix import reduce_records_by_key
    n, W = T + 9, 16
    rng = np.random.default_rng(9)
    k = _keys(rng, n, T, "distinct")
    rows, perm = _records(rng, k, W, ())
    cols = [(8, "i64", "sum"), (None, None, "count")]
    pairs = torch.from_numpy(_pairs_np(k, perm).view(np.int64)).cuda()
    recs = torch.from_numpy(rows.reshape(-1)).cuda()
    need = hs.reduce_records_workspace_bytes(n, 2)
    for kw, nbytes in (("out_vals", 8 * (2 * n - 1)), ("out_keys", 8 * (n - 1)),
                       ("ws", need - 8)):
        buf, view = _guarded(nbytes)
        arg = view if kw == "ws" else view.view(torch.int64)
        with pytest.raises(ValueError):
            reduce_records_by_key(pairs, recs, W, cols, **{kw: arg})
        torch.cuda.synchronize()
        assert bool((buf == CANARY).all().item()), kw + " was written"
    with pytest.raises(ValueError):                      # C = 9
        reduce_records_by_key(pairs, recs, W, [(8, "i64", "sum")] * 9)
    with pytest.raises(ValueError):
        hs.reduce_records_workspace_bytes(n, 9)
    assert hs.reduce_records_max_columns() == 8
    with pytest.raises(ValueError):                      # field past the record
        reduce_records_by_key(pairs, recs, W, [(12, "i64", "sum")])
    with pytest.raises(ValueError):                      # native check too
        hs.reduce_records_count(pairs.data_ptr(), n, recs.data_ptr(), W, 0, 0,
                                [3], [2], [0], 0, 0)
    with pytest.raises(ValueError):                      # rec_bytes % 4
        hs.reduce_records_count(pairs.data_ptr(), n, recs.data_ptr(), 18, 0,
                                0, [2], [0], [0], 0, 0)
    with pytest.raises(ValueError):                      # unknown op code
        hs.reduce_records_count(pairs.data_ptr(), n, recs.data_ptr(), W, 0, 0,
                                [2], [0], [4], 0, 0)


# ---------------------------------------------------------------------------
# reader end to end

W_REC, N_MAP, R_PARTS = 100, 5000, 8


@pytest.fixture
def manager(tmp_path):
    from sparkrdma_amd.conf import ShuffleConf
    from sparkrdma_amd.driver import Driver
    from sparkrdma_amd.manager import ShuffleManager
    conf = ShuffleConf(shm_dir=str(tmp_path), transport="ipc",
                       hbm_pool_size=1 << 30,
                       shuffle_write_block_size=256 << 10,
                       shuffle_read_block_size=4 << 10)
    driver = Driver(conf)
    mgr = ShuffleManager(conf, executor_id=0, driver_port=driver.port)
    yield mgr
    mgr.stop()
    driver.stop()


@pytest.mark.parametrize("kind", ["plain", "in_place"])
def test_reader_end_to_end(manager, kind):
    import torch
    from sparkrdma_amd.aggregate import reduce_records_np
    from sparkrdma_amd.partitioner import HashPartitioner
    rng = np.random.default_rng(100)
    maps = [_sorted_case(rng, N_MAP, 700, W_REC, COLS_100) for _ in range(2)]
    handle = manager.register_shuffle(num_maps=2, num_partitions=R_PARTS)
    for mid, rows in enumerate(maps):
        w = manager.get_writer(handle, mid)
        w.write_device_records(torch.from_numpy(rows.reshape(-1)).cuda(),
                               W_REC, key_bytes=8)
        w.stop(True, partitioner=HashPartitioner(R_PARTS))
    torch.cuda.synchronize()
    if kind == "plain":
        reader = manager.get_reader(handle, 0, R_PARTS - 1)
    else:
        cap = 2 * N_MAP * W_REC + 4096
        hint = torch.full((cap,), 0x5A, dtype=torch.uint8, device="cuda")
        pairs = torch.full((2 * (cap // W_REC) + 16,), -1, dtype=torch.int64,
                           device="cuda")
        reader = manager.get_reader(handle, 0, R_PARTS - 1, arena=hint,
                                    records=(W_REC, 8, pairs), in_place=True)
        with pytest.raises(ValueError):        # disagrees with the spec
            reader.read_records_agg(64, [(None, None, "count")])
    keys, vals = reader.read_records_agg(W_REC, COLS_100)
    torch.cuda.synchronize()                   # before unregister_shuffle
    wk, wv = reduce_records_np(np.concatenate(maps), COLS_100)
    assert np.array_equal(keys.cpu().numpy(), wk)
    for col, g, w in zip(COLS_100, vals, wv):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and np.array_equal(g, w), col
    if kind == "in_place" \
            and manager.conf.fused_record_fetch == "inplace":
        # every block is this executor's: nothing was copied
        assert reader.fetcher.arena is None
        assert bool((hint == 0x5A).all().item())
    manager.unregister_shuffle(handle.shuffle_id)


def test_reader_refuses_ten_byte_keys(manager):
    import torch
    from sparkrdma_amd.partitioner import RangePartitioner
    handle = manager.register_shuffle(num_maps=1, num_partitions=2)
    rng = np.random.default_rng(10)
    rows = rng.integers(0, 256, (64, W_REC), dtype=np.uint8)
    w = manager.get_writer(handle, 0)
    w.write_device_records(torch.from_numpy(rows.reshape(-1)).cuda(), W_REC,
                           key_bytes=10)
    w.stop(True, partitioner=RangePartitioner.uniform(2))
    torch.cuda.synchronize()
    pairs = torch.empty(2 * 64 + 16, dtype=torch.int64, device="cuda")
    hint = torch.empty(64 * W_REC + 4096, dtype=torch.uint8, device="cuda")
    reader = manager.get_reader(handle, 0, 1, arena=hint,
                                records=(W_REC, 10, pairs))
    with pytest.raises(ValueError):
        reader.read_records_agg(W_REC, [(None, None, "count")])
    for _ in reader:
        pass
    torch.cuda.synchronize()
    manager.unregister_shuffle(handle.shuffle_id)


def test_group_by_aggregate_workload(tmp_path):
    from sparkrdma_amd.conf import ShuffleConf
    from sparkrdma_amd.engine import Engine
    from sparkrdma_amd.workloads import GroupByAggregate
    conf = ShuffleConf(shm_dir=str(tmp_path), transport="ipc",
                       hbm_pool_size=1 << 30)
    eng = Engine(conf, rank=0, world_size=1, driver_port=0)
    try:
        for in_place in (False, True):
            wl = GroupByAggregate(eng, rows_per_executor=20_000,
                                  num_keys=1500, partitions_per_executor=8,
                                  device="cuda", validate=True,
                                  in_place=in_place)
            res = wl.run_step()
            assert res.groups == 1500 and res.rows == 20_000
            assert res.shuffle_bytes == 20_000 * 64
    finally:
        eng.shutdown()
