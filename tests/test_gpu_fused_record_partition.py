"""The fused map-side partition of wide records (digits of at most 8 bits):
count_pair_digits + partition_records_fused (ops/csrc/kernels.hip) against
a numpy oracle — partition ids, then for each partition its records in
input order — at the native entries, through the writer on both sides of
the 8/9-bit seam, and through partition_records.

The onesweep tile is 4096 records and a copy batch 4096 words; the sizes
below sit on and around both."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 4096
GUARD = 68          # guard bytes round a destination: 4-byte aligned only
GUARD_BYTE = 0xA5


@pytest.fixture(scope="module")
def hs():
    from sparkrdma_amd.ops import load
    m = load()
    m.set_device(0)
    return m


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _records(rng, n, W):
    """Random rows whose bytes [8, 12) hold the row's input index."""
    arr = rng.integers(0, 256, (n, W), dtype=np.uint8)
    arr[:, 8:12] = np.arange(n, dtype="<u4").view(np.uint8).reshape(n, 4)
    return arr


def _tags(rows):
    return rows[:, 8:12].copy().view("<u4").ravel()


def _pairs(rng, ids):
    """(id, aux) pairs in input order; the aux word's high 16 bits are
    noise the kernels must mask off."""
    n = len(ids)
    pr = np.empty((n, 2), dtype=np.uint64)
    pr[:, 0] = ids
    pr[:, 1] = (rng.integers(0, 1 << 16, n, dtype=np.uint64) << np.uint64(48)
                | np.arange(n, dtype=np.uint64))
    return pr


def _counts(hs, pairs_t, n):
    import torch
    totals = torch.full((256,), -1, dtype=torch.int32, device="cuda")
    hs.count_pair_digits(pairs_t.data_ptr(), n, totals.data_ptr(), _stream())
    return totals.cpu().numpy().astype(np.int64)


def _run_fused(hs, rng, arr, ids):
    """Partition ``arr`` by ``ids`` through the native entries into one
    guarded allocation per non-empty partition, allocated in a shuffled
    order; returns nothing, asserts everything."""
    import torch
    n, W = arr.shape
    recs = torch.from_numpy(arr.reshape(-1)).cuda()
    pairs_t = torch.from_numpy(_pairs(rng, ids).view(np.int64).reshape(-1)) \
        .cuda()
    want = np.bincount(ids, minlength=256)
    counts = _counts(hs, pairs_t, n)
    assert np.array_equal(counts, want)

    bufs = {}
    for p in rng.permutation(256):
        if want[p]:
            bufs[int(p)] = torch.full((2 * GUARD + int(want[p]) * W,),
                                      GUARD_BYTE, dtype=torch.uint8,
                                      device="cuda")
    table = np.zeros(256, dtype=np.int64)      # empty partitions: address 0
    for p, b in bufs.items():
        table[p] = b.data_ptr() + GUARD
    table_t = torch.from_numpy(table).cuda()
    ws = torch.empty(hs.partition_records_workspace_bytes(n),
                     dtype=torch.uint8, device="cuda")
    hs.partition_records_fused(pairs_t.data_ptr(), n, recs.data_ptr(), W,
                               table_t.data_ptr(), ws.data_ptr(), _stream())
    torch.cuda.synchronize()
    order = sorted(bufs)
    flat = torch.cat([bufs[p] for p in order]).cpu().numpy()
    pos = 0
    for p in order:
        size = 2 * GUARD + int(want[p]) * W
        got = flat[pos:pos + size]
        pos += size
        assert (got[:GUARD] == GUARD_BYTE).all(), f"guard before {p}"
        assert (got[-GUARD:] == GUARD_BYTE).all(), f"guard after {p}"
        rows = got[GUARD:-GUARD].reshape(-1, W)
        exp = arr[ids == p]
        assert np.array_equal(_tags(rows), _tags(exp)), \
            f"partition {p}: wrong records or order"
        assert np.array_equal(rows, exp), f"partition {p}: bytes differ"


@pytest.mark.parametrize("spread", [256, 16, 3])
@pytest.mark.parametrize("W", [12, 24, 100, 256])
@pytest.mark.parametrize("n", [1, TILE - 1, TILE, TILE + 1, 5 * TILE + 17,
                               64 * TILE])
def test_native_entry_matches_oracle(hs, n, W, spread):
    rng = np.random.default_rng(n * 1000 + W * 10 + spread)
    arr = _records(rng, n, W)
    # the ids in use are spread over the whole byte, not the low values
    used = rng.permutation(256)[:spread]
    ids = used[rng.integers(0, spread, n)].astype(np.int64)
    _run_fused(hs, rng, arr, ids)


def _degenerate_ids(kind, n):
    if kind == "one":
        return np.full(n, 7, dtype=np.int64)
    if kind == "cycle":
        return np.arange(n, dtype=np.int64) % 256
    # one partition holds all but one record of every tile
    ids = np.full(n, 5, dtype=np.int64)
    for t, first in enumerate(range(0, n, TILE)):
        ids[min(first + 100, n - 1)] = 200 + t
    return ids


@pytest.mark.parametrize("kind", ["one", "cycle", "all_but_one"])
def test_degenerate_distributions(hs, kind):
    n, W = 3 * TILE + 5, 100
    rng = np.random.default_rng(len(kind))
    _run_fused(hs, rng, _records(rng, n, W), _degenerate_ids(kind, n))


@pytest.mark.parametrize("n", [0, 1, TILE, 5 * TILE + 17])
def test_counts_entry(hs, n):
    import torch
    rng = np.random.default_rng(n)
    ids = rng.integers(0, 256, n).astype(np.int64)
    pairs_t = torch.from_numpy(_pairs(rng, ids).view(np.int64).reshape(-1)) \
        .cuda()
    assert np.array_equal(_counts(hs, pairs_t, n),
                          np.bincount(ids, minlength=256))


def test_native_entry_rejects_bad_arguments(hs):
    import torch
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    p = buf.data_ptr()
    ok = dict(pairs=p, n=1, recs=p, rec_bytes=100, dst_table=p, ws=p)
    for bad in (dict(rec_bytes=10), dict(rec_bytes=0), dict(pairs=p + 8),
                dict(recs=p + 2), dict(dst_table=p + 4), dict(ws=p + 4)):
        with pytest.raises(RuntimeError):
            hs.partition_records_fused(**{**ok, **bad})
    with pytest.raises(TypeError):
        hs.partition_records_fused(**{**ok, "n": 1 << 32})
    with pytest.raises(RuntimeError):
        hs.count_pair_digits(p + 8, 1, p)
    torch.cuda.synchronize()


# -- writer level ----------------------------------------------------------

def _partitioner(kind, R, prefix):
    from sparkrdma_amd.partitioner import HashPartitioner, RangePartitioner
    if kind == "hash":
        return HashPartitioner(R)
    if kind == "bounds":
        return RangePartitioner.from_sample(prefix[::7].copy(), R)
    return RangePartitioner.uniform(R)      # pow2 R: key bits, else range


def _write_and_check(tmp_path, monkeypatch, kind, R, n, W, fused, conf_kw,
                     want_spill=False):
    import torch
    from sparkrdma_amd.conf import ShuffleConf
    from sparkrdma_amd.driver import Driver
    from sparkrdma_amd.manager import ShuffleManager
    from sparkrdma_amd.ops import radix

    routes = []
    real = radix.count_record_digits

    def spy(*a, **kw):
        d = real(*a, **kw)
        routes.append(d.hist is None)
        return d

    monkeypatch.setattr(radix, "count_record_digits", spy)
    conf = ShuffleConf(shm_dir=str(tmp_path), transport="ipc", **conf_kw)
    driver = Driver(conf)
    mgr = ShuffleManager(conf, executor_id=0, driver_port=driver.port)
    try:
        rng = np.random.default_rng(R)
        arr = _records(rng, n, W)
        prefix = arr[:, :8].copy().view("<u8").ravel()
        part = _partitioner(kind, R, prefix)
        assert part.gpu_params()[0] == {"bits": 0, "range": 2, "hash": 3,
                                        "bounds": 4}[kind]
        handle = mgr.register_shuffle(num_maps=1, num_partitions=R)
        w = mgr.get_writer(handle, 0)
        w.write_device_records(torch.from_numpy(arr.reshape(-1)).cuda(), W,
                               key_bytes=10)
        w.stop(True, partitioner=part)
        assert routes == [fused]
        if want_spill:
            assert mgr.pool.stats.allocs > 0, "expected host spill"
            assert mgr.gpu.pool.stats.allocs > 1, "expected several blocks"
        want_pids = part.partition_ids(prefix)
        seen = set()
        for ref, data in mgr.get_reader(handle, 0, R - 1):
            chunk = (data.cpu().numpy() if isinstance(data, torch.Tensor)
                     else np.frombuffer(bytes(data), dtype=np.uint8))
            chunk = chunk.reshape(-1, W)
            p = ref.partition
            assert p not in seen
            seen.add(p)
            assert np.array_equal(chunk, arr[want_pids == p]), \
                f"partition {p}: wrong records or order"
        assert seen == set(np.unique(want_pids).tolist())
    finally:
        mgr.stop()
        driver.stop()


@pytest.mark.parametrize("kind,R,fused", [
    ("bits", 256, True), ("range", 200, True), ("hash", 100, True),
    ("bounds", 37, True), ("range", 257, False), ("bits", 512, False)])
def test_writer_routes_match_oracle(tmp_path, monkeypatch, kind, R, fused):
    _write_and_check(tmp_path, monkeypatch, kind, R, 3 * TILE + 5, 100,
                     fused, dict(hbm_pool_size=1 << 30))


def test_writer_fused_route_under_pool_pressure(tmp_path, monkeypatch):
    """HBM (one 8 MB slab) holds at most half of the 16 MB output and a
    block 1 MB of it: the partitions span several HBM blocks and spilled
    groups (the setup of the spill tests in test_gpu_records.py)."""
    n, W, R = 40 * TILE + 5, 100, 200
    pool = 1 << ((n * W // 2).bit_length() - 1)
    assert 2 * pool <= n * W
    _write_and_check(tmp_path, monkeypatch, "range", R, n, W, True,
                     dict(hbm_pool_size=pool, hbm_slab_size=pool,
                          shuffle_write_block_size=1 << 20),
                     want_spill=True)


def test_partition_records_matches_oracle(hs):
    import torch
    from sparkrdma_amd.ops.radix import partition_records
    n, W, nbits = 5 * TILE + 17, 100, 3
    rng = np.random.default_rng(3)
    arr = _records(rng, n, W)
    counts, grouped = partition_records(
        torch.from_numpy(arr.reshape(-1)).cuda(), W, key_bytes=10,
        nbits=nbits)
    ids = (arr[:, :8].copy().view("<u8").ravel() >> np.uint64(64 - nbits)) \
        .astype(np.int64)
    assert np.array_equal(counts, np.bincount(ids, minlength=1 << nbits))
    order = np.argsort(ids, kind="stable")
    assert np.array_equal(grouped.cpu().numpy().reshape(n, W), arr[order])
