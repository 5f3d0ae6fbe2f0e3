"""Range partitioning by arbitrary split points on the GPU write path:
extract_pairs_bounds (ops/csrc/bounds.hip) against numpy.searchsorted, the
writer end to end against the CPU partitioner, and the sampled TeraSort."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U64_MAX = np.uint64(2 ** 64 - 1)
IDX_BASE = (1 << 40) + 12345


@pytest.fixture(scope="module")
def hs():
    from sparkrdma_amd.ops import load
    m = load()
    m.set_device(0)
    return m


def _bound_sets(rng, m):
    """m ascending u64 split points, four ways."""
    rnd = np.sort(rng.integers(0, 2 ** 64, m, dtype=np.uint64))
    run = rnd.copy()
    a = (m - min(m, 10)) // 2
    run[a:a + 10] = run[a]              # a run of 10 equal bounds
    first0 = rnd.copy()
    first0[0] = 0
    last_max = rnd.copy()
    last_max[-1] = U64_MAX
    return {"random": rnd, "run10": np.sort(run), "first0": first0,
            "lastmax": last_max}


def _special_keys(bounds):
    """Every bound, bound +- 1 without wrap, 0 and 2^64 - 1."""
    below = bounds[bounds > 0] - np.uint64(1)
    above = bounds[bounds < U64_MAX] + np.uint64(1)
    return np.concatenate([bounds, below, above,
                           np.array([0, U64_MAX], dtype=np.uint64)])


def _keys(rng, n, special):
    """n keys: random u64 (half of them >= 2^63), every other slot (the
    first included) overwritten by a randomly chosen special key."""
    k = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    slots = np.arange(0, n, 2)
    k[slots] = rng.choice(special, len(slots))
    return k


def _run_kernel(hs, rng, keys, W, key_bytes, bounds_dev, m):
    import torch
    n = len(keys)
    arr = rng.integers(0, 256, (n, W), dtype=np.uint8)
    arr[:, :8] = keys.astype("<u8").view(np.uint8).reshape(n, 8)
    recs = torch.from_numpy(arr.reshape(-1)).cuda()
    # guard words behind the pairs: the kernel writes exactly n pairs
    pairs = torch.full((2 * n + 4,), -7, dtype=torch.int64, device="cuda")
    hs.extract_pairs_bounds(recs.data_ptr(), n, W, key_bytes,
                            pairs.data_ptr(), bounds_dev.data_ptr(), m,
                            torch.cuda.current_stream().cuda_stream,
                            IDX_BASE)
    out = pairs.cpu().numpy()
    assert np.all(out[2 * n:] == -7)
    aux = IDX_BASE + np.arange(n, dtype=np.uint64)
    if key_bytes == 10:
        aux |= arr[:, 8:10].copy().view("<u2").ravel().astype(np.uint64) \
            << np.uint64(48)
    return out[0:2 * n:2].view(np.uint64), out[1:2 * n:2].view(np.uint64), aux


@pytest.mark.parametrize("W,key_bytes", [(8, 8), (16, 8), (100, 10)])
@pytest.mark.parametrize("R", [2, 3, 64, 100, 4096, 4097, 5000, 70000])
def test_kernel_matches_searchsorted(hs, R, W, key_bytes):
    """pair.x == searchsorted(bounds, key, 'right') and pair.y == aux,
    exactly. R = 2 is one bound, 4096 the full LDS table, 4097 the first
    coarse + fine table (s = 1), 70000 has s = 5."""
    import torch
    rng = np.random.default_rng(R * 1000 + W)
    m = R - 1
    for name, bounds in _bound_sets(rng, m).items():
        bdev = torch.from_numpy(bounds.view(np.int64)).cuda()
        special = _special_keys(bounds)
        # the four sizes, then EVERY special key in one launch
        cases = [_keys(rng, n, special) for n in (1, 255, 257, 20000)]
        cases.append(special)
        for keys in cases:
            x, y, aux = _run_kernel(hs, rng, keys, W, key_bytes, bdev, m)
            want = np.searchsorted(bounds, keys, side="right")
            bad = np.nonzero(x != want.astype(np.uint64))[0]
            assert len(bad) == 0, (
                name, len(keys), int(keys[bad[0]]), int(x[bad[0]]),
                int(want[bad[0]]))
            assert np.array_equal(y, aux), (name, len(keys))


def test_kernel_argument_checks(hs):
    import torch
    buf = torch.zeros(64, dtype=torch.int64, device="cuda")
    p = buf.data_ptr()
    with pytest.raises(RuntimeError):
        hs.extract_pairs_bounds(p, 1, 10, 8, p, p, 1)      # rec_bytes % 4
    with pytest.raises(RuntimeError):
        hs.extract_pairs_bounds(p, 1, 16, 9, p, p, 1)      # key_bytes
    with pytest.raises(RuntimeError):
        hs.extract_pairs_bounds(p, 1, 16, 8, p, p, 1, 0, 1 << 48)
    with pytest.raises(RuntimeError):
        hs.extract_pairs_bounds(p, 1, 16, 8, p, p, 1 << 24)


@pytest.mark.parametrize("s", [1, 1000, 100_000])
def test_from_sample_device_matches_numpy(hs, s):
    """A device sample is sorted on the device (unsigned order)."""
    import torch
    from sparkrdma_amd.partitioner import RangePartitioner
    sample = np.random.default_rng(s).integers(0, 2 ** 64, s, dtype=np.uint64)
    dev = torch.from_numpy(sample.view(np.int64)).cuda()
    a = RangePartitioner.from_sample(dev, 64)
    b = RangePartitioner.from_sample(sample, 64)
    assert np.array_equal(a.bounds, b.bounds)
    assert np.array_equal(dev.cpu().numpy().view(np.uint64), sample)


# ---------------------------------------------------------------------------
# writer end to end


@pytest.fixture
def manager(tmp_path):
    from sparkrdma_amd.conf import ShuffleConf
    from sparkrdma_amd.driver import Driver
    from sparkrdma_amd.manager import ShuffleManager
    conf = ShuffleConf(shm_dir=str(tmp_path), transport="ipc",
                       hbm_pool_size=1 << 30)
    driver = Driver(conf)
    mgr = ShuffleManager(conf, executor_id=0, driver_port=driver.port)
    yield mgr
    mgr.stop()
    driver.stop()


N_E2E = 50000


def _skewed(rng, n):
    return (rng.random(n) ** 4 * 2.0 ** 64).astype(np.uint64)


def _part_and_keys(R, distinct=None):
    """Skewed keys and custom bounds from a skewed sample of them."""
    from sparkrdma_amd.partitioner import RangePartitioner
    rng = np.random.default_rng(R)
    keys = _skewed(rng, N_E2E)
    if distinct:
        keys = keys[rng.integers(0, distinct, N_E2E)]
    part = RangePartitioner.from_sample(rng.choice(keys, 8192), R)
    assert part.gpu_params() == (4, 0, R)
    return rng, part, keys


def _read_rows(mgr, handle, R, W):
    """partition -> rows (n_p x W bytes), one device-to-host copy."""
    import torch
    parts = mgr.get_reader(handle, 0, R - 1).collect_partitions()
    order, views = [], []
    for p, chunks in parts.items():
        for c in chunks:
            assert isinstance(c, torch.Tensor)
            order.append((p, c.numel()))
            views.append(c.reshape(-1).view(torch.uint8))
    flat = (torch.cat(views).cpu().numpy() if views
            else np.empty(0, dtype=np.uint8))
    rows = {p: [] for p in range(R)}
    off = 0
    for p, nb in order:
        assert nb % W == 0
        rows[p].append(flat[off:off + nb].reshape(-1, W))
        off += nb
    return {p: (np.concatenate(r) if r else np.empty((0, W), np.uint8))
            for p, r in rows.items()}


def _sorted_rows(a):
    """Rows in a canonical order (lexicographic over the bytes)."""
    if len(a) == 0:
        return a
    return a[np.lexsort(a.T[::-1])]


def _check_split(got, part, arr, R):
    """Every partition holds exactly the rows the CPU partitioner sends
    there; order inside a partition is not specified."""
    prefix = arr[:, :8].copy().view("<u8").ravel()
    pids = part.partition_ids(prefix)
    counts = np.bincount(pids, minlength=R)
    assert [len(got[p]) for p in range(R)] == counts.tolist()
    order = np.argsort(pids, kind="stable")
    srt = arr[order]
    ends = np.cumsum(counts)
    for p in range(R):
        want = srt[ends[p] - counts[p]:ends[p]]
        assert np.array_equal(_sorted_rows(got[p]), _sorted_rows(want)), p


@pytest.mark.parametrize("shape", ["kv16", "keys8", "wide100"])
@pytest.mark.parametrize("R", [100, 5000])
def test_writer_custom_bounds(manager, R, shape):
    """Fails without the feature: custom bounds had no GPU dispatch."""
    import torch
    rng, part, keys = _part_and_keys(R)
    handle = manager.register_shuffle(num_maps=1, num_partitions=R)
    w = manager.get_writer(handle, 0)
    kd = torch.from_numpy(keys.view(np.int64)).cuda()
    if shape == "wide100":
        W = 100
        arr = rng.integers(0, 256, (N_E2E, W), dtype=np.uint8)
        arr[:, :8] = keys.view(np.uint8).reshape(-1, 8)
        w.write_device_records(torch.from_numpy(arr.reshape(-1)).cuda(),
                               W, key_bytes=10)
    elif shape == "kv16":
        W = 16
        vals = rng.integers(0, 2 ** 64, N_E2E, dtype=np.uint64)
        arr = np.stack([keys, vals], axis=1).view(np.uint8).reshape(-1, 16)
        w.write_device_batch(kd, torch.from_numpy(vals.view(np.int64)).cuda())
    else:
        W = 8
        arr = keys.view(np.uint8).reshape(-1, 8)
        w.write_device_batch(kd)
    w.stop(True, partitioner=part)
    assert w.metrics.records_written == N_E2E
    assert w.metrics.bytes_written == N_E2E * W
    _check_split(_read_rows(manager, handle, R, W), part, arr, R)


def test_writer_custom_bounds_combiner_sum(manager):
    """Map-side combine runs before the routing: one row per distinct key,
    each in the partition its bounds assign."""
    import torch
    R = 100
    rng, part, keys = _part_and_keys(R, distinct=3000)
    vals = rng.integers(0, 1 << 62, N_E2E, dtype=np.uint64)
    handle = manager.register_shuffle(num_maps=1, num_partitions=R)
    w = manager.get_writer(handle, 0)
    w.write_device_batch(torch.from_numpy(keys.view(np.int64)).cuda(),
                         torch.from_numpy(vals.view(np.int64)).cuda())
    w.stop(True, partitioner=part, combiner="sum")
    uk, inv = np.unique(keys, return_inverse=True)
    sums = np.zeros(len(uk), dtype=np.uint64)
    np.add.at(sums, inv, vals)          # wraps like the kernel's i64 sum
    assert w.metrics.records_written == len(uk)
    arr = np.stack([uk, sums], axis=1).view(np.uint8).reshape(-1, 16)
    _check_split(_read_rows(manager, handle, R, 16), part, arr, R)


def test_writer_rejects_bounds_of_another_R(manager):
    import torch
    _rng, part, keys = _part_and_keys(100)
    handle = manager.register_shuffle(num_maps=1, num_partitions=64)
    w = manager.get_writer(handle, 0)
    w.write_device_batch(torch.from_numpy(keys.view(np.int64)).cuda())
    with pytest.raises(ValueError):
        w.stop(True, partitioner=part)


# ---------------------------------------------------------------------------
# TeraSort


@pytest.fixture
def engine(tmp_path):
    from sparkrdma_amd.conf import ShuffleConf
    from sparkrdma_amd.engine import Engine
    conf = ShuffleConf(shm_dir=str(tmp_path), transport="ipc",
                       hbm_pool_size=1 << 30)
    eng = Engine(conf, rank=0, world_size=1, driver_port=0)
    yield eng
    eng.shutdown()


@pytest.mark.parametrize("record_bytes", [16, 100])
def test_terasort_sampled_skewed(engine, record_bytes):
    from sparkrdma_amd.partitioner import RangePartitioner
    from sparkrdma_amd.workloads.terasort import TeraSort
    n, R = 200_000, 64
    ts = TeraSort(engine, records_per_executor=n,
                  partitions_per_executor=R, device="cuda", validate=True,
                  record_bytes=record_bytes, partitioner="sampled",
                  key_skew=3)
    for _ in range(2):
        res = ts.run_step()
        assert res.records == n
        assert sum((o.numel() // record_bytes) if record_bytes != 16
                   else o[0].numel() for o in ts.last_outputs) == n
    assert ts.part.gpu_params() == (4, 0, R)
    assert engine.manager.gpu.pool.stats.used_bytes == 0   # all freed
    # the keys really are skewed, and the sampled bounds really balance
    if record_bytes == 16:
        k = ts.keys.cpu().numpy().view(np.uint64)
    else:
        k = ts.recs.cpu().numpy().reshape(n, record_bytes)[:, :8] \
            .copy().view("<u8").ravel()
    cu = np.bincount(RangePartitioner.uniform(R).partition_ids(k),
                     minlength=R)
    c = np.bincount(ts.part.partition_ids(k), minlength=R)
    assert cu.max() > 10 * cu.mean()
    assert c.max() <= 1.5 * c.mean()


def test_terasort_default_is_uniform_top_bits(engine):
    from sparkrdma_amd.partitioner import RangePartitioner
    from sparkrdma_amd.workloads.terasort import TeraSort
    ts = TeraSort(engine, records_per_executor=1000,
                  partitions_per_executor=64, device="cuda")
    assert np.array_equal(ts.part.bounds, RangePartitioner.uniform(64).bounds)
    assert ts.part.gpu_params() == (0, 58, 0)
    assert ts.partitioner == "uniform"
