"""Sampled range partitioning: RangePartitioner.from_sample, sample_bounds
and the TeraSort hookup, on the CPU lanes."""

import multiprocessing as mp
import os
import socket

import numpy as np
import pytest

from sparkrdma_amd.partitioner import RangePartitioner


def _skewed(rng, n):
    """u^4 * 2^64: three quarters of the keys fall below 2^64 / 3."""
    return (rng.random(n) ** 4 * 2.0 ** 64).astype(np.uint64)


@pytest.mark.parametrize("R", [1, 2, 3, 64, 100])
def test_from_sample_shape(R):
    rng = np.random.default_rng(R)
    sample = rng.integers(0, 2 ** 64, 1000, dtype=np.uint64)
    p = RangePartitioner.from_sample(sample, R)
    assert p.num_partitions == R
    assert p.bounds.dtype == np.uint64
    assert len(p.bounds) == R - 1
    assert np.all(p.bounds[1:] >= p.bounds[:-1])
    srt = np.sort(sample)
    want = [srt[(i + 1) * len(srt) // R] for i in range(R - 1)]
    assert p.bounds.tolist() == [int(b) for b in want]


def test_from_sample_torch_matches_numpy():
    import torch
    rng = np.random.default_rng(3)
    sample = rng.integers(0, 2 ** 64, 777, dtype=np.uint64)
    a = RangePartitioner.from_sample(sample, 50)
    b = RangePartitioner.from_sample(
        torch.from_numpy(sample.view(np.int64)), 50)
    assert np.array_equal(a.bounds, b.bounds)


def test_from_sample_empty_raises():
    with pytest.raises(ValueError):
        RangePartitioner.from_sample(np.empty(0, dtype=np.uint64), 8)


def test_from_sample_duplicates():
    """A sample that is 90% one value: bounds repeat, R is kept, and
    partition_ids is still 'count the bounds <= key'."""
    rng = np.random.default_rng(1)
    hot = np.uint64(0x8000_0000_0000_1234)      # above 2^63: unsigned order
    sample = np.where(rng.random(5000) < 0.9, hot,
                      rng.integers(0, 2 ** 64, 5000, dtype=np.uint64))
    R = 32
    p = RangePartitioner.from_sample(sample, R)
    assert p.num_partitions == R and len(p.bounds) == R - 1
    assert np.all(p.bounds[1:] >= p.bounds[:-1])
    assert np.count_nonzero(p.bounds == hot) >= 2
    keys = np.concatenate([
        rng.integers(0, 2 ** 64, 900, dtype=np.uint64),
        np.full(90, hot), p.bounds[:8], p.bounds[:1] - np.uint64(1),
        np.array([0, 2 ** 64 - 1], dtype=np.uint64)])[:1000]
    assert len(keys) == 1000
    bl = [int(b) for b in p.bounds]
    want = [sum(1 for b in bl if b <= int(k)) for k in keys]
    got = p.partition_ids(keys)
    assert got.tolist() == want
    assert got.min() >= 0 and got.max() < R


def test_balance_skewed_keys():
    """Why the feature exists: on skewed keys the sampled bounds keep the
    largest partition within 1.5x the mean, the uniform partitioner puts
    more than 10x the mean into one partition."""
    n, R = 1 << 18, 64
    uni = RangePartitioner.uniform(R)
    worst = 0.0
    for seed in range(20):
        rng = np.random.default_rng(seed)
        keys = _skewed(rng, n)
        sample = rng.choice(keys, 16384, replace=False)
        p = RangePartitioner.from_sample(sample, R)
        c = np.bincount(p.partition_ids(keys), minlength=R)
        assert c.sum() == n
        worst = max(worst, c.max() / c.mean())
        cu = np.bincount(uni.partition_ids(keys), minlength=R)
        assert cu.max() > 10 * cu.mean(), (seed, cu.max() / cu.mean())
    print(f"worst sampled max/mean over 20 seeds: {worst:.3f}")
    assert worst <= 1.5


def test_gpu_params():
    rng = np.random.default_rng(0)
    p = RangePartitioner.from_sample(_skewed(rng, 4096), 100)
    assert p.gpu_params() == (4, 0, 100)
    assert RangePartitioner(np.array([5, 9], dtype=np.uint64)) \
        .gpu_params() == (4, 0, 3)
    # a non-pow2 key span has split points, not a closed form
    assert RangePartitioner.uniform(8, 0, 999).gpu_params() == (4, 0, 8)
    # unchanged: top bits (func 0) and full-range mulhi (func 2)
    assert RangePartitioner.uniform(256).gpu_params() == (0, 56, 0)
    assert RangePartitioner.uniform(100).gpu_params() == (2, 0, 100)
    assert RangePartitioner.uniform(4, key_max=2 ** 32 - 1) \
        .gpu_params() == (0, 30, 0)


def test_gpu_bounds_cached():
    p = RangePartitioner(np.array([1, 2 ** 63, 2 ** 64 - 1], dtype=np.uint64))
    t = p.gpu_bounds("cpu")
    assert t is p.gpu_bounds("cpu")
    assert t.numpy().view(np.uint64).tolist() == [1, 2 ** 63, 2 ** 64 - 1]


def test_terasort_cpu_sampled(tmp_path):
    from sparkrdma_amd.conf import ShuffleConf
    from sparkrdma_amd.engine import Engine
    from sparkrdma_amd.workloads.terasort import TeraSort
    conf = ShuffleConf(shm_dir=str(tmp_path),
                       max_buffer_allocation_size=1 << 30)
    eng = Engine(conf, rank=0, world_size=1, driver_port=0)
    try:
        n, R = 20000, 16
        ts = TeraSort(eng, records_per_executor=n,
                      partitions_per_executor=R, device="cpu",
                      validate=True, partitioner="sampled", key_skew=3)
        for _ in range(2):
            res = ts.run_step()
            assert res.records == n
            k, v = ts.last_outputs[0]
            assert len(k) == n
            assert np.array_equal(k, np.sort(ts.keys))
        assert ts.part.gpu_params() == (4, 0, R)
        # same bound as test_balance_skewed_keys (the sample is 16384 of
        # the 20000 keys); the uniform split of these keys is far worse
        c = np.bincount(ts.part.partition_ids(ts.keys), minlength=R)
        cu = np.bincount(RangePartitioner.uniform(R).partition_ids(ts.keys),
                         minlength=R)
        assert c.max() <= 1.5 * c.mean() < cu.max()
    finally:
        eng.shutdown()


def test_terasort_defaults_unchanged(tmp_path):
    from sparkrdma_amd.conf import ShuffleConf
    from sparkrdma_amd.engine import Engine
    from sparkrdma_amd.workloads.terasort import TeraSort
    conf = ShuffleConf(shm_dir=str(tmp_path),
                       max_buffer_allocation_size=1 << 30)
    eng = Engine(conf, rank=0, world_size=1, driver_port=0)
    try:
        ts = TeraSort(eng, records_per_executor=1000,
                      partitions_per_executor=64, device="cpu", seed=5)
        assert np.array_equal(ts.part.bounds,
                              RangePartitioner.uniform(64).bounds)
        assert ts.part.gpu_params() == (0, 58, 0)
        want = np.random.default_rng(5000).integers(0, 2 ** 64, 1000,
                                                    dtype=np.uint64)
        assert np.array_equal(ts.keys, want)
        with pytest.raises(ValueError):
            TeraSort(eng, 1000, 64, partitioner="nope")
        # a reduce chunk past the sort workspace (1.25x the records per
        # executor + 4096) is reported as a partitioning failure
        ts._check_chunk_fits(16 * (1250 + 4096), 0)
        with pytest.raises(RuntimeError, match="sampled"):
            ts._check_chunk_fits(16 * (1250 + 4097), 0)
    finally:
        eng.shutdown()


def _bounds_worker(rank, world, driver_port, shm_dir, q):
    try:
        import sys
        sys.path.insert(0, os.path.dirname(os.path.dirname(
            os.path.abspath(__file__))))
        from sparkrdma_amd.conf import ShuffleConf
        from sparkrdma_amd.engine import Engine
        from sparkrdma_amd.partitioner import sample_bounds

        conf = ShuffleConf(shm_dir=shm_dir,
                           max_buffer_allocation_size=1 << 30)
        eng = Engine(conf, rank=rank, world_size=world,
                     driver_port=driver_port)
        # every rank holds a DIFFERENT slice of the key space, so bounds
        # from a rank's own keys alone would disagree
        rng = np.random.default_rng(100 + rank)
        keys = (rng.random(30000) ** 4 * 2.0 ** 62).astype(np.uint64) \
            + np.uint64(rank) * np.uint64(2 ** 62)
        part = sample_bounds(eng, keys, 24, 2000, seed=9)
        # the sampling shuffle is gone: a second one gets the next id
        again = sample_bounds(eng, keys, 24, 2000, seed=9)
        assert np.array_equal(part.bounds, again.bounds)
        q.put((rank, part.bounds.tobytes(), keys.tobytes()))
        eng.barrier()
        eng.shutdown()
    except BaseException as e:  # surface failures to the parent
        import traceback
        q.put((rank, f"ERROR: {e}\n{traceback.format_exc()}", b""))
        raise


def test_multiprocess_sample_bounds_agree(tmp_path):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = [ctx.Process(target=_bounds_worker,
                         args=(r, world, port, str(tmp_path), q))
             for r in range(world)]
    for p in procs:
        p.start()
    got, keys = {}, {}
    for _ in range(world):
        rank, payload, kb = q.get(timeout=120)
        assert not isinstance(payload, str), f"rank {rank}: {payload}"
        got[rank] = np.frombuffer(payload, dtype=np.uint64)
        keys[rank] = np.frombuffer(kb, dtype=np.uint64)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert len(got[0]) == 23
    assert np.array_equal(got[0], got[1])
    assert np.all(got[0][1:] >= got[0][:-1])
    # the bounds come from BOTH ranks' keys: they balance the union
    allk = np.concatenate([keys[0], keys[1]])
    c = np.bincount(np.searchsorted(got[0], allk, side="right"),
                    minlength=24)
    assert c.max() <= 1.5 * c.mean()
