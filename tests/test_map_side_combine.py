"""Map-side combine on the CPU lane: ``stop(combiner=...)`` collapses each
map task's rows to one per key, ``read_aos(..., map_side_combined=True)``
merges the partial results (the reference's combineCombinersByKey branch,
RdmaShuffleReader.scala:83-96). The combined path must give what the plain
path gives on the same data while shipping one row per distinct key."""

import numpy as np
import pytest

from sparkrdma_amd.conf import ShuffleConf
from sparkrdma_amd.driver import Driver
from sparkrdma_amd.manager import ShuffleManager
from sparkrdma_amd.partitioner import HashPartitioner
from sparkrdma_amd.reader import ShuffleReader

R = 4
AGGS = ShuffleReader.AGGREGATORS


@pytest.fixture
def cluster(tmp_path):
    conf = ShuffleConf(shm_dir=str(tmp_path), transport="shm",
                       max_buffer_allocation_size=1 << 30)
    driver = Driver(conf)
    conf.driver_port = driver.port
    managers = [ShuffleManager(conf, executor_id=i, driver_port=driver.port)
                for i in range(2)]
    yield managers
    for m in managers:
        m.stop()
    driver.stop()


def _data(agg, seed=0):
    """2 maps x 1000 rows, keys in [0, 50): every key is on both maps."""
    rng = np.random.default_rng(seed)
    ks = [rng.integers(0, 50, 1000, dtype=np.uint64) for _ in range(2)]
    if agg == "sum_f64":
        vs = [rng.random(1000).view(np.uint64) for _ in range(2)]
    else:
        vs = [rng.integers(0, 1000, 1000, dtype=np.uint64) for _ in range(2)]
    return ks, vs


def _write(managers, ks, vs, combiner=None, **kw):
    part = HashPartitioner(R)
    handle = managers[0].register_shuffle(len(managers), R)
    writers = []
    for mid, (mgr, k, v) in enumerate(zip(managers, ks, vs)):
        w = mgr.get_writer(handle, mid)
        w.write_batch(k, v.view(np.uint8).reshape(-1, 8).copy())
        w.stop(True, partitioner=part, combiner=combiner, **kw)
        writers.append(w)
    return handle, writers


def _read(managers, handle, agg, combined):
    uk, out = managers[0].get_reader(handle, 0, R - 1).read_aos(
        aggregator=agg, map_side_combined=combined)
    return np.asarray(uk), np.asarray(out)


@pytest.mark.parametrize("agg", AGGS)
def test_combined_equals_plain(cluster, agg):
    ks, vs = _data(agg)
    plain_h, _ = _write(cluster, ks, vs)
    comb_h, _ = _write(cluster, ks, vs, combiner=agg)
    pk, pv = _read(cluster, plain_h, agg, False)
    ck, cv = _read(cluster, comb_h, agg, True)
    assert np.array_equal(pk, ck)
    assert len(ck) == 50
    if agg == "sum_f64":
        assert np.max(np.abs(pv - cv)) < 1e-9
    else:
        assert np.array_equal(pv.astype(np.uint64), cv.astype(np.uint64))


def test_count_merges_not_recounts(cluster):
    ks, vs = _data("count", seed=1)
    handle, _ = _write(cluster, ks, vs, combiner="count")
    uk, cnt = _read(cluster, handle, "count", True)
    want = np.bincount(np.concatenate(ks).astype(np.int64), minlength=50)
    assert np.array_equal(uk.astype(np.int64), np.nonzero(want)[0])
    assert np.array_equal(cnt.astype(np.int64), want[want > 0])
    assert int(cnt.sum()) == 2000
    # without the merge flag the reader counts ROWS: one per map per key
    uk2, cnt2 = _read(cluster, handle, "count", False)
    maps_with = sum((np.bincount(k.astype(np.int64), minlength=50) > 0)
                    .astype(np.int64) for k in ks)
    assert np.array_equal(uk2, uk)
    assert np.array_equal(cnt2.astype(np.int64), maps_with[maps_with > 0])


def test_writer_metrics_are_post_combine(cluster):
    ks, vs = _data("sum", seed=2)
    _, writers = _write(cluster, ks, vs, combiner="sum")
    for w, k in zip(writers, ks):
        distinct = len(np.unique(k))
        assert w.metrics.records_written == distinct
        assert w.metrics.bytes_written == 16 * distinct
        assert w.metrics.extra["records_combined_in"] == 1000
    _, plain = _write(cluster, ks, vs)
    for w in plain:
        assert w.metrics.records_written == 1000
        assert w.metrics.bytes_written == 16 * 1000
        assert "records_combined_in" not in w.metrics.extra


def test_partial_combine_with_few_key_bits(cluster):
    """Keys differ above bit 8: sorting by 8 bits interleaves them, runs
    fragment, more rows ship — and the merged result is still exact."""
    rng = np.random.default_rng(3)
    ks = [rng.integers(0, 50, 1000, dtype=np.uint64)
          | (rng.integers(0, 4, 1000, dtype=np.uint64) << np.uint64(40))
          for _ in range(2)]
    vs = [rng.integers(0, 1000, 1000, dtype=np.uint64) for _ in range(2)]
    handle, writers = _write(cluster, ks, vs, combiner="sum",
                             combine_key_bits=8)
    uk, sums = _read(cluster, handle, "sum", True)
    want = {}
    for k, v in zip(np.concatenate(ks).tolist(), np.concatenate(vs).tolist()):
        want[k] = want.get(k, 0) + v
    assert dict(zip(uk.tolist(), sums.tolist())) == want
    for w, k in zip(writers, ks):
        assert len(np.unique(k)) <= w.metrics.records_written <= 1000
        assert w.metrics.extra["records_combined_in"] == 1000


def test_combiner_value_errors(cluster):
    part = HashPartitioner(R)
    handle = cluster[0].register_shuffle(2, R)
    k = np.arange(10, dtype=np.uint64)
    v8 = np.zeros((10, 8), dtype=np.uint8)

    w = cluster[0].get_writer(handle, 0)
    w.write_batch(k, v8)
    with pytest.raises(ValueError):
        w.stop(True, partitioner=part, combiner="median")

    w = cluster[0].get_writer(handle, 0)
    w.write_batch(k)                                    # value-less
    with pytest.raises(ValueError):
        w.stop(True, partitioner=part, combiner="sum")

    w = cluster[0].get_writer(handle, 0)
    w.write_batch(k, np.zeros((10, 4), dtype=np.uint8))  # 4-byte values
    with pytest.raises(ValueError):
        w.stop(True, partitioner=part, combiner="sum")

    w = cluster[0].get_writer(handle, 0)
    w.write_records([("a", 1), ("b", 2)])               # pickled lane
    with pytest.raises(ValueError):
        w.stop(True, combiner="sum")

    class _FakeRecords:                                 # wide-record lane:
        def numel(self):                                # stop() must refuse
            return 32                                   # before touching it
    w = cluster[0].get_writer(handle, 0)
    w.write_device_records(_FakeRecords(), 16)
    with pytest.raises(ValueError):
        w.stop(True, partitioner=part, combiner="sum")


def test_map_side_combined_needs_aggregator(cluster):
    handle = cluster[0].register_shuffle(2, R)
    with pytest.raises(ValueError):
        cluster[0].get_reader(handle, 0, R - 1).read_aos(
            map_side_combined=True)


@pytest.mark.parametrize("agg", ["sum", "count"])
def test_reduce_by_key_workload_cpu(tmp_path, agg):
    from sparkrdma_amd.engine import Engine
    from sparkrdma_amd.workloads.reduce_by_key import ReduceByKey
    conf = ShuffleConf(shm_dir=str(tmp_path), transport="shm",
                       max_buffer_allocation_size=1 << 30)
    eng = Engine(conf, rank=0, world_size=1, driver_port=0)
    try:
        rows = 20_000
        res = {}
        for combine in (True, False):
            wl = ReduceByKey(eng, rows_per_executor=rows, num_keys=300,
                             partitions_per_executor=8, device="cpu",
                             validate=True, aggregator=agg,
                             map_side_combine=combine)
            res[combine] = wl.run_step()
        assert res[True].groups == res[False].groups == 300
        assert res[True].shuffle_bytes == 16 * res[True].groups
        assert res[False].shuffle_bytes == 16 * rows
    finally:
        eng.shutdown()
