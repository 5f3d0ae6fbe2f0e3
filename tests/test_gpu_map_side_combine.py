"""Map-side combine on the GPU 16-byte lane: write_device_batch +
stop(combiner=...) sorts the map task's rows, collapses them with the
reduce_by_key kernel and ships one row per distinct key; read_aos merges."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture
def engine(tmp_path):
    from sparkrdma_amd.conf import ShuffleConf
    from sparkrdma_amd.engine import Engine
    conf = ShuffleConf(shm_dir=str(tmp_path), transport="ipc",
                       hbm_pool_size=2 << 30)
    eng = Engine(conf, rank=0, world_size=1, driver_port=0)
    yield eng
    eng.shutdown()


@pytest.fixture
def manager(tmp_path):
    from sparkrdma_amd.conf import ShuffleConf
    from sparkrdma_amd.driver import Driver
    from sparkrdma_amd.manager import ShuffleManager
    conf = ShuffleConf(shm_dir=str(tmp_path), transport="ipc",
                       hbm_pool_size=1 << 30,
                       shuffle_write_block_size=1 << 20)
    driver = Driver(conf)
    mgr = ShuffleManager(conf, executor_id=0, driver_port=driver.port)
    yield mgr
    mgr.stop()
    driver.stop()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


@pytest.mark.parametrize("agg", ["sum", "count", "min", "max"])
def test_workload_ships_one_row_per_key(engine, agg):
    from sparkrdma_amd.workloads.reduce_by_key import ReduceByKey
    rows, nk = 200_000, 3000
    res = {}
    for combine in (True, False):
        wl = ReduceByKey(engine, rows_per_executor=rows, num_keys=nk,
                         partitions_per_executor=32, device="cuda",
                         validate=True, aggregator=agg,
                         map_side_combine=combine)
        res[combine] = wl.run_step()
    assert res[True].groups == nk and res[False].groups == nk
    assert res[True].shuffle_bytes == 16 * nk
    assert res[False].shuffle_bytes == 16 * rows


def test_two_maps_count_is_merged(manager):
    from sparkrdma_amd.partitioner import HashPartitioner
    R, n = 16, 50_000
    part = HashPartitioner(R)
    handle = manager.register_shuffle(num_maps=2, num_partitions=R)
    rng = np.random.default_rng(41)
    ks = [rng.integers(0, 700, n, dtype=np.uint64) for _ in range(2)]
    for mid, k in enumerate(ks):
        w = manager.get_writer(handle, mid)
        w.write_device_batch(_dev(k), _dev(k))
        w.stop(True, partitioner=part, combiner="count")
        distinct = len(np.unique(k))
        assert w.metrics.records_written == distinct
        assert w.metrics.bytes_written == 16 * distinct
        assert w.metrics.extra["records_combined_in"] == n
    uk, cnt = manager.get_reader(handle, 0, R - 1).read_aos(
        aggregator="count", map_side_combined=True)
    torch.cuda.synchronize()
    want = np.bincount(np.concatenate(ks).astype(np.int64), minlength=700)
    assert np.array_equal(uk.cpu().numpy(), np.nonzero(want)[0])
    assert np.array_equal(cnt.cpu().numpy(), want[want > 0])
    # read as raw rows the same shuffle holds one row per map per key
    uk2, rows = manager.get_reader(handle, 0, R - 1).read_aos(
        aggregator="count")
    torch.cuda.synchronize()
    assert torch.equal(uk2, uk)
    assert np.all(rows.cpu().numpy() == 2)


def test_more_than_4096_partitions(manager):
    from sparkrdma_amd.partitioner import HashPartitioner
    R, n = 8192, 50_000
    part = HashPartitioner(R)
    handle = manager.register_shuffle(num_maps=1, num_partitions=R)
    rng = np.random.default_rng(43)
    k = rng.integers(0, 9000, n, dtype=np.uint64)
    v = rng.integers(0, 1 << 62, n, dtype=np.uint64)
    w = manager.get_writer(handle, 0)
    w.write_device_batch(_dev(k), _dev(v))
    w.stop(True, partitioner=part, combiner="sum")
    distinct = len(np.unique(k))
    assert w.metrics.records_written == distinct
    assert w.metrics.bytes_written == 16 * distinct
    uk, sums = manager.get_reader(handle, 0, R - 1).read_aos(
        aggregator="sum", map_side_combined=True)
    torch.cuda.synchronize()
    want = {}
    for kk, vv in zip(k.tolist(), v.tolist()):
        want[kk] = (want.get(kk, 0) + vv) & (2 ** 64 - 1)
    got = dict(zip(uk.cpu().numpy().view(np.uint64).tolist(),
                   sums.cpu().numpy().view(np.uint64).tolist()))
    assert got == want


def test_combiner_refuses_wide_records(manager):
    from sparkrdma_amd.partitioner import HashPartitioner
    R = 16
    handle = manager.register_shuffle(num_maps=1, num_partitions=R)
    recs = torch.zeros(100 * 24, dtype=torch.uint8, device="cuda")
    w = manager.get_writer(handle, 0)
    w.write_device_records(recs, 24)
    with pytest.raises(ValueError):
        w.stop(True, partitioner=HashPartitioner(R), combiner="sum")
