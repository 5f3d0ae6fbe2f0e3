"""Variable-length rows on the GPU shuffle path: write_device_varlen ->
stop() -> read_varlen, against the numpy mirror of sparkrdma_amd/varlen.py."""

from collections import Counter

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

R = 16


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


@pytest.fixture
def engine(tmp_path):
    from sparkrdma_amd.conf import ShuffleConf
    from sparkrdma_amd.engine import Engine
    conf = ShuffleConf(shm_dir=str(tmp_path), transport="ipc",
                       hbm_pool_size=1 << 30)
    eng = Engine(conf, rank=0, world_size=1, driver_port=0)
    yield eng
    eng.shutdown()


def make_rows(rng, n, num_keys, max_len=64, long_rows=0):
    lens = rng.integers(0, max_len + 1, n)
    if long_rows:
        lens[rng.choice(n, long_rows, replace=False)] = 10_000
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    keys = rng.integers(0, num_keys, n, dtype=np.uint64)
    data = rng.integers(0, 256, int(offsets[-1]), dtype=np.uint8)
    return keys, offsets, data


def to_dev(keys, offsets, data):
    return (torch.from_numpy(np.ascontiguousarray(keys).view(np.int64)).cuda(),
            torch.from_numpy(np.ascontiguousarray(offsets)).cuda(),
            torch.from_numpy(np.ascontiguousarray(data)).cuda())


def to_host(keys, offsets, data):
    torch.cuda.synchronize()
    assert keys.is_cuda and offsets.is_cuda and data.is_cuda
    assert keys.dtype == torch.int64 and offsets.dtype == torch.int64
    assert data.dtype == torch.uint8
    k = keys.cpu().numpy().view(np.uint64)
    o, d = offsets.cpu().numpy(), data.cpu().numpy()
    assert len(o) == len(k) + 1 and o[0] == 0 and o[-1] == len(d)
    assert np.all(np.diff(o) >= 0)
    return k, o, d


def rows_of(keys, offsets, data):
    buf = np.asarray(data).tobytes()
    return Counter((int(keys[r]), buf[offsets[r]:offsets[r + 1]])
                   for r in range(len(keys)))


def write(manager, handle, map_id, rows, part, batches=1):
    k, o, d = rows
    w = manager.get_writer(handle, map_id)
    cuts = np.linspace(0, len(k), batches + 1).astype(int)
    for a, b in zip(cuts[:-1], cuts[1:]):
        w.write_device_varlen(*to_dev(k[a:b], o[a:b + 1] - o[a],
                                      d[o[a]:o[b]]))
    w.stop(True, partitioner=part)
    return w


def published_segments(manager, handle, lo, hi):
    """(partition, bytes) of every non-empty block, copied back."""
    out = []
    for ref, blk in manager.get_reader(handle, lo, hi):
        if len(blk):
            out.append((ref.partition, blk.cpu().numpy().tobytes()))
    return out


def test_two_maps_round_trip(manager):
    from sparkrdma_amd.partitioner import HashPartitioner
    from sparkrdma_amd.varlen import (partition_varlen_np,
                                      unpack_varlen_segment)
    rng = np.random.default_rng(5)
    part = HashPartitioner(R)
    handle = manager.register_shuffle(num_maps=2, num_partitions=R)
    inputs = [make_rows(rng, 20_000, 700, long_rows=4) for _ in range(2)]
    want = Counter()
    for mid, rows in enumerate(inputs):
        w = write(manager, handle, mid, rows, part, batches=mid + 1)
        want += rows_of(*rows)
        k, o, d = rows
        mirror = partition_varlen_np(k, o, d, part.partition_ids(k), R)
        assert w.metrics.records_written == 20_000
        assert w.metrics.bytes_written == sum(len(s) for s in mirror)

    # what was published is the wire format, partition by partition
    segs = published_segments(manager, handle, 0, R - 1)
    assert len(segs) == 2 * R
    total = 0
    for p, seg in segs:
        assert len(seg) % 16 == 0
        k, o, d = unpack_varlen_segment(seg)
        assert np.all(part.partition_ids(k) == p)
        total += len(k)
    assert total == 40_000

    got = to_host(*manager.get_reader(handle, 0, R - 1).read_varlen())
    assert rows_of(*got) == want

    k, o, d = to_host(*manager.get_reader(handle, 0, R - 1)
                      .read_varlen(ordering=True))
    assert np.all(k[1:] >= k[:-1])
    assert rows_of(k, o, d) == want

    seen = Counter()
    for p in range(R):
        k, o, d = to_host(*manager.get_reader(handle, p, p).read_varlen())
        assert np.all(part.partition_ids(k) == p)
        seen += rows_of(k, o, d)
    assert seen == want


def test_segments_equal_the_numpy_mirror(manager):
    """The scatter keeps input order inside a partition, so a map task's
    published bytes are exactly partition_varlen_np's."""
    from sparkrdma_amd.partitioner import HashPartitioner
    from sparkrdma_amd.varlen import partition_varlen_np
    rng = np.random.default_rng(6)
    part = HashPartitioner(R)
    handle = manager.register_shuffle(num_maps=1, num_partitions=R)
    k, o, d = make_rows(rng, 3000, 1 << 40, max_len=33, long_rows=1)
    write(manager, handle, 0, (k, o, d), part)
    mirror = partition_varlen_np(k, o, d, part.partition_ids(k), R)
    got = dict(published_segments(manager, handle, 0, R - 1))
    for p in range(R):
        assert got.get(p, b"") == mirror[p], f"partition {p}"


def test_one_key_empty_map_and_empty_rows(manager):
    from sparkrdma_amd.partitioner import HashPartitioner
    part = HashPartitioner(R)
    handle = manager.register_shuffle(num_maps=3, num_partitions=R)
    rng = np.random.default_rng(8)
    # map 0: one key only, so 15 of the 16 partitions are empty
    k, o, d = make_rows(rng, 500, 1)
    k[:] = 123456789
    write(manager, handle, 0, (k, o, d), part)
    # map 1: no rows
    w = write(manager, handle, 1, (np.empty(0, np.uint64),
                                   np.zeros(1, np.int64),
                                   np.empty(0, np.uint8)), part)
    assert w.metrics.records_written == 0 and w.metrics.bytes_written == 0
    # map 2: rows, but every one of length zero
    k2 = rng.integers(0, 5, 300, dtype=np.uint64)    # <= 5 partitions
    w = write(manager, handle, 2, (k2, np.zeros(301, np.int64),
                                   np.empty(0, np.uint8)), part)
    assert w.metrics.records_written == 300
    home = int(part.partition_ids(k[:1])[0])
    got = to_host(*manager.get_reader(handle, home, home).read_varlen())
    pid2 = part.partition_ids(k2)
    want = rows_of(k, o, d) + Counter((int(x), b"") for x in k2[pid2 == home])
    assert rows_of(*got) == want
    empty = next(p for p in range(R) if p != home and not np.any(pid2 == p))
    for ordering in (False, True):
        k3, o3, d3 = manager.get_reader(handle, empty, empty).read_varlen(
            ordering=ordering)
        assert k3.is_cuda and k3.numel() == 0 and d3.numel() == 0
        assert o3.cpu().tolist() == [0]
    allrows = to_host(*manager.get_reader(handle, 0, R - 1)
                      .read_varlen(ordering=True))
    assert rows_of(*allrows) == rows_of(k, o, d) + Counter(
        (int(x), b"") for x in k2)


def test_non_pow2_range_partitioner(manager):
    from sparkrdma_amd.partitioner import RangePartitioner
    Rn = 12
    part = RangePartitioner.uniform(Rn)
    assert part.gpu_params() is not None and part.gpu_params()[0] != 4
    handle = manager.register_shuffle(num_maps=1, num_partitions=Rn)
    rng = np.random.default_rng(9)
    k, o, d = make_rows(rng, 5000, 1 << 63, max_len=40)
    k = rng.integers(0, 2 ** 64, 5000, dtype=np.uint64)
    write(manager, handle, 0, (k, o, d), part)
    seen = Counter()
    for p in range(Rn):
        kk, oo, dd = to_host(*manager.get_reader(handle, p, p).read_varlen())
        assert np.all(part.partition_ids(kk) == p)
        seen += rows_of(kk, oo, dd)
    assert seen == rows_of(k, o, d)


def test_limits_raise(manager):
    from sparkrdma_amd.partitioner import HashPartitioner, RangePartitioner
    rows = to_dev(np.array([1, 2], np.uint64), np.array([0, 2, 3], np.int64),
                  np.zeros(3, np.uint8))
    handle = manager.register_shuffle(num_maps=1, num_partitions=8192)
    w = manager.get_writer(handle, 0)
    w.write_device_varlen(*rows)
    with pytest.raises(ValueError, match="R <= 4096"):
        w.stop(True, partitioner=HashPartitioner(8192))
    handle = manager.register_shuffle(num_maps=1, num_partitions=4)
    w = manager.get_writer(handle, 0)
    w.write_device_varlen(*rows)
    split = RangePartitioner(np.array([10, 20, 30], dtype=np.uint64))
    with pytest.raises(ValueError, match="split-point"):
        w.stop(True, partitioner=split)
    with pytest.raises(ValueError, match="variable-length"):
        w.stop(True, partitioner=HashPartitioner(4), combiner="sum")
    with pytest.raises(ValueError, match="mixed"):
        w.write_device_batch(rows[0], rows[0])
    with pytest.raises(ValueError, match="mixed"):
        w.write_varlen(np.array([1], np.uint64), np.array([0, 1], np.int64),
                       np.zeros(1, np.uint8))
    # none of the refusals changed the writer: it still commits
    w.stop(True, partitioner=HashPartitioner(4))
    k, _o, d = to_host(*manager.get_reader(handle, 0, 3).read_varlen())
    assert sorted(k.tolist()) == [1, 2] and len(d) == 3


@pytest.mark.parametrize("offsets,nbytes", [([0, 5, 3, 8], 8),
                                            ([0, 2, 4, 9], 8),
                                            ([1, 2, 4, 8], 8)])
def test_bad_offsets_raise_from_stop(manager, offsets, nbytes):
    from sparkrdma_amd.partitioner import HashPartitioner
    handle = manager.register_shuffle(num_maps=1, num_partitions=R)
    w = manager.get_writer(handle, 0)
    w.write_device_varlen(*to_dev(np.array([1, 2, 3], np.uint64),
                                  np.array(offsets, np.int64),
                                  np.zeros(nbytes, np.uint8)))
    with pytest.raises(ValueError, match="offsets"):
        w.stop(True, partitioner=HashPartitioner(R))
    assert w.metrics.records_written == 0 and w.metrics.bytes_written == 0
    # nothing was published: the map's entry in the driver table is unset
    from sparkrdma_amd.map_output import DriverTable
    entries = DriverTable.parse(manager._read_driver_table(handle))
    assert [key for _addr, key in entries] == [0]


def test_read_varlen_refuses_fixed_record_readers(manager):
    from sparkrdma_amd.partitioner import HashPartitioner
    from sparkrdma_amd.reader import ShuffleReader
    handle = manager.register_shuffle(num_maps=1, num_partitions=R)
    rng = np.random.default_rng(10)
    write(manager, handle, 0, make_rows(rng, 100, 10), HashPartitioner(R))
    rd = ShuffleReader(manager, handle, 0, R - 1, in_place=True)
    with pytest.raises(ValueError, match="read_varlen"):
        rd.read_varlen()
    for _ in rd:
        pass


def test_group_by_key_workload(engine):
    from sparkrdma_amd.workloads.groupby import GroupByKey
    g = GroupByKey(engine, rows_per_executor=50_000, num_keys=3000,
                   device="cuda", validate=True)
    res = g.run_step()
    assert res.rows == 50_000 and res.groups == 3000
