"""Variable-length rows: the wire format of sparkrdma_amd/varlen.py and the
CPU lane end to end (``write_varlen`` -> ``read_varlen``)."""

from collections import Counter

import numpy as np
import pytest

from sparkrdma_amd.conf import ShuffleConf
from sparkrdma_amd.driver import Driver
from sparkrdma_amd.manager import ShuffleManager
from sparkrdma_amd.partitioner import HashPartitioner
from sparkrdma_amd.varlen import (pack_varlen_segment, partition_varlen_np,
                                  segment_bytes, unpack_varlen_segment)

R = 16


def make_rows(rng, n, num_keys, max_len=64, long_rows=0):
    """n rows of length 0..max_len, plus ``long_rows`` of 10 000 bytes."""
    lens = rng.integers(0, max_len + 1, n)
    if long_rows:
        lens[rng.choice(n, long_rows, replace=False)] = 10_000
    offsets = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=offsets[1:])
    keys = rng.integers(0, num_keys, n, dtype=np.uint64)
    data = rng.integers(0, 256, int(offsets[-1]), dtype=np.uint8)
    return keys, offsets, data


def rows_of(keys, offsets, data):
    """The rows as a multiset of (key, payload)."""
    keys, offsets = np.asarray(keys), np.asarray(offsets)
    buf = np.asarray(data).tobytes()
    return Counter((int(keys[r]), buf[offsets[r]:offsets[r + 1]])
                   for r in range(len(keys)))


def check_csr(keys, offsets, data):
    assert len(offsets) == len(keys) + 1
    assert offsets[0] == 0 and offsets[-1] == len(data)
    assert np.all(np.diff(offsets) >= 0)


# ---------------------------------------------------------------- format


def test_pack_unpack_round_trip():
    rng = np.random.default_rng(0)
    keys, offsets, data = make_rows(rng, 300, 1 << 62, long_rows=1)
    seg = pack_varlen_segment(keys, offsets, data)
    k2, o2, d2 = unpack_varlen_segment(seg)
    assert k2.dtype == np.uint64 and o2.dtype == np.int64
    assert d2.dtype == np.uint8
    assert np.array_equal(k2, keys)
    assert np.array_equal(o2, offsets)
    assert np.array_equal(d2, data)
    # a memoryview of a longer buffer parses the same way
    k3, _o3, d3 = unpack_varlen_segment(memoryview(b"x" * 16 + seg)[16:])
    assert np.array_equal(k3, keys) and np.array_equal(d3, data)


@pytest.mark.parametrize("lens", [[5], [0], [0, 0, 0], [16], [1, 15],
                                  [7, 0, 9, 3]])
def test_header_and_padding(lens):
    n = len(lens)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    heap = int(offsets[-1])
    keys = np.arange(100, 100 + n, dtype=np.uint64)
    data = np.arange(1, heap + 1, dtype=np.uint8)
    seg = pack_varlen_segment(keys, offsets, data)
    assert len(seg) % 16 == 0
    assert len(seg) == segment_bytes(n, heap)
    assert len(seg) - (16 + 16 * n + heap) in range(16)
    words = np.frombuffer(seg[:16 + 16 * n], dtype="<u8")
    assert words[0] == n and words[1] == heap
    assert np.array_equal(words[2::2], keys)
    assert np.array_equal(words[3::2], offsets[1:].astype(np.uint64))
    assert seg[16 + 16 * n:16 + 16 * n + heap] == data.tobytes()
    assert set(seg[16 + 16 * n + heap:]) <= {0}


def test_no_rows_is_an_empty_segment():
    empty = (np.empty(0, np.uint64), np.zeros(1, np.int64),
             np.empty(0, np.uint8))
    assert pack_varlen_segment(*empty) == b""
    assert segment_bytes(0, 0) == 0
    k, o, d = unpack_varlen_segment(b"")
    assert len(k) == 0 and len(d) == 0 and o.tolist() == [0]


def test_unpack_rejects_malformed():
    seg = pack_varlen_segment(np.array([1, 2], np.uint64),
                              np.array([0, 3, 5], np.int64),
                              np.arange(5, dtype=np.uint8))
    with pytest.raises(ValueError):
        unpack_varlen_segment(seg[:-8])              # not a multiple of 16
    with pytest.raises(ValueError):
        unpack_varlen_segment(seg + bytes(16))       # header/length mismatch
    bad = bytearray(seg)
    bad[16 + 8:16 + 16] = (9).to_bytes(8, "little")  # end[0] > end[1]
    with pytest.raises(ValueError):
        unpack_varlen_segment(bytes(bad))


def test_partition_against_row_loop():
    rng = np.random.default_rng(1)
    keys, offsets, data = make_rows(rng, 2000, 500, long_rows=2)
    pids = rng.integers(0, R, len(keys))
    pids[pids == 5] = 6                              # partition 5 is empty
    segs = partition_varlen_np(keys, offsets, data, pids, R)
    assert len(segs) == R and segs[5] == b""
    buf = data.tobytes()
    for p in range(R):
        want_k, want_rows = [], []
        for r in range(len(keys)):                   # stable: input order
            if pids[r] == p:
                want_k.append(int(keys[r]))
                want_rows.append(buf[offsets[r]:offsets[r + 1]])
        k, o, d = unpack_varlen_segment(segs[p])
        check_csr(k, o, d)
        assert k.tolist() == want_k
        got = d.tobytes()
        assert [got[o[r]:o[r + 1]] for r in range(len(k))] == want_rows


# ------------------------------------------------------- CPU lane, end to end


@pytest.fixture
def cluster(tmp_path):
    conf = ShuffleConf(shm_dir=str(tmp_path), transport="shm",
                       max_buffer_allocation_size=1 << 30,
                       shuffle_write_block_size=1 << 16)
    driver = Driver(conf)
    conf.driver_port = driver.port
    managers = [ShuffleManager(conf, executor_id=i, driver_port=driver.port)
                for i in range(2)]
    yield managers
    for m in managers:
        m.stop()
    driver.stop()


def test_cpu_lane_end_to_end(cluster):
    rng = np.random.default_rng(2)
    part = HashPartitioner(R)
    # map 2 writes nothing; keys of maps 0 and 1 overlap
    handle = cluster[0].register_shuffle(3, R)
    inputs = [make_rows(rng, 5000, 700, long_rows=3) for _ in range(2)]
    want = Counter()
    for mid, (k, o, d) in enumerate(inputs):
        w = cluster[mid].get_writer(handle, mid)
        w.write_varlen(k[:2000], o[:2001], d)        # two batches
        w.write_varlen(k[2000:], o[2000:] - o[2000], d[o[2000]:])
        w.stop(True, partitioner=part)
        want += rows_of(k, o, d)
        assert w.metrics.records_written == 5000
        segs = partition_varlen_np(k, o, d, part.partition_ids(k), R)
        assert w.metrics.bytes_written == sum(len(s) for s in segs)
        # several pool blocks: no 64 KiB block holds them all
        assert w.metrics.bytes_written > 3 * (1 << 16)
    w = cluster[0].get_writer(handle, 2)
    w.write_varlen(np.empty(0, np.uint64), np.zeros(1, np.int64),
                   np.empty(0, np.uint8))
    w.stop(True, partitioner=part)
    assert w.metrics.records_written == 0 and w.metrics.bytes_written == 0

    k, o, d = cluster[1].get_reader(handle, 0, R - 1).read_varlen()
    check_csr(k, o, d)
    assert rows_of(k, o, d) == want

    k, o, d = cluster[0].get_reader(handle, 0, R - 1).read_varlen(
        ordering=True)
    check_csr(k, o, d)
    assert np.all(k[1:] >= k[:-1])
    assert rows_of(k, o, d) == want

    # partition by partition: every row once, and in its own partition
    seen = Counter()
    for p in range(R):
        k, o, d = cluster[1].get_reader(handle, p, p).read_varlen()
        assert np.all(part.partition_ids(k) == p)
        seen += rows_of(k, o, d)
    assert seen == want


def test_cpu_lane_empty_range(cluster):
    part = HashPartitioner(R)
    handle = cluster[0].register_shuffle(1, R)
    w = cluster[0].get_writer(handle, 0)
    key = np.full(10, 42, dtype=np.uint64)           # one key: one partition
    w.write_varlen(key, np.arange(11, dtype=np.int64) * 3,
                   np.arange(30, dtype=np.uint8))
    w.stop(True, partitioner=part)
    home = int(part.partition_ids(key[:1])[0])
    other = (home + 1) % R
    for ordering in (False, True):
        k, o, d = cluster[1].get_reader(handle, other, other).read_varlen(
            ordering=ordering)
        assert len(k) == 0 and len(d) == 0 and o.tolist() == [0]
        assert o.dtype == np.int64 and d.dtype == np.uint8
    k, o, d = cluster[1].get_reader(handle, home, home).read_varlen()
    assert len(k) == 10 and d.tolist() == list(range(30))


@pytest.mark.parametrize("offsets", [[1, 3, 5], [0, 4, 2], [0, 2, 9],
                                     [0, 2]])
def test_bad_offsets_raise(cluster, offsets):
    handle = cluster[0].register_shuffle(1, R)
    w = cluster[0].get_writer(handle, 0)
    with pytest.raises(ValueError):
        w.write_varlen(np.array([1, 2], np.uint64),
                       np.array(offsets, np.int64),
                       np.zeros(6, np.uint8))


def test_mixed_lanes_raise(cluster):
    handle = cluster[0].register_shuffle(1, R)
    rows = (np.array([1], np.uint64), np.array([0, 2], np.int64),
            np.zeros(2, np.uint8))
    w = cluster[0].get_writer(handle, 0)
    w.write_varlen(*rows)
    with pytest.raises(ValueError, match="mixed"):
        w.write_batch(np.array([1], np.uint64))
    with pytest.raises(ValueError, match="mixed"):
        w.write_records([(1, b"x")])
    w = cluster[0].get_writer(handle, 0)
    w.write_batch(np.array([1], np.uint64))
    with pytest.raises(ValueError, match="mixed"):
        w.write_varlen(*rows)
    w = cluster[0].get_writer(handle, 0)
    w.write_records([(1, b"x")])
    with pytest.raises(ValueError, match="mixed"):
        w.write_varlen(*rows)


def test_combiner_raises(cluster):
    handle = cluster[0].register_shuffle(1, R)
    w = cluster[0].get_writer(handle, 0)
    w.write_varlen(np.array([1], np.uint64), np.array([0, 2], np.int64),
                   np.zeros(2, np.uint8))
    with pytest.raises(ValueError, match="variable-length"):
        w.stop(True, partitioner=HashPartitioner(R), combiner="sum")
    # nothing changed: the plain stop still commits
    w.stop(True, partitioner=HashPartitioner(R))
    k, _o, d = cluster[1].get_reader(handle, 0, R - 1).read_varlen()
    assert k.tolist() == [1] and len(d) == 2


def test_read_varlen_refuses_fixed_record_readers(cluster):
    from sparkrdma_amd.reader import ShuffleReader
    handle = cluster[0].register_shuffle(1, R)
    w = cluster[0].get_writer(handle, 0)
    w.write_varlen(np.array([1], np.uint64), np.array([0, 2], np.int64),
                   np.zeros(2, np.uint8))
    w.stop(True, partitioner=HashPartitioner(R))
    for kw in ({"in_place": True}, {"records": (100, 10, None)},
               {"records": (100, 10, None), "in_place": True}):
        rd = ShuffleReader(cluster[1], handle, 0, R - 1, **kw)
        with pytest.raises(ValueError, match="read_varlen"):
            rd.read_varlen()
        for _ in rd:                                 # let the fetch finish
            pass
