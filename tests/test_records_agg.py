"""Keyed aggregation of wide records, CPU lane: the numpy mirror
(aggregate.reduce_records_np), the column checks both lanes share, the
reader hookup read_records_agg and the GroupByAggregate workload."""

import numpy as np
import pytest

from sparkrdma_amd.aggregate import (COLUMN_DTYPES, COLUMN_OPS, MAX_COLUMNS,
                                     check_columns, reduce_records_np)
from sparkrdma_amd.conf import ShuffleConf
from sparkrdma_amd.driver import Driver
from sparkrdma_amd.manager import ShuffleManager
from sparkrdma_amd.partitioner import HashPartitioner

NP_OF = {"i32": "<i4", "u32": "<u4", "i64": "<i8", "f32": "<f4", "f64": "<f8"}
W = 40
#: one field per dtype: (offset, dtype)
FIELDS = ((8, "i32"), (12, "u32"), (16, "i64"), (24, "f32"), (28, "f64"))


def _rows(rng, n, nkeys):
    """uint8 [n, 40]: u64 key | i32 | u32 | i64 | f32 | f64 | 4 pad bytes.
    Float fields are integer-valued below 2^20: sums are exact."""
    rows = rng.integers(0, 256, (n, W), dtype=np.uint8)

    def put(off, a):
        rows[:, off:off + a.dtype.itemsize] = \
            a.view(np.uint8).reshape(n, a.dtype.itemsize)
    put(0, rng.integers(0, nkeys, n, dtype=np.uint64).astype("<u8"))
    put(8, rng.integers(-(1 << 31), 1 << 31, n).astype("<i4"))
    put(12, rng.integers(0, 1 << 32, n).astype("<u4"))
    put(16, rng.integers(-(1 << 62), 1 << 62, n).astype("<i8"))
    put(24, rng.integers(-(1 << 20), 1 << 20, n).astype("<f4"))
    put(28, rng.integers(-(1 << 20), 1 << 20, n).astype("<f8"))
    return rows


def _field(rows, off, dtype):
    nd = np.dtype(NP_OF[dtype])
    return rows[:, off:off + nd.itemsize].copy().view(nd).reshape(-1)


def _wrap(x):
    return (x + (1 << 63)) % (1 << 64) - (1 << 63)


def _oracle(rows, off, dtype, op):
    """key -> reduction, by a python dict over python numbers."""
    keys = _field(rows, 0, "i64").tolist()
    if op == "count":
        out = {}
        for k in keys:
            out[k] = out.get(k, 0) + 1
        return out
    vals = _field(rows, off, dtype).tolist()
    out = {}
    for k, v in zip(keys, vals):
        if k not in out:
            out[k] = v
        elif op == "sum":
            out[k] = out[k] + v if isinstance(v, float) else _wrap(out[k] + v)
        else:
            out[k] = min(out[k], v) if op == "min" else max(out[k], v)
    return out


@pytest.fixture(scope="module")
def rows():
    return _rows(np.random.default_rng(5), 3000, 37)


@pytest.mark.parametrize("op", COLUMN_OPS)
@pytest.mark.parametrize("off,dtype", FIELDS)
def test_mirror_matches_dict_oracle(rows, off, dtype, op):
    keys, (col,) = reduce_records_np(rows, [(off, dtype, op)])
    assert keys.dtype == np.int64
    isfloat = dtype in ("f32", "f64") and op != "count"
    assert col.dtype == (np.float64 if isfloat else np.int64)
    assert np.all(keys.view(np.uint64)[1:] > keys.view(np.uint64)[:-1])
    assert dict(zip(keys.tolist(), col.tolist())) == \
        _oracle(rows, off, dtype, op)


def test_mirror_many_columns_end_bit_and_empty(rows):
    cols = [(8, "i32", "sum"), (28, "f64", "max"), (None, None, "count"),
            (0, "u32", "min")]           # the last one overlaps the key
    keys, vals = reduce_records_np(rows, cols, end_bit=8)
    assert len(vals) == 4 and all(len(v) == len(keys) for v in vals)
    assert dict(zip(keys.tolist(), vals[0].tolist())) == \
        _oracle(rows, 8, "i32", "sum")
    assert np.array_equal(vals[3], keys)          # keys < 2^32 here
    assert int(vals[2].sum()) == len(rows)
    k0, v0 = reduce_records_np(rows[:0], cols)
    assert k0.dtype == np.int64 and len(k0) == 0
    assert [v.dtype for v in v0] == [np.int64, np.float64, np.int64, np.int64]


def test_mirror_i64_sum_wraps():
    rows = np.zeros((3, 16), np.uint8)
    rows[:, 8:16] = np.array([2 ** 63 - 1, 2 ** 63 - 1, 5], "<i8") \
        .view(np.uint8).reshape(3, 8)
    _k, (s,) = reduce_records_np(rows, [(8, "i64", "sum")])
    assert s.tolist() == [_wrap(2 * (2 ** 63 - 1) + 5)]


@pytest.mark.parametrize("columns", [
    [(8, "i16", "sum")],                    # unknown dtype
    [(8, "i32", "mean")],                   # unknown op
    [(8, "i32", "sum_f64")],                # no float sum of an int column
    [(10, "i32", "sum")],                   # offset not a multiple of 4
    [(-4, "i32", "sum")],
    [(36, "i64", "sum")],                   # field past the record
    [(40, "i32", "sum")],
    [],                                     # C outside [1, max]
    [(8, "i32", "sum")] * (MAX_COLUMNS + 1),
    [(8, "i32")],                           # not a triple
])
def test_check_columns_rejects(columns):
    with pytest.raises(ValueError):
        check_columns(columns, W)


def test_check_columns_accepts():
    assert MAX_COLUMNS == 8
    got = check_columns([(36, "i32", "sum"), (32, "f64", "max"),
                         (None, None, "count")] + [(0, "u32", "min")] * 5, W)
    assert got[0] == (36, COLUMN_DTYPES.index("i32"), COLUMN_OPS.index("sum"))
    assert got[2][2] == COLUMN_OPS.index("count")
    with pytest.raises(ValueError):
        check_columns([(8, "i32", "sum")], 42)    # rec_bytes % 4


# ---------------------------------------------------------------------------
# reader end to end, two managers (the cluster of test_reader_aggregation)

@pytest.fixture
def cluster(tmp_path):
    # transport="shm": the CPU lane also where a GPU is visible
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


def _write(managers, R, rows_per_map):
    handle = managers[0].register_shuffle(len(managers), R)
    for mid, (mgr, rows) in enumerate(zip(managers, rows_per_map)):
        w = mgr.get_writer(handle, mid)
        w.write_batch(_field(rows, 0, "i64").view(np.uint64), rows[:, 8:])
        w.stop(True, partitioner=HashPartitioner(R))
    return handle


def test_read_records_agg_cpu(cluster):
    R = 4
    rng = np.random.default_rng(6)
    per_map = [_rows(rng, 1000, 50) for _ in range(2)]
    handle = _write(cluster, R, per_map)
    cols = [(8, "i32", "sum"), (12, "u32", "max"), (16, "i64", "min"),
            (24, "f32", "sum"), (28, "f64", "min"), (None, None, "count")]
    keys, vals = cluster[0].get_reader(handle, 0, R - 1) \
        .read_records_agg(W, cols)
    allrows = np.concatenate(per_map)
    assert len(keys) == 50
    for (off, dtype, op), col in zip(cols, vals):
        assert dict(zip(keys.tolist(), col.tolist())) == \
            _oracle(allrows, off, dtype, op), (off, dtype, op)
    wk, wv = reduce_records_np(allrows, cols)
    assert np.array_equal(keys, wk)
    assert all(np.array_equal(a, b) for a, b in zip(vals, wv))
    # a block that is not whole records
    with pytest.raises(ValueError):
        cluster[0].get_reader(handle, 0, R - 1).read_records_agg(
            44, [(None, None, "count")])
    with pytest.raises(ValueError):
        cluster[0].get_reader(handle, 0, R - 1).read_records_agg(
            W, [(40, "i32", "sum")])


def test_group_by_aggregate_workload_cpu(tmp_path):
    from sparkrdma_amd.engine import Engine
    from sparkrdma_amd.workloads import GroupByAggregate
    conf = ShuffleConf(shm_dir=str(tmp_path), transport="shm",
                       max_buffer_allocation_size=1 << 30)
    eng = Engine(conf, rank=0, world_size=1, driver_port=0)
    try:
        for Wb in (64, 40):
            wl = GroupByAggregate(eng, rows_per_executor=5000, num_keys=300,
                                  partitions_per_executor=8, device="cpu",
                                  validate=True, record_bytes=Wb)
            res = wl.run_step()
            assert res.groups == 300 and res.rows == 5000
            assert res.shuffle_bytes == 5000 * Wb
        with pytest.raises(ValueError):
            GroupByAggregate(eng, 10, record_bytes=36)
        with pytest.raises(ValueError):
            GroupByAggregate(eng, 10, record_bytes=42)
    finally:
        eng.shutdown()
