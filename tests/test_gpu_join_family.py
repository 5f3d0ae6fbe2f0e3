"""The GPU join family (ops/join.py merge_join, ops/csrc/join.hip) for all
six join types: every output field exactly equal, order included, to the
loop oracle of join_oracle.py where the output is small and to
joins.merge_join_np (itself checked against that oracle in test_joins.py)
otherwise. T = EXPAND_TILE output rows per block of the expand kernel; a
block searches its range of driving rows in LDS up to EXPAND_LDS_ROWS rows
and in global memory beyond; a block of the probe kernel stages a window of
the searched side in LDS up to PROBE_LDS_KEYS keys. Both branches of both
kernels are pinned to shapes below.
"""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from join_oracle import assert_same, loop_join  # noqa: E402

from sparkrdma_amd.joins import JOIN_TYPES, merge_join_np, row_counts  # noqa: E402

pytestmark = pytest.mark.gpu

U64 = np.uint64
SIGN_KEYS = np.array([0, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1], dtype=U64)


@pytest.fixture(scope="module")
def J():
    from sparkrdma_amd.ops import join, load
    m = load()
    m.set_device(0)
    assert m.join_expand_tile() == join.EXPAND_TILE
    assert m.join_expand_lds_rows() == join.EXPAND_LDS_ROWS
    assert m.join_probe_lds_keys() == join.PROBE_LDS_KEYS
    return join


def _dev(x):
    import torch
    if x is None:
        return None
    return torch.from_numpy(np.array(x, copy=True).view(np.int64)).cuda()


def _vals(seed, n):
    # never 0 (0 means null) and unrelated to the keys
    return np.random.default_rng(seed).integers(1, 2 ** 64, n, dtype=U64)


def _gpu_join(J, ak, av, bk, bv, how, indices=True):
    import torch
    out = J.merge_join(_dev(ak), _dev(av), _dev(bk), _dev(bv), how=how,
                       indices=indices)
    torch.cuda.synchronize()
    assert out.keys.dtype == torch.int64 and out.a_valid.dtype == torch.bool
    return out


def _check(J, ak, bk, how, oracle, what, with_vals=True):
    av = _vals(1, len(ak)) if with_vals else None
    bv = _vals(2, len(bk)) if with_vals else None
    got = _gpu_join(J, ak, av, bk, bv, how)
    assert_same(got, oracle(ak, av, bk, bv, how, indices=True),
                f"{what}/{how}")
    return got


def _max_range(ak, bk, how, tile):
    """Longest range of driving rows any output tile spans, and the output
    total — which search branch the expand kernel takes for this shape."""
    if how == "right_outer":
        ak, bk = bk, ak
    m = np.searchsorted(bk, ak, "right") - np.searchsorted(bk, ak, "left")
    cnt = np.asarray(row_counts(m, how), dtype=np.int64)
    off = np.cumsum(cnt) - cnt
    total = int(cnt.sum())
    first = np.arange(0, total, tile, dtype=np.int64)
    last = np.minimum(first + tile, total) - 1
    i0 = np.searchsorted(off, first, "right") - 1
    i1 = np.searchsorted(off, last, "right") - 1
    return (int((i1 - i0 + 1).max()) if total else 0), total


# ---- shapes, built once -------------------------------------------------

def _random_dups():
    rng = np.random.default_rng(1)
    return (np.sort(rng.integers(0, 10_000, 100_003, dtype=U64)),
            np.sort(rng.integers(0, 10_000, 80_001, dtype=U64)))


def _sparse():
    rng = np.random.default_rng(2)
    return (np.sort(rng.integers(0, 1 << 40, 100_003, dtype=U64)),
            np.sort(rng.integers(0, 1 << 40, 80_001, dtype=U64)))


def _sparse_planted():
    """_sparse with every 20th key of A also put into B (every 200th
    twice): a few tiles of matches, 20 driving rows apart, so that every
    tile spans about 20 * T driving rows."""
    a, b = _sparse()
    return a, np.sort(np.concatenate((b, a[::20], a[::200])))


def _skew(T):
    hot = U64(1 << 33)
    lo_a = np.arange(0, 2000, 2, dtype=U64)             # 1000 below, even
    lo_b = np.arange(1, 2000, 2, dtype=U64)             # 1000 below, odd
    hi_a = hot + U64(2) + np.arange(0, 2000, 2, dtype=U64)
    hi_b = hot + U64(1) + np.arange(0, 2000, 2, dtype=U64)
    lo_b[::10] = lo_a[::10]                             # some shared keys
    hi_b[::10] = hi_a[::10]
    a = np.concatenate((lo_a, np.full(2 * T + 7, hot, dtype=U64), hi_a))
    b = np.concatenate((lo_b, np.full(257, hot, dtype=U64), hi_b))
    return a, b


SHAPES = {"random_dups": _random_dups, "sparse": _sparse,
          "sparse_planted": _sparse_planted}
_cache = {}


def _shape(name, T=None):
    if name not in _cache:
        _cache[name] = _skew(T) if name == "skew" else SHAPES[name]()
        for k in _cache[name]:
            assert np.all(k[1:] >= k[:-1])
            k.setflags(write=False)
    return _cache[name]


# ---- tests --------------------------------------------------------------

@pytest.mark.parametrize("how", JOIN_TYPES)
@pytest.mark.parametrize("shape", ("random_dups", "sparse", "sparse_planted",
                                   "skew"))
def test_large_shapes_match_numpy_mirror(J, shape, how):
    ak, bk = _shape(shape, J.EXPAND_TILE)
    _check(J, ak, bk, how, merge_join_np, shape)


def test_both_search_branches_run(J):
    """The shapes above reach both branches of the expand kernel's owner
    search, and tiles in the middle of a run."""
    T, cap = J.EXPAND_TILE, J.EXPAND_LDS_ROWS
    rng_dups, total = _max_range(*_shape("random_dups"), "inner", T)
    assert 1 < rng_dups <= cap and total > 4 * T            # LDS
    for how in ("inner", "left_semi"):                      # global
        r, total = _max_range(*_shape("sparse_planted"), how, T)
        assert r > cap and total > T, (how, r, total)
    # the hot run of A is a stretch of zero-count rows inside one anti tile
    r, _ = _max_range(*_shape("skew", T), "left_anti", T)
    assert r > cap
    # each hot row of A owns 257 rows: tiles lie inside one run
    r, total = _max_range(*_shape("skew", T), "inner", T)
    assert r <= cap and total >= (2 * T + 7) * 257
    # random 40-bit keys: (almost) nothing matches, left outer is all null
    _, total = _max_range(*_shape("sparse"), "inner", T)
    assert total < 16
    # the probe kernel: windows staged in LDS, and B's blocks inside the
    # hot key facing A's longer hot run, searched in global memory
    assert 0 < _max_probe_window(*_shape("random_dups")) <= J.PROBE_LDS_KEYS
    a, b = _shape("skew", T)
    assert _max_probe_window(a, b) <= J.PROBE_LDS_KEYS
    assert _max_probe_window(b, a) > J.PROBE_LDS_KEYS   # right / full outer


def _max_probe_window(pk, qk, block=256):
    """Longest stretch of Q that one block of probing rows can touch."""
    last = np.minimum(np.arange(block, len(pk) + block, block), len(pk)) - 1
    w = (np.searchsorted(qk, pk[last], "right")
         - np.searchsorted(qk, pk[::block], "left"))
    return int(w.max())


@pytest.mark.parametrize("how", JOIN_TYPES)
def test_all_equal(J, how):
    ak, bk = np.full(1_500, 42, dtype=U64), np.full(1_100, 42, dtype=U64)
    got = _check(J, ak, bk, how, merge_join_np, "all_equal")
    want_rows = {"inner": 1_650_000, "left_outer": 1_650_000,
                 "right_outer": 1_650_000, "full_outer": 1_650_000,
                 "left_semi": 1_500, "left_anti": 0}[how]
    assert got.keys.numel() == want_rows


@pytest.mark.parametrize("how", JOIN_TYPES)
@pytest.mark.parametrize("edge", (None, -1, 0, 1))
def test_tile_edges(J, edge, how):
    n = 1 if edge is None else J.EXPAND_TILE + edge
    k = (np.arange(n, dtype=U64) * U64(3)) + U64(5)
    _check(J, k, k.copy(), how, loop_join, f"n={n}")


@pytest.mark.parametrize("how", JOIN_TYPES)
@pytest.mark.parametrize("case", ("empty_a", "empty_b", "both_empty",
                                  "disjoint"))
def test_empty_and_disjoint(J, case, how):
    import torch
    some = np.sort(np.random.default_rng(3).integers(0, 50, 300, dtype=U64))
    none = np.empty(0, dtype=U64)
    ak, bk = {"empty_a": (none, some), "empty_b": (some, none),
              "both_empty": (none, none),
              "disjoint": (some * U64(2), some * U64(2) + U64(1))}[case]
    got = _check(J, ak, bk, how, loop_join, case)
    for f in ("keys", "a_vals", "a_idx"):
        assert getattr(got, f).dtype == torch.int64
    if how in ("inner", "left_semi") or case == "both_empty":
        assert got.keys.numel() == 0


@pytest.mark.parametrize("how", JOIN_TYPES)
def test_sign_bit_keys(J, how):
    ak = np.sort(np.repeat(SIGN_KEYS, [3, 1, 2, 4]))
    bk = np.sort(np.repeat(SIGN_KEYS, [2, 2, 0, 3]))
    _check(J, ak, bk, how, loop_join, "sign_bit")


@pytest.mark.parametrize("how", JOIN_TYPES)
def test_vals_none_and_indices_gather(J, how):
    """Without payloads the value outputs are None; gathering the inputs by
    the returned indices (-1 masked to null) rebuilds every other field."""
    import torch
    ak, bk = _shape("random_dups")
    av, bv = _vals(1, len(ak)), _vals(2, len(bk))
    bare = _gpu_join(J, ak, None, bk, None, how, indices=True)
    assert bare.a_vals is None and bare.b_vals is None
    full = _gpu_join(J, ak, av, bk, bv, how, indices=True)
    noidx = _gpu_join(J, ak, av, bk, bv, how, indices=False)
    assert noidx.a_idx is None and noidx.b_idx is None
    assert torch.equal(noidx.keys, full.keys)
    one_sided = how in ("left_semi", "left_anti")
    assert (full.b_vals is None) == one_sided
    assert (full.b_idx is None) == one_sided

    def gather(src, idx):
        src = _dev(src)
        out = torch.zeros(idx.numel(), dtype=torch.int64, device="cuda")
        ok = idx >= 0
        out[ok] = src[idx[ok]]
        return out

    for o in (bare, full):
        assert torch.equal(o.a_valid, o.a_idx >= 0)
        keys = gather(ak, o.a_idx)
        if not one_sided:
            assert torch.equal(o.b_valid, o.b_idx >= 0)
            keys = torch.where(o.a_valid, keys, gather(bk, o.b_idx))
        assert torch.equal(o.keys, keys)
    assert torch.equal(full.a_vals, gather(av, full.a_idx))
    if not one_sided:
        assert torch.equal(full.b_vals, gather(bv, full.b_idx))
    # one payload only
    half = _gpu_join(J, ak, None, bk, bv, how, indices=False)
    assert half.a_vals is None
    if not one_sided:
        assert torch.equal(half.b_vals, full.b_vals)


def test_inner_equals_merge_join_sorted(J):
    import torch
    ak, bk = _shape("random_dups")
    a, av, b, bv = (_dev(ak), _dev(_vals(1, len(ak))), _dev(bk),
                    _dev(_vals(2, len(bk))))
    jk, ja, jb = J.merge_join_sorted(a, av, b, bv)
    new = J.merge_join(a, av, b, bv, how="inner")
    torch.cuda.synchronize()
    assert jk.numel() > 0
    assert torch.equal(new.keys, jk)
    assert torch.equal(new.a_vals, ja) and torch.equal(new.b_vals, jb)
    assert bool(new.a_valid.all()) and bool(new.b_valid.all())


def test_bad_arguments_raise(J):
    import torch
    k = _dev(np.arange(8, dtype=U64))
    with pytest.raises(ValueError):
        J.merge_join(k, None, k, None, how="cross")
    with pytest.raises(ValueError):
        J.merge_join(k.to(torch.int32), None, k, None)
    with pytest.raises(ValueError):
        J.merge_join(k.cpu(), None, k, None)
    with pytest.raises(ValueError):
        J.merge_join(k[::2], None, k, None)
    with pytest.raises(ValueError):
        J.merge_join(k, k[:4].contiguous(), k, None)
    with pytest.raises(ValueError):
        J.merge_join(k, None, k, k.double())
    with pytest.raises(ValueError):
        J.merge_join(k.view(2, 4), None, k, None)


@pytest.fixture
def engine(tmp_path):
    from sparkrdma_amd.conf import ShuffleConf
    from sparkrdma_amd.engine import Engine
    conf = ShuffleConf(shm_dir=str(tmp_path), transport="ipc",
                       hbm_pool_size=2 << 30)
    eng = Engine(conf, rank=0, world_size=1, driver_port=0)
    yield eng
    eng.shutdown()


@pytest.mark.parametrize("how", JOIN_TYPES)
def test_sql_join_workload_gpu(engine, how):
    from sparkrdma_amd.workloads.sql_join import SortMergeJoin
    j = SortMergeJoin(engine, rows_per_executor=200_000,
                      partitions_per_executor=64, device="cuda",
                      key_space_bits=18, validate=True, how=how)
    r = j.run_step()
    assert r.how == how
    want_pos = {"inner": (1, 0, 0), "left_outer": (1, 1, 0),
                "right_outer": (1, 0, 1), "full_outer": (1, 1, 1),
                "left_semi": (1, 0, 0), "left_anti": (0, 1, 0)}[how]
    got = (r.matches, r.left_only, r.right_only)
    assert tuple(int(g > 0) for g in got) == want_pos, got


def test_sql_join_workload_gpu_inner_family_equals_default(engine):
    from sparkrdma_amd.workloads.sql_join import SortMergeJoin
    kw = dict(rows_per_executor=200_000, partitions_per_executor=64,
              device="cuda", key_space_bits=18, validate=True)
    old = SortMergeJoin(engine, **kw).run_step()
    new = SortMergeJoin(engine, kernel="family", **kw).run_step()
    assert old.matches == new.matches > 0
    assert (new.left_only, new.right_only) == (0, 0)
