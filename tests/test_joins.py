"""joins.merge_join_np, the numpy mirror of the GPU join family, against the
brute-force loop oracle of join_oracle.py for all six join types, and the
sql_join workload's CPU lane for each type."""

import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from join_oracle import assert_same, loop_join  # noqa: E402

from sparkrdma_amd.joins import (JOIN_TYPES, JoinOutput,  # noqa: E402
                                 check_join_type, merge_join_np)

U64 = np.uint64
SIGN_KEYS = np.array([0, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1], dtype=U64)


def _sorted_keys(rng, n, hi):
    return np.sort(rng.integers(0, hi, n, dtype=U64))


def _vals(rng, n):
    return rng.integers(1, 2 ** 64, n, dtype=U64)   # never 0: 0 means null


def _cases():
    rng = np.random.default_rng(11)
    c = {}
    c["random_dups"] = (_sorted_keys(rng, 1500, 400),
                        _sorted_keys(rng, 1100, 400))
    c["disjoint"] = (np.arange(0, 600, 2, dtype=U64),
                     np.arange(1, 500, 2, dtype=U64))
    c["all_equal"] = (np.full(120, 7, dtype=U64), np.full(150, 7, dtype=U64))
    c["empty_a"] = (np.empty(0, dtype=U64), _sorted_keys(rng, 50, 20))
    c["empty_b"] = (_sorted_keys(rng, 50, 20), np.empty(0, dtype=U64))
    c["both_empty"] = (np.empty(0, dtype=U64), np.empty(0, dtype=U64))
    c["single_match"] = (np.array([5], dtype=U64), np.array([5], dtype=U64))
    c["single_miss"] = (np.array([5], dtype=U64), np.array([6], dtype=U64))
    c["sign_bit"] = (np.sort(np.repeat(SIGN_KEYS, [3, 1, 2, 4])),
                     np.sort(np.repeat(SIGN_KEYS, [2, 2, 0, 3])))
    return c


CASES = _cases()


@pytest.mark.parametrize("how", JOIN_TYPES)
@pytest.mark.parametrize("case", sorted(CASES))
def test_merge_join_np_matches_loop_oracle(case, how):
    ak, bk = CASES[case]
    rng = np.random.default_rng(5)
    av, bv = _vals(rng, len(ak)), _vals(rng, len(bk))
    got = merge_join_np(ak, av, bk, bv, how, indices=True)
    assert isinstance(got, JoinOutput)
    want = loop_join(ak, av, bk, bv, how, indices=True)
    assert len(want["keys"]) <= 20_000
    assert_same(got, want, f"{case}/{how}")


@pytest.mark.parametrize("how", JOIN_TYPES)
def test_int64_keys_compare_unsigned(how):
    """int64 views of keys above 2^63 still order as unsigned, and the
    result's keys keep the input dtype."""
    ak, bk = CASES["sign_bit"]
    rng = np.random.default_rng(6)
    av, bv = _vals(rng, len(ak)), _vals(rng, len(bk))
    got = merge_join_np(ak.view(np.int64), av, bk.view(np.int64), bv, how)
    assert got.keys.dtype == np.int64
    assert got.a_idx is None and got.b_idx is None
    assert_same(got, loop_join(ak, av, bk, bv, how), how)


@pytest.mark.parametrize("how", JOIN_TYPES)
@pytest.mark.parametrize("drop", ("a", "b", "both"))
def test_vals_none(how, drop):
    ak, bk = CASES["random_dups"]
    rng = np.random.default_rng(7)
    av = None if drop in ("a", "both") else _vals(rng, len(ak))
    bv = None if drop in ("b", "both") else _vals(rng, len(bk))
    got = merge_join_np(ak, av, bk, bv, how, indices=True)
    if av is None:
        assert got.a_vals is None
    if bv is None:
        assert got.b_vals is None
    assert_same(got, loop_join(ak, av, bk, bv, how, indices=True),
                f"{how}/{drop}")


@pytest.mark.parametrize("how", ("left_semi", "left_anti"))
def test_one_sided_joins_have_no_b_fields(how):
    ak, bk = CASES["random_dups"]
    got = merge_join_np(ak, ak.copy(), bk, bk.copy(), how, indices=True)
    assert got.b_vals is None and got.b_valid is None and got.b_idx is None
    assert got.a_valid.all()


def test_empty_sides_follow_from_the_definitions():
    ak, bk = CASES["empty_b"]
    lo = merge_join_np(ak, ak.copy(), bk, bk.copy(), "left_outer",
                       indices=True)
    assert np.array_equal(lo.keys, ak) and not lo.b_valid.any()
    assert (lo.b_vals == 0).all() and (lo.b_idx == -1).all()
    anti = merge_join_np(ak, ak.copy(), bk, bk.copy(), "left_anti")
    assert np.array_equal(anti.keys, ak)
    assert len(merge_join_np(ak, None, bk, None, "inner").keys) == 0


def test_unknown_join_type_raises():
    ak, bk = CASES["single_match"]
    with pytest.raises(ValueError):
        merge_join_np(ak, None, bk, None, "cross")
    with pytest.raises(ValueError):
        check_join_type("outer")
    for how in JOIN_TYPES:
        check_join_type(how)


def test_bad_inputs_raise():
    ak, bk = CASES["single_match"]
    with pytest.raises(ValueError):
        merge_join_np(ak.astype(np.float64), None, bk, None, "inner")
    with pytest.raises(ValueError):
        merge_join_np(ak, np.zeros(3, dtype=U64), bk, None, "inner")


@pytest.fixture
def engine(tmp_path):
    from sparkrdma_amd.conf import ShuffleConf
    from sparkrdma_amd.engine import Engine
    # transport="shm": the host data plane also where a GPU is present, so
    # that the CPU lane under test reads numpy arrays
    conf = ShuffleConf(shm_dir=str(tmp_path), transport="shm",
                       max_buffer_allocation_size=1 << 30)
    eng = Engine(conf, rank=0, world_size=1, driver_port=0)
    yield eng
    eng.shutdown()


@pytest.mark.parametrize("how", JOIN_TYPES)
def test_sql_join_workload_cpu(engine, how):
    from sparkrdma_amd.workloads.sql_join import SortMergeJoin
    j = SortMergeJoin(engine, rows_per_executor=30_000,
                      partitions_per_executor=16, device="cpu",
                      key_space_bits=16, validate=True, how=how)
    r = j.run_step()
    assert r.how == how
    # 30k rows in a 16-bit key space: every count a type reports is > 0
    want_pos = {"inner": (1, 0, 0), "left_outer": (1, 1, 0),
                "right_outer": (1, 0, 1), "full_outer": (1, 1, 1),
                "left_semi": (1, 0, 0), "left_anti": (0, 1, 0)}[how]
    got = (r.matches, r.left_only, r.right_only)
    assert tuple(int(g > 0) for g in got) == want_pos, got


def test_sql_join_workload_inner_family_equals_default(engine):
    from sparkrdma_amd.workloads.sql_join import SortMergeJoin
    kw = dict(rows_per_executor=30_000, partitions_per_executor=16,
              device="cpu", key_space_bits=16, validate=True)
    old = SortMergeJoin(engine, **kw).run_step()
    new = SortMergeJoin(engine, kernel="family", **kw).run_step()
    assert old.how == new.how == "inner"
    assert old.matches == new.matches > 0
    assert (new.left_only, new.right_only) == (0, 0)
    with pytest.raises(ValueError):
        SortMergeJoin(engine, how="left_outer", kernel="sorted", **kw)
    with pytest.raises(ValueError):
        SortMergeJoin(engine, how="cross", **kw)
