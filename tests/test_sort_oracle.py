"""The checkers of sort_oracle.py must reject wrong answers, or the GPU
edge tests that lean on them (test_gpu_sort_edges.py) could pass vacuously.
Each case hands check_sorted a hand-made output with exactly one kind of
defect. Also here: the pass-count helper and the digit windows the sort
wrappers derive from it, which need no GPU."""

import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from sort_oracle import check_sorted, expect_partition, window  # noqa: E402


def _case(n=300, hi=8, seed=0):
    """Keys with long runs of equal window values plus differing bits above
    the 8-bit window, index payload, and the true stable order."""
    rng = np.random.default_rng(seed)
    low = rng.integers(0, hi, n, dtype=np.uint64)
    high = rng.integers(0, 1 << 20, n, dtype=np.uint64) << np.uint64(8)
    keys = low | high
    order = np.argsort(low, kind="stable")
    return keys, np.arange(n), order


def _check(keys, order, start_bit=0, end_bit=8, stable=True):
    check_sorted(keys, np.arange(keys.size), keys[order], order, start_bit,
                 end_bit, stable)


def test_accepts_the_stable_argsort():
    keys, idx, order = _case()
    _check(keys, order, stable=True)
    _check(keys, order, stable=False)
    # int64 views of keys with the sign bit set are read as unsigned
    k = np.array([1 << 63, 5, (1 << 64) - 1, 0], dtype=np.uint64)
    order = np.argsort(k, kind="stable")
    check_sorted(k.view(np.int64), np.arange(4), k[order].view(np.int64),
                 order, 0, 64, True)


def test_rejects_swap_inside_a_run_of_equal_keys():
    keys, idx, order = _case()
    w = window(keys[order], 0, 8)
    j = int(np.flatnonzero(w[1:] == w[:-1])[0])
    bad = order.copy()
    bad[[j, j + 1]] = bad[[j + 1, j]]
    _check(keys, bad, stable=False)         # still ordered, pairs intact
    with pytest.raises(AssertionError, match="stable order"):
        _check(keys, bad, stable=True)


def test_rejects_key_with_its_neighbours_payload():
    keys, idx, order = _case()
    got_keys = keys[order]
    # a place where the neighbours differ as whole keys but not in the
    # window: the output stays ordered, only the pairing is broken
    w = window(got_keys, 0, 8)
    j = int(np.flatnonzero((w[1:] == w[:-1])
                           & (got_keys[1:] != got_keys[:-1]))[0])
    bad_payload = order.copy()
    bad_payload[[j, j + 1]] = bad_payload[[j + 1, j]]
    for stable in (False, True):
        with pytest.raises(AssertionError, match="parted from their payload"):
            check_sorted(keys, idx, got_keys, bad_payload, 0, 8, stable)


def test_rejects_duplicated_and_lost_row():
    keys, idx, order = _case()
    bad = order.copy()
    bad[11] = bad[10]                       # row order[11] lost, [10] twice
    for stable in (False, True):
        with pytest.raises(AssertionError, match="no permutation"):
            _check(keys, bad, stable=stable)
    # payload values outside [0, n) are no permutation either
    bad = order.copy()
    bad[0] = keys.size
    with pytest.raises(AssertionError, match="no permutation"):
        check_sorted(keys, idx, keys[order], bad, 0, 8, False)


def test_rejects_order_by_wider_window_as_stable():
    # sorted by bits [0, 12): the 4 bits above the window lead, so the
    # 8-bit window is not even ordered; masked to keys whose bits [8, 12)
    # are equal it is ordered but would not be stable for another reason
    keys, idx, _ = _case()
    wide = np.argsort(window(keys, 0, 12), kind="stable")
    with pytest.raises(AssertionError, match="not ordered"):
        _check(keys, wide, 0, 8, stable=True)
    # the same output is a correct stable answer for the window it sorted
    _check(keys, wide, 0, 12, stable=True)
    # ordered by the window AND 4 bits BELOW it: ordered, not stable
    keys = keys << np.uint64(4) | (np.arange(keys.size, dtype=np.uint64)[::-1]
                                   & np.uint64(15))
    low = np.argsort(window(keys, 0, 12), kind="stable")
    _check(keys, low, 4, 12, stable=False)
    with pytest.raises(AssertionError, match="stable order"):
        _check(keys, low, 4, 12, stable=True)


def test_rejects_one_adjacent_inversion():
    keys, idx, order = _case()
    w = window(keys[order], 0, 8)
    j = int(np.flatnonzero(w[1:] != w[:-1])[0])
    bad = order.copy()
    bad[[j, j + 1]] = bad[[j + 1, j]]
    for stable in (False, True):
        with pytest.raises(AssertionError, match="1 inversions"):
            _check(keys, bad, stable=stable)


def test_window_not_at_bit_zero():
    keys, idx, _ = _case()
    shifted = keys << np.uint64(44)
    order = np.argsort(window(shifted, 44, 52), kind="stable")
    _check(shifted, order, 44, 52, stable=True)
    with pytest.raises(AssertionError):
        _check(shifted, order[::-1].copy(), 44, 52, stable=False)


def test_expect_partition():
    keys = np.array([0x30, 0x10, 0x3F, 0x00, 0x1A], dtype=np.uint64)
    counts, order = expect_partition(keys, 4, 2)
    assert counts.tolist() == [1, 2, 0, 2]
    assert order.tolist() == [3, 1, 4, 0, 2]
    counts, order = expect_partition(np.zeros(0, dtype=np.uint64), 60, 4)
    assert counts.tolist() == [0] * 16 and order.size == 0
    top = np.array([(1 << 64) - 1, 1 << 63, 0], dtype=np.uint64)
    counts, order = expect_partition(top, 63, 1)
    assert counts.tolist() == [1, 2] and order.tolist() == [2, 0, 1]


def test_pass_helper_table():
    from sparkrdma_amd.ops.radix import onesweep_passes
    for s in range(0, 64):
        for e in range(s + 1, 65):
            assert onesweep_passes(s, e) == math.ceil((e - s) / 8), (s, e)
        for e in (65, 68, 72, 128):
            assert onesweep_passes(s, e) == onesweep_passes(s, 64), (s, e)
    for s, e in ((0, 0), (8, 8), (9, 8), (64, 64), (64, 72), (70, 72)):
        assert onesweep_passes(s, e) == 0, (s, e)
    # the cases the old floor division got wrong
    assert onesweep_passes(4, 64) == 8
    assert onesweep_passes(57, 64) == 1
    assert onesweep_passes(60, 64) == 1


def _cpu_lsd(keys, calls):
    """What the native calls do, in numpy: each call steps 8-bit digits up
    from its start bit, clamped to [56, 64), one stable pass per digit."""
    order = np.arange(keys.size)
    passes = 0
    for lo, hi in calls:
        for p in range(math.ceil((hi - lo) / 8)):
            sb = min(lo + 8 * p, 56)
            d = (keys[order] >> np.uint64(sb)) & np.uint64(255)
            order = order[np.argsort(d, kind="stable")]
            passes += 1
    return order, passes


def test_digit_windows_order_by_the_window():
    """Every window whose top is at bit 8 or above is served by native
    calls that leave it ordered, in onesweep_passes() passes in all, and
    stably when it is whole digits. One native call over a window that
    ends mid-digit would bin by bits above the window; shown for (0, 12)."""
    from sparkrdma_amd.ops.radix import _digit_windows, onesweep_passes
    rng = np.random.default_rng(5)
    keys = rng.integers(0, (1 << 64) - 1, 2000, dtype=np.uint64,
                        endpoint=True)
    for s in range(0, 64):
        for e in range(max(s + 1, 8), 65):
            calls = _digit_windows(s, e)
            order, passes = _cpu_lsd(keys, calls)
            assert passes == onesweep_passes(s, e), (s, e, calls)
            check_sorted(keys, np.arange(keys.size), keys[order], order, s, e,
                         stable=(e - s) % 8 == 0)
    assert _digit_windows(0, 12) == [(0, 8), (4, 12)]
    assert _digit_windows(4, 64) == [(4, 64)]
    assert _digit_windows(8, 72) == [(8, 64)]
    assert _digit_windows(8, 8) == []
    order, _ = _cpu_lsd(keys, [(0, 12)])
    with pytest.raises(AssertionError, match="not ordered"):
        check_sorted(keys, np.arange(keys.size), keys[order], order, 0, 12,
                     False)


def test_small_digit_check():
    from sparkrdma_amd.ops.radix import _check_small_digit
    for nbits in (1, 2, 3):
        _check_small_digit(nbits, 64 - nbits, 0)
        _check_small_digit(nbits, 64 - nbits, 1)
        _check_small_digit(nbits, 10, 2)        # range / hash-mod: no shift
        _check_small_digit(nbits, 10, 3)
        for func in (0, 1):
            with pytest.raises(ValueError, match="nbits"):
                _check_small_digit(nbits, 10, func)
    for nbits in range(4, 13):
        _check_small_digit(nbits, 10, 0)
