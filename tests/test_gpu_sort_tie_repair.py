"""Wide-record sort (kernels.hip sort_records_u64): the truncated sort with
tie repair and the full pass sequence, vs the numpy oracle, byte for byte: a
stable argsort of the 80-bit key. Keys of the truncated-sort tests are built
from the values sort_records_plan returns, so the position and length of
every run in the run-bit order is known, and every test asserts the path the
call took — a test of one path must not pass by way of another.

Every call sorts into a canary-guarded ``out`` with canary-guarded pair
buffers and a workspace of exactly sort_records_workspace_bytes bytes; all
guards must come back untouched."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CANARY = 0xA5
PAD = 256           # guard bytes on each side (keeps 16-byte alignment)


@pytest.fixture(scope="module")
def hs():
    from sparkrdma_amd.ops import load
    m = load()
    m.set_device(0)
    return m


def _oracle(arr, key_bytes):
    prefix = arr[:, :8].copy().view("<u8").ravel()
    if key_bytes == 8:
        return arr[np.argsort(prefix, kind="stable")]
    lo = arr[:, 8:10].copy().view("<u2").ravel()
    return arr[np.lexsort((lo, prefix))]      # stable, prefix is primary


def _guarded(nbytes):
    import torch
    buf = torch.full((PAD + nbytes + PAD,), CANARY, dtype=torch.uint8,
                     device="cuda")
    return buf, buf[PAD:PAD + nbytes]


def _check_guards(buf, what):
    got = buf.cpu().numpy()
    assert np.all(got[:PAD] == CANARY), what + ": written before"
    assert np.all(got[-PAD:] == CANARY), what + ": written past the end"


def _sort(hs, arr, key_bytes, end_bit=64, fuse=True, seg_lens=None):
    """sort_records with every buffer between canaries; returns (sorted
    records, path taken). ``seg_lens``: hand the records over as segments
    of these lengths, each a buffer of its own, instead of contiguously."""
    import torch
    from sparkrdma_amd.ops.radix import (sort_records,
                                         sort_records_workspace_bytes)
    n, W = arr.shape
    recs, segments = torch.from_numpy(arr.reshape(-1)).cuda(), None
    if seg_lens is not None:
        assert sum(seg_lens) == n
        firsts = np.cumsum([0] + list(seg_lens[:-1]))
        bufs = [recs[f * W:(f + c) * W].clone()
                for f, c in zip(firsts, seg_lens)]
        segments = [(int(f), c, b.data_ptr())
                    for f, c, b in zip(firsts, seg_lens, bufs)]
        recs = n * W
    out_buf, out = _guarded(n * W)
    pairs_buf, pairs = _guarded(n * 16)
    tmp_buf, tmp = _guarded(n * 16)
    ws_buf, ws = _guarded(sort_records_workspace_bytes(n, end_bit, key_bytes))
    res = sort_records(recs, W, key_bytes=key_bytes, end_bit=end_bit,
                       out=out, pairs=pairs.view(torch.int64),
                       tmp=tmp.view(torch.int64), ws=ws, fuse=fuse,
                       segments=segments)
    torch.cuda.synchronize()
    path = hs.last_sort_path()
    assert res.data_ptr() == out.data_ptr()
    for buf, what in ((out_buf, "out"), (pairs_buf, "pairs"),
                      (tmp_buf, "tmp"), (ws_buf, "ws")):
        _check_guards(buf, what)
    return out.cpu().numpy().reshape(n, W), path


def _records(rng, prefix, lo16, W):
    """Random payload (which tells records with equal keys apart, so the
    oracle comparison checks tie order), the input index as a tag at bytes
    12..16, and the given key."""
    n = prefix.size
    arr = rng.integers(0, 256, (n, W), dtype=np.uint8)
    arr[:, 12:16] = np.arange(n, dtype="<u4").view(np.uint8).reshape(n, 4)
    arr[:, :8] = prefix.astype("<u8").view(np.uint8).reshape(n, 8)
    arr[:, 8:10] = lo16.astype("<u2").view(np.uint8).reshape(n, 2)
    return arr


def _longest_run(prefix, lo_bit, run_bits):
    rv = (prefix >> np.uint64(lo_bit)) & np.uint64((1 << run_bits) - 1)
    return int(np.unique(rv, return_counts=True)[1].max())


def _engineered(hs, rng, W, key_bytes, end_bit=64, long_run=None,
                vary_top=False, dup_heavy=True):
    """n = 3T + 5 records whose run-bit order holds, at known positions:
    a run of 2 across the first tile boundary (T-1, T); a run of L (or
    ``long_run``) starting at 2T-1, its body wholly inside the halo; a run
    of 3 starting at 3T-1, the last element of the last full tile; a run
    of 2 ending at n-1; a run of 3 starting at position 0. Within the
    runs the low prefix bits and keylo16 come from a tiny range, so exact
    duplicates of full keys occur. Records are in shuffled input order."""
    T, L = hs.tie_repair_tile(), hs.tie_repair_max_run()
    n = 3 * T + 5
    lo_bit, passes, run_bits = hs.sort_records_plan(n, end_bit)
    assert passes > 0 and (1 << run_bits) > n
    top = end_bit - 8
    rv = np.arange(n, dtype=np.uint64)          # position p <-> run value
    runs = [(0, 3), (T - 1, 2), (2 * T - 1, long_run or L), (3 * T - 1, 3),
            (n - 2, 2), (100, 2), (T + 500, 5), (2 * T + 700, 4)]
    in_run = np.zeros(n, dtype=bool)
    for a, ln in runs:
        assert not in_run[a:a + ln].any()
        rv[a:a + ln] = a
        in_run[a:a + ln] = True
    low = rng.integers(0, 1 << lo_bit, n, dtype=np.uint64)
    lo16 = rng.integers(0, 1 << 16, n, dtype=np.uint64)
    if dup_heavy:
        k = int(in_run.sum())
        low[in_run] = rng.integers(0, 3, k, dtype=np.uint64)
        lo16[in_run] = rng.integers(0, 2, k, dtype=np.uint64)
    if key_bytes == 8:
        lo16[:] = rng.integers(0, 1 << 16, n, dtype=np.uint64)  # payload
    topd = (rng.integers(0, 256, n, dtype=np.uint64) if vary_top
            else np.full(n, 0x5A, dtype=np.uint64))
    above = np.uint64(0)
    if end_bit < 64:                 # bits above end_bit: constant, non-zero
        above = np.uint64(((1 << (64 - end_bit)) - 1) << end_bit)
    prefix = above | (topd << np.uint64(top)) | (rv << np.uint64(lo_bit)) | low
    want_longest = max(ln for _, ln in runs)
    assert _longest_run(prefix, lo_bit, run_bits) == want_longest
    perm = rng.permutation(n)
    return _records(rng, prefix[perm], lo16[perm], W)


# 1. random keys -----------------------------------------------------------

RANDOM_CASES = [(100_000, 100, 10), (7_777, 24, 8)]


def _random_case(hs, n, W, key_bytes):
    rng = np.random.default_rng(n)
    prefix = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    lo16 = rng.integers(0, 1 << 16, n, dtype=np.uint64)
    lo_bit, passes, run_bits = hs.sort_records_plan(n, 64)
    assert passes > 0
    # inputs first: a failure below then points at the kernel
    assert _longest_run(prefix, lo_bit, run_bits) <= hs.tie_repair_max_run()
    return _records(rng, prefix, lo16, W)


@pytest.mark.parametrize("n,W,key_bytes", RANDOM_CASES)
def test_random_keys(hs, n, W, key_bytes):
    arr = _random_case(hs, n, W, key_bytes)
    got, path = _sort(hs, arr, key_bytes)
    assert path == 1
    assert np.array_equal(got, _oracle(arr, key_bytes))


# 2. engineered runs -------------------------------------------------------

@pytest.mark.parametrize("W,key_bytes", [(100, 10), (24, 8)])
def test_engineered_runs(hs, W, key_bytes):
    arr = _engineered(hs, np.random.default_rng(W), W, key_bytes)
    got, path = _sort(hs, arr, key_bytes)
    assert path == 1
    assert np.array_equal(got, _oracle(arr, key_bytes))


# 3. one run of L + 1: fallback -------------------------------------------

def test_run_longer_than_L_falls_back(hs):
    L = hs.tie_repair_max_run()
    arr = _engineered(hs, np.random.default_rng(3), 100, 10, long_run=L + 1)
    got, path = _sort(hs, arr, 10)
    assert path == 2
    assert np.array_equal(got, _oracle(arr, 10))


# 4. top digits vary inside runs -------------------------------------------

def test_top_digits_vary_inside_runs(hs):
    arr = _engineered(hs, np.random.default_rng(4), 100, 10, vary_top=True)
    got, path = _sort(hs, arr, 10)
    assert path == 1
    assert np.array_equal(got, _oracle(arr, 10))


# 5. end_bit below 64 (the multi-GPU shape) ---------------------------------

@pytest.mark.parametrize("end_bit", [56, 52])
def test_end_bit_below_64(hs, end_bit):
    arr = _engineered(hs, np.random.default_rng(end_bit), 100, 10,
                      end_bit=end_bit, vary_top=True)
    got, path = _sort(hs, arr, 10, end_bit=end_bit)
    assert path == 1
    assert np.array_equal(got, _oracle(arr, 10))


# 6. edges -----------------------------------------------------------------

def test_edge_sizes(hs):
    T = hs.tie_repair_tile()
    rng = np.random.default_rng(6)
    for n in (1, 2, T - 1, T, T + 1):
        lo_bit, passes, run_bits = hs.sort_records_plan(n, 64)
        assert passes > 0
        # every position pairs with its neighbour: runs of 2 throughout,
        # one of them across the tile boundary when n > T
        rv = (np.arange(n, dtype=np.uint64) + np.uint64(n > T)) >> np.uint64(1)
        low = rng.integers(0, 2, n, dtype=np.uint64)
        prefix = (np.uint64(0x5A) << np.uint64(56)) | \
            (rv << np.uint64(lo_bit)) | low
        lo16 = rng.integers(0, 2, n, dtype=np.uint64)
        perm = rng.permutation(n)
        arr = _records(rng, prefix[perm], lo16[perm], 100)
        got, path = _sort(hs, arr, 10)
        assert path == 1, n
        assert np.array_equal(got, _oracle(arr, 10)), n


# 7. switch off == switch on -------------------------------------------------

def test_repair_off_gives_identical_bytes(hs):
    cases = [(_random_case(hs, n, W, kb), kb) for n, W, kb in RANDOM_CASES]
    cases.append((_engineered(hs, np.random.default_rng(7), 100, 10), 10))
    for arr, kb in cases:
        on, path_on = _sort(hs, arr, kb)
        hs.set_tie_repair(0)
        try:
            off, path_off = _sort(hs, arr, kb)
        finally:
            hs.set_tie_repair(1)
        assert (path_on, path_off) == (1, 0)
        assert np.array_equal(on, off)


def test_bypassed_without_fuse(hs):
    """fuse=False takes the full sequence and reports path 0."""
    import torch
    from sparkrdma_amd.ops.radix import sort_records
    arr = _engineered(hs, np.random.default_rng(8), 100, 10)
    recs = torch.from_numpy(arr.reshape(-1)).cuda()
    out = sort_records(recs, 100, key_bytes=10, fuse=False)
    torch.cuda.synchronize()
    assert hs.last_sort_path() == 0
    assert np.array_equal(out.cpu().numpy().reshape(arr.shape),
                          _oracle(arr, 10))


# 8. the full pass sequence ------------------------------------------------

def _shared_top(rng, n, W, end_bit):
    """Records whose prefix bits from end_bit up are equal (all ones) and
    random below; every fourth record repeats the full key of the one
    before it, so ties occur at every end_bit."""
    low = rng.integers(0, 1 << end_bit, n, dtype=np.uint64)
    lo16 = rng.integers(0, 1 << 16, n, dtype=np.uint64)
    dup = np.arange(3, n, 4)
    low[dup], lo16[dup] = low[dup - 1], lo16[dup - 1]
    above = np.uint64((((1 << (64 - end_bit)) - 1) << end_bit) & (2**64 - 1))
    return _records(rng, above | low, lo16, W)


def _full_sizes(hs):
    """One tile; one record past a 4096-pair onesweep tile; several
    tie-repair tiles."""
    return (1, 4097, 3 * hs.tie_repair_tile() + 5)


@pytest.mark.parametrize("end_bit", [64, 59, 8])
@pytest.mark.parametrize("fuse", [True, False])
@pytest.mark.parametrize("key_bytes", [8, 10])
def test_full_sequence(hs, key_bytes, fuse, end_bit):
    rng = np.random.default_rng(end_bit + key_bytes)
    hs.set_tie_repair(0)
    try:
        for n in _full_sizes(hs):
            arr = _shared_top(rng, n, 100, end_bit)
            got, path = _sort(hs, arr, key_bytes, end_bit=end_bit, fuse=fuse)
            assert path == 0, n
            assert np.array_equal(got, _oracle(arr, key_bytes)), n
    finally:
        hs.set_tie_repair(1)


@pytest.mark.parametrize("key_bytes", [8, 10])
def test_end_bit_zero(hs, key_bytes):
    """No prefix pass for the fused gather to ride: the plain gather must
    write every record. Order: the low 16-bit word alone (key_bytes 10),
    the input order (key_bytes 8)."""
    rng = np.random.default_rng(key_bytes)
    for n in _full_sizes(hs):
        arr = _shared_top(rng, n, 100, 0)
        got, path = _sort(hs, arr, key_bytes, end_bit=0, fuse=True)
        assert path == 0, n
        # `out` starts as canary bytes throughout: all of it is compared
        if key_bytes == 8:
            want = arr
        else:
            lo = arr[:, 8:10].copy().view("<u2").ravel()
            want = arr[np.argsort(lo, kind="stable")]
        assert np.array_equal(want, _oracle(arr, key_bytes)), n
        assert np.array_equal(got, want), n


@pytest.mark.parametrize("end_bit", [64, 59, 8])
@pytest.mark.parametrize("key_bytes", [8, 10])
def test_full_sequence_segmented(hs, key_bytes, end_bit):
    """Three segments of unequal length, one a single record, through the
    plain sort and gather_records: the contiguous result."""
    n = 3 * hs.tie_repair_tile() + 5
    arr = _shared_top(np.random.default_rng(end_bit), n, 100, end_bit)
    hs.set_tie_repair(0)
    try:
        want, path_c = _sort(hs, arr, key_bytes, end_bit=end_bit, fuse=False)
        got, path_s = _sort(hs, arr, key_bytes, end_bit=end_bit, fuse=False,
                            seg_lens=[4097, 1, n - 4098])
    finally:
        hs.set_tie_repair(1)
    assert (path_c, path_s) == (0, 0)
    assert np.array_equal(want, _oracle(arr, key_bytes))
    assert np.array_equal(got, want)


def test_workspace_size(hs):
    """sort_records_workspace_bytes covers the onesweep layout of the full
    sequence, is at most one 16-byte slot larger, and grows with end_bit."""
    from sparkrdma_amd.ops.radix import sort_records_workspace_bytes
    for n in (1, 4096, 4097):
        for key_bytes in (8, 10):
            prev = 0
            for end_bit in range(65):
                passes = -(-end_bit // 8) + (2 if key_bytes > 8 else 0)
                base = hs.onesweep_workspace_bytes(n, passes)
                got = sort_records_workspace_bytes(n, end_bit, key_bytes)
                assert base <= got <= base + 16, (n, key_bytes, end_bit)
                assert got >= prev, (n, key_bytes, end_bit)
                prev = got
