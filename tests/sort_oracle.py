"""Plain numpy checkers for the radix partition and sort kernels, shared by
test_sort_oracle.py (which proves they reject wrong answers) and
test_gpu_sort_edges.py. No torch, no GPU, nothing from sparkrdma_amd.

Keys are 64-bit arrays read as unsigned. Every comparison is exact integer
equality; a failed check raises AssertionError."""

import numpy as np


def _u64(a):
    a = np.ascontiguousarray(a)
    assert a.dtype in (np.uint64, np.int64), a.dtype
    return a.view(np.uint64)


def window(keys, start_bit, end_bit):
    """(k >> start_bit) & (2^(end_bit - start_bit) - 1) as uint64."""
    nbits = end_bit - start_bit
    assert 0 <= start_bit and 0 < nbits and end_bit <= 64
    mask = np.uint64((1 << nbits) - 1)
    return (_u64(keys) >> np.uint64(start_bit)) & mask


def expect_partition(keys_u64, shift, nbits):
    """One stable bucket-scatter pass by digit = (k >> shift) & (2^nbits-1):
    returns (counts int64[2^nbits], order) with out[j] = in[order[j]]."""
    digit = window(keys_u64, shift, shift + nbits).astype(np.int64)
    counts = np.bincount(digit, minlength=1 << nbits)
    return counts, np.argsort(digit, kind="stable")


def check_sorted(keys_in, payload_in, got_keys, got_payload, start_bit,
                 end_bit, stable):
    """``payload_in`` is arange(n), so ``got_payload`` names each output
    row's source row. Checks, in this order: no row lost or duplicated,
    every key still with its payload, the window value non-decreasing, and
    when ``stable`` the one permutation a stable sort by the window gives."""
    keys_in, got_keys = _u64(keys_in), _u64(got_keys)
    payload_in = np.asarray(payload_in).astype(np.int64)
    got_payload = np.asarray(got_payload).astype(np.int64)
    n = keys_in.size
    assert np.array_equal(payload_in, np.arange(n)), "payload_in != arange"
    assert got_keys.shape == (n,) and got_payload.shape == (n,), \
        f"output sizes {got_keys.shape}, {got_payload.shape} for n = {n}"
    seen = np.bincount(got_payload[(got_payload >= 0) & (got_payload < n)],
                       minlength=n)
    assert np.array_equal(seen, np.ones(n, dtype=seen.dtype)), \
        (f"payload is no permutation: {int((seen == 0).sum())} rows lost, "
         f"{int((seen > 1).sum())} duplicated")
    torn = np.flatnonzero(got_keys != keys_in[got_payload])
    assert torn.size == 0, \
        f"{torn.size} keys parted from their payload, first at {torn[:4]}"
    w = window(got_keys, start_bit, end_bit)
    inv = np.flatnonzero(w[1:] < w[:-1])
    assert inv.size == 0, \
        (f"bits [{start_bit}, {end_bit}) not ordered: {inv.size} inversions, "
         f"first after output row {inv[:4]}")
    if stable:
        want = np.argsort(window(keys_in, start_bit, end_bit), kind="stable")
        bad = np.flatnonzero(got_payload != want)
        assert bad.size == 0, \
            (f"not the stable order of bits [{start_bit}, {end_bit}): "
             f"{bad.size} rows differ, first at output row {bad[:4]}")
