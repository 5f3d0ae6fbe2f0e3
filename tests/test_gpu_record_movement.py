"""Record-moving kernels vs numpy oracles, byte for byte: gather_records
in both destination modes and the fused final sort pass. The kernels only
copy, so there is no tolerance. Every output sits between canary bytes
(and, in the partition layout, canaries between partitions) that must
come back untouched."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CANARY = 0xA5
# >= 256 canary bytes on each side; 260 leaves the written span only
# 4-byte aligned, the weakest alignment the kernels accept
PAD = 260


@pytest.fixture(scope="module")
def hs():
    from sparkrdma_amd.ops import load
    m = load()
    m.set_device(0)
    return m


def _block_records(W):
    """Records one gather block covers (kernels.hip gather_records)."""
    return min(1024, max(1, 32768 // (W // 4)))


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _records(rng, n, W):
    return rng.integers(0, 256, (n, W), dtype=np.uint8)


def _canary_buf(nbytes):
    import torch
    return torch.full((nbytes,), CANARY, dtype=torch.uint8, device="cuda")


# ---------------------------------------------------------------------------
# gather_records, dst_mode 0

@pytest.mark.parametrize("W", [8, 12, 24, 100, 104, 256])
def test_gather_mode0_permutation(hs, W):
    import torch
    B = _block_records(W)
    rng = np.random.default_rng(W)
    idx_base = 37          # records live idx_base slots into a larger arena
    for n in (1, 63, 64, 65, B - 1, B, B + 1, 3 * B + 17):
        arena = _records(rng, idx_base + n + 5, W)
        perm = rng.permutation(n).astype(np.uint64)
        pairs = np.empty((n, 2), dtype=np.uint64)
        pairs[:, 0] = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
        hi16 = rng.integers(1, 1 << 16, n, dtype=np.uint64)  # never zero
        pairs[:, 1] = (hi16 << np.uint64(48)) | (perm + np.uint64(idx_base))
        want = arena[idx_base + perm.astype(np.int64)]

        recs_t = torch.from_numpy(arena.reshape(-1)).cuda()
        pairs_t = torch.from_numpy(pairs.view(np.int64).reshape(-1)).cuda()
        buf = _canary_buf(PAD + n * W + PAD)
        hs.gather_records(recs_t.data_ptr(), pairs_t.data_ptr(), n, W, 0,
                          buf.data_ptr() + PAD, 0, 0, 0, 0, 0, 0, _stream())
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert np.all(got[:PAD] == CANARY), (W, n)
        assert np.all(got[PAD + n * W:] == CANARY), (W, n)
        assert np.array_equal(got[PAD:PAD + n * W].reshape(n, W), want), (W, n)


# ---------------------------------------------------------------------------
# gather_records, dst_mode 1 (partition layout)

def _digits(keys, case):
    if case["func"] == 2:      # kPartRange: mulhi(key, nparts)
        return np.array([(int(k) * case["nparts"]) >> 64 for k in keys],
                        dtype=np.int64)
    return ((keys >> np.uint64(case["shift"])) &
            np.uint64(case["nd"] - 1)).astype(np.int64)


MODE1_CASES = {
    "16_digits": dict(nd=16, shift=60, func=0, nparts=0),
    "256_digits": dict(nd=256, shift=56, func=0, nparts=0),
    "empty_digit": dict(nd=16, shift=60, func=0, nparts=0, empty=3),
    "one_digit": dict(nd=16, shift=60, func=0, nparts=0, only=9),
    "range_12_parts": dict(nd=16, shift=0, func=2, nparts=12),
}


@pytest.mark.parametrize("W", [24, 100])
@pytest.mark.parametrize("name", list(MODE1_CASES))
def test_gather_mode1_partitions(hs, name, W):
    import torch
    case = MODE1_CASES[name]
    nd = case["nd"]
    n = 3 * _block_records(W) + 17
    rng = np.random.default_rng(len(name) * 1000 + W)
    arr = _records(rng, n, W)
    keys = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    if "empty" in case:
        hit = (keys >> np.uint64(60)) == np.uint64(case["empty"])
        keys[hit] ^= np.uint64(1 << 63)       # move them to another digit
    if "only" in case:
        keys = (keys >> np.uint64(4)) | np.uint64(case["only"] << 60)
    d = _digits(keys, case)
    if "empty" in case:
        assert not np.any(d == case["empty"])
    if "only" in case:
        assert np.all(d == case["only"])

    # pairs grouped by digit (stable), as the scatter kernel leaves them
    order = np.argsort(d, kind="stable")
    hi16 = rng.integers(1, 1 << 16, n, dtype=np.uint64)
    pairs = np.empty((n, 2), dtype=np.uint64)
    pairs[:, 0] = keys[order]
    pairs[:, 1] = (hi16 << np.uint64(48)) | order.astype(np.uint64)
    counts = np.bincount(d, minlength=nd)
    starts = np.zeros(nd, dtype=np.int64)
    np.cumsum(counts[:-1], out=starts[1:])

    # destination: PAD | part 0 | PAD | part 1 | ... | PAD — with W = 100
    # and PAD = 260 the partition bases are only 4-byte aligned
    offs = np.zeros(nd, dtype=np.int64)
    pos = PAD
    for p in range(nd):
        offs[p] = pos
        pos += int(counts[p]) * W + PAD
    buf = _canary_buf(pos)
    want = np.full(pos, CANARY, dtype=np.uint8)
    grouped = arr[order]
    for p in range(nd):
        seg = grouped[starts[p]:starts[p] + counts[p]].reshape(-1)
        want[offs[p]:offs[p] + seg.size] = seg

    recs_t = torch.from_numpy(arr.reshape(-1)).cuda()
    pairs_t = torch.from_numpy(pairs.view(np.int64).reshape(-1)).cuda()
    dst_addr = torch.from_numpy(buf.data_ptr() + offs).cuda()
    dstart = torch.from_numpy(starts.astype(np.uint32).view(np.int32)).cuda()
    hs.gather_records(recs_t.data_ptr(), pairs_t.data_ptr(), n, W, 1, 0,
                      dst_addr.data_ptr(), dstart.data_ptr(), case["shift"],
                      nd - 1, case["func"], case["nparts"], _stream())
    torch.cuda.synchronize()
    # one comparison covers the records AND every canary gap
    assert np.array_equal(buf.cpu().numpy(), want)


# ---------------------------------------------------------------------------
# fused final sort pass

def _sort_oracle(arr, key_bytes):
    prefix = arr[:, :8].copy().view("<u8").ravel()
    if key_bytes == 8:
        return arr[np.argsort(prefix, kind="stable")]
    lo = arr[:, 8:10].copy().view("<u2").ravel()
    return arr[np.lexsort((lo, prefix))]      # stable, prefix is primary


def _sort_guarded(arr, W, key_bytes, fuse):
    """sort_records into a canary-guarded buffer; returns the records after
    checking the guards."""
    import torch
    from sparkrdma_amd.ops.radix import sort_records
    n = arr.shape[0]
    recs = torch.from_numpy(arr.reshape(-1)).cuda()
    buf = _canary_buf(PAD + n * W + PAD)
    out = sort_records(recs, W, key_bytes=key_bytes,
                       out=buf[PAD:PAD + n * W], fuse=fuse)
    torch.cuda.synchronize()
    assert out.data_ptr() == buf.data_ptr() + PAD
    got = buf.cpu().numpy()
    assert np.all(got[:PAD] == CANARY), (n, W, key_bytes, fuse)
    assert np.all(got[PAD + n * W:] == CANARY), (n, W, key_bytes, fuse)
    return got[PAD:PAD + n * W].reshape(n, W)


@pytest.mark.parametrize("key_bytes", [8, 10])
@pytest.mark.parametrize("W", [12, 100, 256])
def test_fused_sort_matches_oracle_and_unfused(hs, W, key_bytes):
    rng = np.random.default_rng(W * 16 + key_bytes)
    for n in (1, 4095, 4096, 4097, 3 * 4096 + 17):
        arr = _records(rng, n, W)
        want = _sort_oracle(arr, key_bytes)
        fused = _sort_guarded(arr, W, key_bytes, fuse=True)
        plain = _sort_guarded(arr, W, key_bytes, fuse=False)
        assert np.array_equal(fused, want), (n, W, key_bytes)
        assert np.array_equal(plain, want), (n, W, key_bytes)


def _equal_prefix_records(rng, n, W):
    """Few distinct keys, so most neighbours tie; the random payload tells
    equal-key records apart, which makes the oracle comparison a
    stability check."""
    arr = _records(rng, n, W)
    prefixes = rng.integers(0, 2 ** 64, 5, dtype=np.uint64)
    arr[:, :8] = prefixes[rng.integers(0, 5, n)].view(np.uint8).reshape(n, 8)
    arr[:, 8] = rng.integers(0, 3, n)
    arr[:, 9] = 0
    return arr


@pytest.mark.parametrize("key_bytes", [8, 10])
def test_fused_sort_stable_on_equal_prefixes(hs, key_bytes):
    rng = np.random.default_rng(77)
    n, W = 3 * 4096 + 17, 100
    arr = _equal_prefix_records(rng, n, W)
    want = _sort_oracle(arr, key_bytes)
    assert np.array_equal(_sort_guarded(arr, W, key_bytes, fuse=True), want)
