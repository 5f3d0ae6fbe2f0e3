"""Local wide-record blocks read in place (kernels.hip extract_records and
record_src, pool.cpp extract_records_batch, the fetcher's in-place lane,
sort_records(segments=...)), byte for byte: nothing here computes, records
are only found, repacked and moved, so there is no tolerance.

Kernel: the pairs must equal the numpy formula and what fetch_records and
extract_pairs write for the same bytes; canaries around the pairs and the
source itself must come back untouched. Sort: records scattered over 1, 2,
37 and 1000 segments sort to the bytes a contiguous buffer gives, on every
path of sort_records. Fetcher and TeraSort: conf ``inplace`` against
``local`` and ``off``."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CANARY = 0xA5
POISON = 0xEE
PAD = 256                 # canary bytes on each side of the pairs
SRC_OFF = 4               # the source starts 4 bytes into its buffer
IDX_BASES = (37, (1 << 40) + 37)


@pytest.fixture(scope="module")
def hs():
    from sparkrdma_amd.ops import load
    m = load()
    m.set_device(0)
    return m


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def _want_pairs(arr, key_bytes, idx_base):
    """numpy formula: (u64 LE prefix, keylo16 << 48 | idx_base + e)."""
    n = len(arr)
    want = np.empty((n, 2), dtype=np.uint64)
    want[:, 0] = arr[:, :8].copy().view("<u8").ravel()
    aux = np.uint64(idx_base) + np.arange(n, dtype=np.uint64)
    if key_bytes > 8:
        aux |= arr[:, 8:10].copy().view("<u2").ravel().astype(np.uint64) \
            << np.uint64(48)
    want[:, 1] = aux
    return want


# ---------------------------------------------------------------------------
# extract-only kernel


class _Run:
    """One (src, size) entry with its buffers and expectations."""

    def __init__(self, rng, n, W, key_bytes, idx_base):
        import torch
        self.n, self.W, self.key_bytes, self.idx_base = n, W, key_bytes, idx_base
        self.arr = rng.integers(0, 256, (n, W), dtype=np.uint8)
        host = np.full(SRC_OFF + n * W + 12, 0x3C, dtype=np.uint8)
        host[SRC_OFF:SRC_OFF + n * W] = self.arr.reshape(-1)
        self.src_host = host
        self.src = torch.from_numpy(host).cuda()
        self.pairs = torch.full((PAD + 16 * n + PAD,), CANARY,
                                dtype=torch.uint8, device="cuda")
        assert self.src.data_ptr() % 16 == 0 and self.pairs.data_ptr() % 16 == 0

    @property
    def entry(self):
        return (self.src.data_ptr() + SRC_OFF, self.n * self.W,
                self.pairs.data_ptr() + PAD, self.idx_base)

    def check(self, hs):
        import torch
        n, W = self.n, self.W
        pr = self.pairs.cpu().numpy()
        assert np.all(pr[:PAD] == CANARY), "canary before pairs"
        assert np.all(pr[PAD + 16 * n:] == CANARY), "canary after pairs"
        got = pr[PAD:PAD + 16 * n].copy().view("<u8").reshape(n, 2)
        want = _want_pairs(self.arr, self.key_bytes, self.idx_base)
        assert np.array_equal(got, want), "pairs != numpy formula"
        src = self.src.data_ptr() + SRC_OFF
        ref = torch.empty(2 * n, dtype=torch.int64, device="cuda")
        hs.extract_pairs(src, n, W, self.key_bytes, ref.data_ptr(), _stream(),
                         idx_base=self.idx_base)
        torch.cuda.synchronize()
        assert np.array_equal(
            got, ref.cpu().numpy().view(np.uint64).reshape(n, 2)), \
            "pairs != extract_pairs"
        ref.fill_(-1)
        dst = torch.empty(n * W, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        hs.wait_event(hs.read_records_batch(
            0, [dst.data_ptr()], [src], [n * W], W, self.key_bytes,
            [ref.data_ptr()], [self.idx_base]))
        assert np.array_equal(
            got, ref.cpu().numpy().view(np.uint64).reshape(n, 2)), \
            "pairs != fetch_records"
        assert np.array_equal(self.src.cpu().numpy(), self.src_host), \
            "source modified"


def _extract(hs, runs):
    import torch
    torch.cuda.synchronize()          # buffers filled on torch's stream
    e = [r.entry for r in runs]
    ev = hs.extract_records_batch(
        0, [x[0] for x in e], [x[1] for x in e], runs[0].W,
        runs[0].key_bytes, [x[2] for x in e], [x[3] for x in e])
    hs.wait_event(ev)


@pytest.mark.parametrize("W,key_bytes", [(12, 10), (100, 10), (100, 8),
                                         (256, 8)])
def test_extract_records_vs_oracles(hs, W, key_bytes):
    T = hs.fetch_block_records(W)     # records per block of the kernel
    rng = np.random.default_rng(W * 16 + key_bytes)
    for n in (1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17):
        for idx_base in IDX_BASES:
            run = _Run(rng, n, W, key_bytes, idx_base)
            _extract(hs, [run])
            run.check(hs)


def test_three_entries_one_event(hs):
    W = 100
    T = hs.fetch_block_records(W)
    rng = np.random.default_rng(5)
    runs = [_Run(rng, T + 3, W, 10, 37), _Run(rng, 1, W, 10, (1 << 40) + 37),
            _Run(rng, 200, W, 10, 5000)]
    _extract(hs, runs)
    for run in runs:
        run.check(hs)


def test_rejects_partial_records(hs):
    rng = np.random.default_rng(6)
    run = _Run(rng, 4, 100, 10, 0)
    s, size, p, b = run.entry
    with pytest.raises(RuntimeError):
        hs.extract_records_batch(0, [s], [size - 4], 100, 10, [p], [b])
    with pytest.raises(RuntimeError):
        hs.extract_records_batch(0, [s], [size], 100, 10, [p], [b, b])


# ---------------------------------------------------------------------------
# segmented sort

N_REC, R_PARTS = 5000, 8
SEG_COUNTS = (1, 2, 37, 1000)


def _mk_records(rng, n, W):
    arr = rng.integers(0, 256, (n, W), dtype=np.uint8)
    # a run of equal prefixes, so the 16 low key bits decide some orders;
    # they are distinct, so the sorted output does not depend on the order
    # in which the fetches were laid out in the arena
    tied = np.arange(1, 141, 7)     # 20 records: a run the tie repair handles
    arr[tied, :8] = arr[0, :8]
    arr[tied, 8:10] = tied.astype("<u2").view(np.uint8).reshape(-1, 2)
    return arr


_INPUTS = {}


def _input(W, all_equal):
    """(records, numpy oracle of the sorted bytes), built once per shape."""
    key = (W, all_equal)
    if key not in _INPUTS:
        arr = _mk_records(np.random.default_rng(21 + W), N_REC, W)
        if all_equal:
            arr[:, :8] = arr[0, :8]   # one run of 5000 > 32: the fallback
        prefix = arr[:, :8].copy().view("<u8").ravel()
        lo = arr[:, 8:10].copy().view("<u2").ravel()
        order = np.lexsort((np.arange(N_REC), lo, prefix))   # stable, 80 bits
        arr.setflags(write=False)
        want = arr[order].reshape(-1)
        want.setflags(write=False)
        _INPUTS[key] = (arr, want)
    return _INPUTS[key]


def _cuts(nseg):
    """Segment boundaries in record indices: uneven, some of one record."""
    if nseg == 1:
        return [0, N_REC]
    if nseg == 2:
        return [0, 1777, N_REC]
    if nseg == 1000:
        return list(range(0, N_REC + 1, 5))
    rng = np.random.default_rng(nseg)
    inner = set(rng.choice(np.arange(3, N_REC - 3), nseg - 7, replace=False)
                .tolist())
    inner |= {1, 2, N_REC - 1}        # records 0, 1 and the last: alone
    while len(inner) < nseg - 1:
        inner.add(int(rng.integers(3, N_REC - 3)))
    cuts = [0] + sorted(inner) + [N_REC]
    assert len(cuts) == nseg + 1
    return cuts


def _scatter(arr, nseg):
    """Lay the records out as nseg segments. Returns (segments, tensors to
    keep alive). 2 segments: one buffer, the second segment at the LOWER
    address. 37: one allocation each, poisoned on both sides. 1000: one
    buffer with 12 poisoned bytes between neighbours (not contiguous, so
    nothing can be merged)."""
    import torch
    W = arr.shape[1]
    cuts = _cuts(nseg)
    spans = list(zip(cuts[:-1], cuts[1:]))
    if nseg == 37:
        segs, keep = [], []
        for a, b in spans:
            host = np.full(28 + (b - a) * W + 36, POISON, dtype=np.uint8)
            host[28:28 + (b - a) * W] = arr[a:b].reshape(-1)
            t = torch.from_numpy(host).cuda()
            keep.append(t)
            segs.append((a, b - a, t.data_ptr() + 28))
        assert sum(1 for _a, c, _p in segs if c == 1) >= 3
        return segs, keep
    gap = 12
    host = np.full(N_REC * W + gap * (nseg + 1), POISON, dtype=np.uint8)
    offs, pos = {}, gap
    for a, b in (reversed(spans) if nseg == 2 else spans):
        host[pos:pos + (b - a) * W] = arr[a:b].reshape(-1)
        offs[a] = pos
        pos += (b - a) * W + gap
    t = torch.from_numpy(host).cuda()
    segs = [(a, b - a, t.data_ptr() + offs[a]) for a, b in spans]
    if nseg == 2:
        assert segs[1][2] < segs[0][2]
    return segs, [t]


def _sort(hs, arr, segments, fuse=True, pairs_filled=True):
    """sort_records on a contiguous buffer (segments None) or on segments;
    the pairs always come from the contiguous bytes when pairs_filled."""
    import torch
    from sparkrdma_amd.ops.radix import extract_pairs, sort_records
    W = arr.shape[1]
    recs = torch.from_numpy(arr.reshape(-1).copy()).cuda()
    pairs = extract_pairs(recs, W, 10) if pairs_filled else None
    out = sort_records(recs if segments is None else N_REC * W, W,
                       key_bytes=10, pairs=pairs, pairs_filled=pairs_filled,
                       fuse=fuse, segments=segments)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("variant", ["default", "unfused", "no_tie_repair",
                                     "all_equal"])
@pytest.mark.parametrize("W", [100, 256])
def test_segmented_sort_matches_contiguous(hs, W, variant):
    arr, want = _input(W, variant == "all_equal")
    fuse = variant != "unfused"
    try:
        if variant == "no_tie_repair":
            hs.set_tie_repair(0)
        base = _sort(hs, arr, None, fuse=fuse)
        assert np.array_equal(base, want), "contiguous sort != numpy oracle"
        for nseg in SEG_COUNTS:
            segs, keep = _scatter(arr, nseg)
            assert len(segs) == nseg
            got = _sort(hs, arr, segs, fuse=fuse)
            assert np.array_equal(got, base), (W, variant, nseg)
            path = hs.last_sort_path()
            if variant == "all_equal":
                assert path == 2, "a run of 5000 must take the fallback"
            elif variant == "default":
                assert path == 1
            else:
                assert path == 0
            del keep
    finally:
        hs.set_tie_repair(1)


@pytest.mark.parametrize("W", [100, 256])
def test_segmented_sort_extracts_per_segment(hs, W):
    """pairs_filled=False: the pairs come from the segments themselves,
    each with its own idx_base."""
    arr, want = _input(W, False)
    for nseg in SEG_COUNTS:
        segs, keep = _scatter(arr, nseg)
        got = _sort(hs, arr, segs, pairs_filled=False)
        assert np.array_equal(got, want), (W, nseg)
        del keep


def test_segments_must_cover_every_record(hs):
    arr, _want = _input(100, False)
    segs, _keep = _scatter(arr, 37)
    with pytest.raises(ValueError):
        _sort(hs, arr, segs[:-1])
    with pytest.raises(ValueError):
        _sort(hs, arr, segs + [segs[3]])


# ---------------------------------------------------------------------------
# fetcher: in place against local and off

W_REC = 100
FILL = 0x5A


def _shuffle_once(tmp_path, mode, arena_bytes):
    """Write N_REC records through a world-1 manager and fetch them back
    with in_place=True under conf.fused_record_fetch = mode. Returns a dict
    of what the consumer sees, with the records sorted through
    record_segments() while the shuffle is still registered."""
    import torch
    from sparkrdma_amd.conf import ShuffleConf
    from sparkrdma_amd.driver import Driver
    from sparkrdma_amd.manager import ShuffleManager
    from sparkrdma_amd.ops import load
    from sparkrdma_amd.ops.radix import sort_records
    from sparkrdma_amd.partitioner import RangePartitioner
    from sparkrdma_amd.reader import DeviceView

    hs = load()
    conf = ShuffleConf(shm_dir=str(tmp_path), transport="ipc",
                       hbm_pool_size=1 << 30,
                       shuffle_write_block_size=256 << 10,
                       shuffle_read_block_size=4 << 10,
                       fused_record_fetch=mode)
    driver = Driver(conf)
    mgr = ShuffleManager(conf, executor_id=0, driver_port=driver.port)
    try:
        handle = mgr.register_shuffle(num_maps=1, num_partitions=R_PARTS)
        arr = _mk_records(np.random.default_rng(21), N_REC, W_REC)
        recs = torch.from_numpy(arr.reshape(-1)).cuda()
        w = mgr.get_writer(handle, 0)
        w.write_device_records(recs, W_REC, key_bytes=10)
        w.stop(True, partitioner=RangePartitioner.uniform(R_PARTS))
        hint = torch.full((arena_bytes,), FILL, dtype=torch.uint8,
                          device="cuda")
        pairs = torch.full((2 * (arena_bytes // W_REC) + 16,), -1,
                           dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        reader = mgr.get_reader(handle, 0, R_PARTS - 1, arena=hint,
                                records=(W_REC, 10, pairs), in_place=True)
        views = [v for _ref, v in reader]
        assert len(views) > 1
        f = reader.fetcher
        total = f.total_bytes
        assert total == N_REC * W_REC
        segs = f.record_segments()
        grew = f._arena_buf is not hint
        s = torch.cuda.current_stream().cuda_stream
        done = None
        if not grew:
            # the consumer's side of the contract: pairs of the ranges the
            # kernels did not serve are extracted from the arena buffer
            pos = 0
            for off, ln in f.pair_ranges() + [(total, 0)]:
                if off > pos:
                    hs.extract_pairs(
                        f._arena_buf.data_ptr() + pos, (off - pos) // W_REC,
                        W_REC, 10, pairs.data_ptr() + pos // W_REC * 16, s,
                        idx_base=pos // W_REC)
                pos = off + ln
            out = sort_records(total, W_REC, key_bytes=10, pairs=pairs,
                               pairs_filled=True, segments=segs)
            torch.cuda.synchronize()
            done = pairs[:2 * N_REC].cpu().numpy().copy()
        else:
            out = sort_records(total, W_REC, key_bytes=10, segments=segs)
            torch.cuda.synchronize()
        lo, hi = hint.data_ptr(), hint.data_ptr() + hint.numel()
        return dict(
            segs=segs, pairs=done, grew=grew, sorted=out.cpu().numpy().copy(),
            arena_is_none=f.arena is None,
            in_hint=[lo <= p and p + c * W_REC <= hi for _a, c, p in segs],
            hint_untouched=bool((hint == FILL).all().item()),
            n_views=len(views),
            n_device_views=sum(isinstance(v, DeviceView) for v in views),
            fused_bytes=sum(ln for _off, ln in f.pair_ranges()))
    finally:
        mgr.stop()
        driver.stop()


@pytest.fixture(scope="module")
def off_lane(tmp_path_factory):
    """The switch off: the reference for the other modes."""
    r = _shuffle_once(tmp_path_factory.mktemp("off"), "off",
                      N_REC * W_REC + 4096)
    assert not r["grew"] and r["fused_bytes"] == 0
    arr = _mk_records(np.random.default_rng(21), N_REC, W_REC)
    prefix = arr[:, :8].copy().view("<u8").ravel()
    lo = arr[:, 8:10].copy().view("<u2").ravel()
    want = arr[np.lexsort((lo, prefix))].reshape(-1)   # 80-bit keys distinct
    assert np.array_equal(r["sorted"], want)
    return r


def _covers_once(segs):
    pos = 0
    for first, cnt, _ptr in segs:
        assert first == pos and cnt > 0
        pos += cnt
    assert pos == N_REC


@pytest.mark.parametrize("mode", ["inplace", "local", "off"])
def test_fetcher_in_place(tmp_path, off_lane, mode):
    r = (off_lane if mode == "off" else
         _shuffle_once(tmp_path, mode, N_REC * W_REC + 4096))
    assert not r["grew"]
    _covers_once(r["segs"])
    if mode == "inplace":
        assert not any(r["in_hint"]), "a segment lies in the hint buffer"
        assert r["hint_untouched"], "something was copied into the arena"
        assert r["arena_is_none"]
        assert r["n_device_views"] == r["n_views"]
        assert r["fused_bytes"] == N_REC * W_REC
    else:
        assert all(r["in_hint"]) and len(r["segs"]) == 1
        assert not r["arena_is_none"] and r["n_device_views"] == 0
        assert not r["hint_untouched"]
    assert np.array_equal(r["pairs"], off_lane["pairs"])
    assert np.array_equal(r["sorted"], off_lane["sorted"])


def test_fetcher_in_place_undersized_hint(tmp_path, off_lane):
    r = _shuffle_once(tmp_path, "inplace", 2 * (N_REC * W_REC // R_PARTS))
    assert r["grew"], "the undersized hint should have forced growth"
    _covers_once(r["segs"])
    # fetches deferred to the grown arena land behind the others, so the
    # virtual arena is a permutation of the off lane's; sorted bytes agree
    assert np.array_equal(r["sorted"], off_lane["sorted"])


# ---------------------------------------------------------------------------
# TeraSort


def _terasort(tmp_path, mode, steps=1, **kw):
    from sparkrdma_amd.conf import ShuffleConf
    from sparkrdma_amd.engine import Engine
    from sparkrdma_amd.workloads.terasort import TeraSort
    d = tmp_path / f"{mode}{len(kw)}"
    d.mkdir()
    conf = ShuffleConf(shm_dir=str(d), transport="ipc",
                       hbm_pool_size=1 << 30,
                       shuffle_write_block_size=256 << 10,
                       shuffle_read_block_size=4 << 10,
                       fused_record_fetch=mode)
    eng = Engine(conf, rank=0, world_size=1, driver_port=0)
    try:
        ts = TeraSort(eng, records_per_executor=N_REC,
                      partitions_per_executor=R_PARTS, device="cuda",
                      mode="framework", validate=True,
                      record_bytes=W_REC, seed=3, **kw)
        outs = []
        for _ in range(steps):
            ts.run_step()
            outs.append(ts.last_outputs[0].cpu().numpy().copy())
        return outs
    finally:
        eng.shutdown()


@pytest.mark.parametrize("kw", [{}, {"partitioner": "sampled",
                                     "key_skew": 1.0}],
                         ids=["uniform", "sampled_skewed"])
def test_terasort_inplace_matches_off(tmp_path, kw):
    got = _terasort(tmp_path, "inplace", **kw)[0]
    want = _terasort(tmp_path, "off", **kw)[0]
    assert got.size == N_REC * W_REC
    assert np.array_equal(got, want)


def test_terasort_two_steps_reuse_blocks(tmp_path):
    """The second step's blocks reuse the slab ranges the first step's
    in-place segments pointed into (released by unregister_shuffle)."""
    a, b = _terasort(tmp_path, "inplace", steps=2)
    assert a.size == N_REC * W_REC
    assert np.array_equal(a, b)
