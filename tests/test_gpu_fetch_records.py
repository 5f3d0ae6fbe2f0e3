"""Fused one-sided fetch of wide records (kernels.hip fetch_records_kernel,
pool.cpp read_records_batch, the fetcher's fused lane), byte for byte: the
kernel only copies and repacks, so there is no tolerance.

Kernel tests: the destination must equal the source, the pairs must equal
both the numpy formula and extract_pairs on the same bytes, the canaries
around the destination and around the pairs must come back untouched, and
the source must be unchanged. Fetcher tests: the fused lane on and off
give the same arena, the same pairs and the same sorted output."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CANARY = 0xA5
PAD = 256                 # canary bytes on each side of every output
SRC_OFF = 4               # source: 4 mod 16
DST_OFF = PAD + 12        # destination: 12 mod 16 -> mutually 8 mod 16
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


class _Run:
    """One (dst, src, size) entry with its buffers and expectations."""

    def __init__(self, rng, n, W, key_bytes, idx_base):
        import torch
        self.n, self.W, self.key_bytes, self.idx_base = n, W, key_bytes, idx_base
        self.arr = rng.integers(0, 256, (n, W), dtype=np.uint8)
        host = np.full(SRC_OFF + n * W + 12, 0x3C, dtype=np.uint8)
        host[SRC_OFF:SRC_OFF + n * W] = self.arr.reshape(-1)
        self.src_host = host
        self.src = torch.from_numpy(host).cuda()
        self.dst = torch.full((DST_OFF + n * W + PAD,), CANARY,
                              dtype=torch.uint8, device="cuda")
        self.pairs = torch.full((PAD + 16 * n + PAD,), CANARY,
                                dtype=torch.uint8, device="cuda")
        assert self.src.data_ptr() % 16 == 0 and self.dst.data_ptr() % 16 == 0
        assert self.pairs.data_ptr() % 16 == 0

    @property
    def entry(self):
        return (self.dst.data_ptr() + DST_OFF, self.src.data_ptr() + SRC_OFF,
                self.n * self.W, self.pairs.data_ptr() + PAD, self.idx_base)

    def check(self, hs):
        import torch
        n, W = self.n, self.W
        dst = self.dst.cpu().numpy()
        assert np.array_equal(dst[DST_OFF:DST_OFF + n * W],
                              self.arr.reshape(-1)), "destination != source"
        assert np.all(dst[:DST_OFF] == CANARY), "canary before destination"
        assert np.all(dst[DST_OFF + n * W:] == CANARY), \
            "canary after destination"
        pr = self.pairs.cpu().numpy()
        assert np.all(pr[:PAD] == CANARY), "canary before pairs"
        assert np.all(pr[PAD + 16 * n:] == CANARY), "canary after pairs"
        got = pr[PAD:PAD + 16 * n].copy().view("<u8").reshape(n, 2)
        want = _want_pairs(self.arr, self.key_bytes, self.idx_base)
        assert np.array_equal(got, want), "pairs != numpy formula"
        ref = torch.empty(2 * n, dtype=torch.int64, device="cuda")
        hs.extract_pairs(self.src.data_ptr() + SRC_OFF, n, W, self.key_bytes,
                         ref.data_ptr(), _stream(), idx_base=self.idx_base)
        torch.cuda.synchronize()
        assert np.array_equal(
            got, ref.cpu().numpy().view(np.uint64).reshape(n, 2)), \
            "pairs != extract_pairs"
        assert np.array_equal(self.src.cpu().numpy(), self.src_host), \
            "source modified"


def _fetch(hs, runs):
    import torch
    torch.cuda.synchronize()          # buffers filled on torch's stream
    e = [r.entry for r in runs]
    ev = hs.read_records_batch(
        0, [x[0] for x in e], [x[1] for x in e], [x[2] for x in e],
        runs[0].W, runs[0].key_bytes, [x[3] for x in e], [x[4] for x in e])
    hs.wait_event(ev)


@pytest.mark.parametrize("W,key_bytes", [
    (8, 8), (12, 8), (12, 10), (100, 8), (100, 10), (104, 8), (104, 10),
    (256, 8), (256, 10)])
def test_fetch_records_vs_oracles(hs, W, key_bytes):
    T = hs.fetch_block_records(W)     # records per block of the kernel
    assert T == min(1024, max(1, 4096 // (W // 4)))
    rng = np.random.default_rng(W * 16 + key_bytes)
    for n in (1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17):
        for idx_base in IDX_BASES:
            run = _Run(rng, n, W, key_bytes, idx_base)
            _fetch(hs, [run])
            run.check(hs)


def test_three_entries_one_event(hs):
    """Three (dst, src, size) entries in a single call, one of a single
    record, behind one completion event."""
    W = 100
    T = hs.fetch_block_records(W)
    rng = np.random.default_rng(5)
    runs = [_Run(rng, T + 3, W, 10, 37), _Run(rng, 1, W, 10, (1 << 40) + 37),
            _Run(rng, 200, W, 10, 5000)]
    _fetch(hs, runs)
    for run in runs:
        run.check(hs)


def test_rejects_partial_records(hs):
    rng = np.random.default_rng(6)
    run = _Run(rng, 4, 100, 10, 0)
    d, s, size, p, b = run.entry
    with pytest.raises(RuntimeError):
        hs.read_records_batch(0, [d], [s], [size - 4], 100, 10, [p], [b])


# ---------------------------------------------------------------------------
# fetcher: fused lane on / off

W_REC, N_REC, R_PARTS = 100, 5000, 8


def _mk_records(rng, n, W):
    arr = rng.integers(0, 256, (n, W), dtype=np.uint8)
    # a run of equal prefixes, so the 16 low key bits decide some orders;
    # they are distinct, so the sorted output does not depend on the order
    # in which the fetches were laid out in the arena
    tied = np.arange(1, 141, 7)     # 20 records: a run the tie repair handles
    arr[tied, :8] = arr[0, :8]
    arr[tied, 8:10] = tied.astype("<u2").view(np.uint8).reshape(-1, 2)
    return arr


def _shuffle_once(tmp_path, mode, arena_bytes, spec_W=W_REC):
    """Write N_REC records through a world-1 manager, fetch them back with
    a record spec under conf.fused_record_fetch = mode. Returns (arena
    bytes, finished pairs or None, fused ranges, arena grew?, sentinel
    pairs untouched?)."""
    import torch
    from sparkrdma_amd.conf import ShuffleConf
    from sparkrdma_amd.driver import Driver
    from sparkrdma_amd.manager import ShuffleManager
    from sparkrdma_amd.ops import load
    from sparkrdma_amd.partitioner import RangePartitioner

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
        hint = torch.zeros(arena_bytes, dtype=torch.uint8, device="cuda")
        pairs = torch.full((2 * (arena_bytes // spec_W) + 16,), -1,
                           dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        reader = mgr.get_reader(handle, 0, R_PARTS - 1, arena=hint,
                                records=(spec_W, 10, pairs))
        nblocks = sum(1 for _ in reader)
        assert nblocks > 1
        f = reader.fetcher
        arena = f.arena
        assert arena.numel() == N_REC * W_REC
        grew = f._arena_buf is not hint
        ranges = f.pair_ranges()
        untouched = bool((pairs == -1).all().item())
        done = None
        if spec_W == W_REC:
            # the consumer's side of the contract, as TeraSort does it
            s = torch.cuda.current_stream().cuda_stream
            if grew:
                done = torch.empty(2 * N_REC, dtype=torch.int64,
                                   device="cuda")
                hs.extract_pairs(arena.data_ptr(), N_REC, W_REC, 10,
                                 done.data_ptr(), s)
            else:
                pos = 0
                for off, ln in ranges + [(arena.numel(), 0)]:
                    if off > pos:
                        hs.extract_pairs(
                            arena.data_ptr() + pos, (off - pos) // W_REC,
                            W_REC, 10, pairs.data_ptr() + pos // W_REC * 16,
                            s, idx_base=pos // W_REC)
                    pos = off + ln
                done = pairs[:2 * N_REC]
            torch.cuda.synchronize()
            done = done.cpu().numpy().copy()
        return arena.cpu().numpy().copy(), done, ranges, grew, untouched
    finally:
        mgr.stop()
        driver.stop()


@pytest.fixture(scope="module")
def plain_lane(tmp_path_factory):
    """The switch off: today's path, the reference for every other case."""
    arena, pairs, ranges, grew, _ = _shuffle_once(
        tmp_path_factory.mktemp("off"), "off", N_REC * W_REC + 4096)
    assert ranges == [] and not grew
    return arena, pairs


def _sorted(arena_np, pairs_np):
    import torch
    from sparkrdma_amd.ops.radix import sort_records
    arena = torch.from_numpy(arena_np).cuda()
    pairs = torch.from_numpy(pairs_np).cuda()
    out = sort_records(arena, W_REC, key_bytes=10, pairs=pairs,
                       pairs_filled=True)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("mode", ["local", "host"])
def test_fetcher_fused_lane_matches_plain(tmp_path, plain_lane, mode):
    arena, pairs, ranges, grew, _ = _shuffle_once(
        tmp_path, mode, N_REC * W_REC + 4096)
    assert not grew
    assert len(ranges) > 1, "several fetches expected"
    assert sum(ln for _off, ln in ranges) == N_REC * W_REC, \
        "every fetch should have taken the fused lane"
    assert np.array_equal(arena, plain_lane[0])
    assert np.array_equal(pairs, plain_lane[1])
    assert np.array_equal(_sorted(arena, pairs), _sorted(*plain_lane))


def test_fetcher_grown_arena_falls_back(tmp_path, plain_lane):
    arena, pairs, _ranges, grew, _ = _shuffle_once(
        tmp_path, "local", 2 * (N_REC * W_REC // R_PARTS))
    assert grew, "the undersized hint should have forced growth"
    # fetches deferred to the grown arena land behind the others, so the
    # arena is a permutation of the plain lane's; the sorted bytes agree
    assert np.array_equal(_sorted(arena, pairs), _sorted(*plain_lane))


def test_fetcher_spec_width_not_dividing(tmp_path, plain_lane):
    """A spec whose W divides no fetch length: every fetch takes the plain
    lane and the pair buffer is never written."""
    arena, _pairs, ranges, grew, untouched = _shuffle_once(
        tmp_path, "local", N_REC * W_REC + 4096, spec_W=4096)
    assert ranges == [] and not grew and untouched
    assert np.array_equal(arena, plain_lane[0])


def test_terasort_switch_on_off_identical(tmp_path):
    """The whole wide TeraSort step, fused lane on against off: identical
    sorted bytes."""
    from sparkrdma_amd.conf import ShuffleConf
    from sparkrdma_amd.engine import Engine
    from sparkrdma_amd.workloads.terasort import TeraSort
    outs = {}
    for mode in ("local", "off"):
        d = tmp_path / mode
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
                          record_bytes=W_REC, seed=3)
            ts.run_step()
            outs[mode] = ts.last_outputs[0].cpu().numpy().copy()
        finally:
            eng.shutdown()
    assert outs["local"].size == N_REC * W_REC
    assert np.array_equal(outs["local"], outs["off"])
