"""The write path's block layout without a GPU: the greedy grouping policy
against a brute-force statement of it, and the GPU lanes' placement step
over a real BlockPool with made-up slab addresses."""

from types import SimpleNamespace

import numpy as np
import pytest

from sparkrdma_amd.block_pool import BlockPool
from sparkrdma_amd.map_output import MapTaskOutput, make_key
from sparkrdma_amd.writer import ShuffleWriter, _GpuLayout, group_partitions

WRITE_BLOCK = 100


def _policy_cases():
    rng = np.random.default_rng(2024)
    cases = [[7], [0], [0, 0, 0, 0], [60, 40, 1], [10, 250, 10],
             [0, 0, 30, 80, 0, 0], [0, 100, 0], [101], [50, 50, 50, 50]]
    for _ in range(300):
        R = int(rng.integers(1, 41))
        hi = int(rng.choice([3, 40, 120, 300]))
        seg = rng.integers(0, hi, R)
        seg[rng.random(R) < 0.3] = 0
        cases.append(seg.tolist())
    return cases


def test_group_partitions_is_the_greedy_policy():
    for seg in _policy_cases():
        groups = group_partitions(np.array(seg, dtype=np.int64), WRITE_BLOCK)
        # consecutive runs covering 0..R-1 exactly once, none empty
        assert all(groups), seg
        assert [p for g in groups for p in g] == list(range(len(seg))), seg
        sizes = [sum(seg[p] for p in g) for g in groups]
        for g, size in zip(groups, sizes):
            # over the block size only as a single partition
            assert size <= WRITE_BLOCK or len(g) == 1, (seg, g)
        for prev_size, g in zip(sizes, groups[1:]):
            # greedy: the next group's first partition did not fit
            assert prev_size + seg[g[0]] > WRITE_BLOCK, (seg, g)


def test_group_partitions_hand_cases():
    assert group_partitions([60, 40, 1], 100) == [[0, 1], [2]]
    assert group_partitions([10, 250, 10], 100) == [[0], [1], [2]]
    assert group_partitions([0, 0, 0], 100) == [[0, 1, 2]]
    assert group_partitions([5], 100) == [[0]]
    assert group_partitions([], 100) == []


SLAB = 1 << 20
HBM_BASE = 0x7F00_0000_0000       # made-up device addresses, 1 TiB apart
EXECUTOR = 3


class _HostSegment:
    def __init__(self):
        self.buf = bytearray(SLAB)

    def write(self, off, data):
        self.buf[off:off + len(data)] = data


class _StubManager:
    """What the layout step touches: alloc_table, the HBM pool with its
    slab bases, executor_id and the block size for placement; the host
    pool, its segments, keep_alive and publish for the finishing step."""

    def __init__(self, hbm_slabs: int, write_block: int):
        self.executor_id = EXECUTOR
        self.conf = SimpleNamespace(shuffle_write_block_size=write_block)
        self._gpu_slabs = iter(range(0x8000, 0x8000 + 64))
        self.gpu = SimpleNamespace(
            pool=BlockPool(SLAB, hbm_slabs * SLAB,
                           lambda size: next(self._gpu_slabs)),
            local_base=lambda seg_id: HBM_BASE + ((seg_id & 0x7FFF) << 40))
        self.segments = {}
        self.pool = BlockPool(SLAB, 64 * SLAB, self._alloc_host)
        self.kept = self.published = None

    def _alloc_host(self, size):
        seg_id = 16 + len(self.segments)
        self.segments[seg_id] = _HostSegment()
        return seg_id

    def alloc_table(self, num_partitions, shuffle_id=None):
        self.table = MapTaskOutput(num_partitions)
        return self.table, 4096

    def data_segment(self, seg_id):
        return self.segments[seg_id]

    def keep_alive(self, handle, map_id, blocks):
        self.kept = list(blocks)

    def publish_map_output(self, handle, map_id, table_addr):
        self.published = (map_id, table_addr)


def _layout(seg_bytes, nd, hbm_slabs=1, write_block=256 << 10):
    mgr = _StubManager(hbm_slabs, write_block)
    handle = SimpleNamespace(shuffle_id=9, num_partitions=len(seg_bytes))
    writer = ShuffleWriter(mgr, handle, map_id=5)
    return mgr, writer, _GpuLayout(writer, seg_bytes, nd, "cpu")


def _spill_case():
    """R = 18 partitions in nd = 32 digits, 256 KiB blocks, one 1 MiB
    slab. The groups: [0, 1] all empty; [2] oversized (a 512 KiB block);
    [3, 4, 5] and [6] fill the slab; [7], [8, 9, 10], [11..15] and
    [16, 17] must spill. Empty partitions at both ends, inside groups and
    as a group's tail."""
    kib = [0, 0, 300, 120, 0, 80, 200, 200, 100, 0, 100, 57, 0, 0, 0, 0,
           230, 0]
    return np.array(kib, dtype=np.int64) << 10


def test_placement_addresses_and_table():
    """Placement alone: every non-empty partition gets the device address
    its table entry names (HBM) or a slot of the staging tensor
    (spilled); groups are back to back in partition order; empty
    partitions and digits >= R stay 0. The partitions of an all-empty
    group get the (0, 0, meta_key) entry; an empty partition inside a
    placed group keeps, as it always did, the block's key and its running
    offset with length 0."""
    seg = _spill_case()
    R, nd = len(seg), 32
    mgr, writer, lay = _layout(seg, nd)
    groups = group_partitions(seg, mgr.conf.shuffle_write_block_size)
    spilled = [parts for parts, _total in lay.spilled]
    assert spilled == [[7], [8, 9, 10], [11, 12, 13, 14, 15], [16, 17]]
    assert groups[:4] == [[0, 1], [2], [3, 4, 5], [6]]
    stage_lo = lay.stage.data_ptr()
    assert lay.stage.numel() == sum(int(seg[g].sum()) for g in spilled)
    meta_key = make_key(EXECUTOR, 1)
    assert lay.dst.shape == (nd,) and lay.dst.dtype == np.int64
    assert not lay.dst[R:].any()
    stage_next = stage_lo
    for g in groups:
        nonempty = [p for p in g if seg[p]]
        for p in g:
            if not seg[p]:
                assert lay.dst[p] == 0
        if not nonempty:
            for p in g:
                loc = mgr.table.get(p)
                assert (loc.addr, loc.length, loc.key) == (0, 0, meta_key)
            continue
        if g in spilled:
            # staged in spill order, back to back; table filled later
            assert lay.dst[nonempty[0]] == stage_next
            stage_next += int(seg[g].sum())
        else:
            first = mgr.table.get(g[0])
            seg_id = first.key & 0xFFFF
            assert first.key == make_key(EXECUTOR, seg_id)
            for p in g:
                loc = mgr.table.get(p)
                assert (loc.length, loc.key) == (seg[p], first.key)
                assert loc.addr == first.addr + seg[g[0]:p].sum()
                if seg[p]:
                    assert lay.dst[p] == \
                        mgr.gpu.local_base(seg_id) + loc.addr
        for a, b in zip(nonempty, nonempty[1:]):
            assert lay.dst[b] == lay.dst[a] + seg[a:b].sum()
    assert stage_next == stage_lo + lay.stage.numel()
    placed = sum(int(seg[g].sum()) for g in groups if g not in spilled)
    assert writer.metrics.bytes_written == placed
    assert [b.pool for b in lay.blocks] == [mgr.gpu.pool] * len(lay.blocks)


def test_finish_moves_spilled_groups_to_host_blocks(monkeypatch):
    """The finishing step with the device synchronise patched out (there
    is no device here; the staging tensor is host memory): the bytes the
    kernel would have left in the staging tensor arrive in host pool
    blocks at the offsets the table names, and everything is counted."""
    import torch
    monkeypatch.setattr(torch.cuda, "synchronize", lambda: None)
    seg = _spill_case()
    R = len(seg)
    mgr, writer, lay = _layout(seg, 32)
    # stand in for the kernel: partition p's bytes are all p + 1
    stage_lo = lay.stage.data_ptr()
    spilled_parts = [p for parts, _t in lay.spilled for p in parts]
    for p in spilled_parts:
        if seg[p]:
            off = int(lay.dst[p]) - stage_lo
            lay.stage[off:off + int(seg[p])] = p + 1
    n_hbm = len(lay.blocks)
    lay.finish(records=1234)
    assert writer.metrics.bytes_written == seg.sum()
    assert writer.metrics.records_written == 1234
    assert mgr.published == (5, 4096)
    assert mgr.kept == lay.blocks and len(mgr.kept) == n_hbm + len(lay.spilled)
    assert all(b.pool is mgr.pool for b in mgr.kept[n_hbm:])
    for parts, _total in lay.spilled:
        locs = [mgr.table.get(p) for p in parts]
        for p, loc, nxt in zip(parts, locs, locs[1:] + [None]):
            assert loc.length == seg[p]
            seg_id = loc.key & 0xFFFF
            assert loc.key == make_key(EXECUTOR, seg_id)
            if nxt is not None:
                assert nxt.addr == loc.addr + seg[p]
            data = mgr.segments[seg_id].buf[loc.addr:loc.addr + loc.length]
            assert data == bytes([p + 1]) * int(seg[p])
    # the table is complete: every partition's length is its byte count
    assert [mgr.table.get(p).length for p in range(R)] == seg.tolist()


def test_placement_without_pressure_has_no_staging():
    seg = _spill_case()
    mgr, writer, lay = _layout(seg, 32, hbm_slabs=4)
    assert not lay.spilled and lay.stage.numel() == 0
    assert writer.metrics.bytes_written == seg.sum()
    assert np.count_nonzero(lay.dst) == np.count_nonzero(seg)


@pytest.mark.parametrize("seg", [[0, 0, 0], [0, 5 << 20, 0]])
def test_placement_degenerate(seg):
    """All-empty output; one partition larger than a slab (the pool cannot
    serve it at all, so it spills, a group of its own)."""
    seg = np.array(seg, dtype=np.int64)
    mgr, writer, lay = _layout(seg, 16)
    assert [parts for parts, _t in lay.spilled] == \
        ([[1]] if seg.any() else [])
    assert lay.stage.numel() == seg.sum()
    assert (lay.dst != 0).tolist()[:3] == (seg != 0).tolist()
