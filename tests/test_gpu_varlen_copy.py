"""varlen_copy_kernel (ops/csrc/varlen.hip) alone, against a numpy byte
loop. Every destination range lies between 64 guard bytes of a fixed pattern
on either side, and the whole destination buffer — ranges, guards, gaps —
is compared after every copy: a store outside a range fails the test."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 64
PATTERN = 0xA5


@pytest.fixture(scope="module")
def mod():
    from sparkrdma_amd.ops import load
    return load()


@pytest.fixture(scope="module")
def T(mod):
    return mod.varlen_copy_tile_bytes()


@pytest.fixture(scope="module")
def L(mod):
    return mod.varlen_copy_lds_rows()


def _i64(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).cuda()


def run_copy(lens, seg_first, dst_align=(0,), src_align=None, seed=0,
             wide_loads=True):
    """Copy rows of ``lens`` bytes (row r's source at alignment
    ``src_align[r % len]``, default r % 16) into ranges
    ``[seg_first[s], seg_first[s + 1])`` at destination alignment
    ``dst_align[s % len]`` and compare with the byte loop."""
    from sparkrdma_amd.ops.varlen import exclusive_scan, varlen_copy
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int64)
    n = len(lens)
    seg_first = np.asarray(seg_first, dtype=np.int64)
    S = len(seg_first) - 1
    # sources: row r at the next address with the wanted alignment
    src_off = np.zeros(n, dtype=np.int64)
    pos = 0
    for r in range(n):
        want = (src_align[r % len(src_align)] if src_align is not None
                else r % 16)
        pos += (want - pos) % 16
        src_off[r] = pos
        pos += int(lens[r])
    src_np = rng.integers(0, 256, pos + 16, dtype=np.uint8)
    cum_np = np.concatenate([[0], np.cumsum(lens)])
    # destinations: guard | range | guard, each range at its alignment
    dst_off = np.zeros(S, dtype=np.int64)
    pos = 0
    for s in range(S):
        pos += GUARD
        pos += (dst_align[s % len(dst_align)] - pos) % 16
        dst_off[s] = pos
        pos += int(cum_np[seg_first[s + 1]] - cum_np[seg_first[s]]) + GUARD
    want = np.full(pos + 16, PATTERN, dtype=np.uint8)
    for s in range(S):                          # the byte loop
        at = int(dst_off[s])
        for r in range(seg_first[s], seg_first[s + 1]):
            for b in range(int(lens[r])):
                want[at] = src_np[src_off[r] + b]
                at += 1
    src = torch.from_numpy(src_np).cuda()
    dst = torch.full((len(want),), PATTERN, dtype=torch.uint8, device="cuda")
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    cum = exclusive_scan(_i64(lens))
    assert cum.cpu().tolist() == cum_np.tolist()
    copied = varlen_copy(cum, _i64(src_off) + src.data_ptr(),
                         _i64(seg_first), _i64(dst_off) + dst.data_ptr(),
                         total=int(cum_np[-1]), wide_loads=wide_loads)
    torch.cuda.synchronize()
    assert copied == int(cum_np[-1])
    got = dst.cpu().numpy()
    diff = np.nonzero(got != want)[0]
    assert len(diff) == 0, (f"{len(diff)} bytes differ, first at "
                            f"{diff[:8].tolist()} of {len(want)}")


def test_constants_match_the_wrapper(mod):
    from sparkrdma_amd.ops import varlen
    assert varlen.TILE_BYTES == mod.varlen_copy_tile_bytes()
    assert varlen.LDS_ROWS == mod.varlen_copy_lds_rows()


def _cycle_rows():
    """Every length 0..40 at every source alignment 0..15, three times
    over: 1968 rows, about 39 KB — more than one tile."""
    lens, aligns = [], []
    for _rep in range(3):
        for ln in range(41):
            for al in range(16):
                lens.append(ln)
                aligns.append(al)
    return lens, aligns


@pytest.mark.parametrize("wide_loads", [True, False])
def test_every_length_and_source_alignment(wide_loads):
    lens, aligns = _cycle_rows()
    run_copy(lens, [0, 900, len(lens)], dst_align=(0,), src_align=aligns,
             wide_loads=wide_loads)


@pytest.mark.parametrize("dst_align", [1, 8, 15])
def test_every_length_and_source_alignment_unaligned_dst(dst_align):
    lens, aligns = _cycle_rows()
    run_copy(lens, [0, 900, len(lens)], dst_align=(dst_align, 16 - dst_align),
             src_align=aligns)


def test_index_slab_row_in_front():
    """One range: a long aligned slab row of 16 + 16 n bytes, then the n
    payload rows — the shape of one partition's segment."""
    lens, aligns = _cycle_rows()
    n = len(lens)
    run_copy([16 + 16 * n] + lens, [0, n + 1], dst_align=(0,),
             src_align=[0] + aligns)


@pytest.mark.parametrize("dst_align", [0, 5])
def test_one_row_longer_than_three_tiles(T, dst_align):
    run_copy([3 * T + 5], [0, 1], dst_align=(dst_align,), src_align=[3])


@pytest.mark.parametrize("dst_align", [0, 11])
def test_rows_ending_on_tile_edges(T, dst_align):
    # ends at T, 2T - 1, 3T: on an edge, one short of it, and on it again
    run_copy([T, T - 1, T + 1, 9], [0, 4], dst_align=(dst_align,))
    run_copy([T, T - 1, T + 1, 9], [0, 1, 2, 3, 4],
             dst_align=(dst_align, 3, 0, 9))


@pytest.mark.parametrize("wide_loads", [True, False])
def test_more_one_byte_rows_than_the_lds_window(L, wide_loads):
    run_copy([1] * (L + 100), [0, L + 100], dst_align=(7,),
             wide_loads=wide_loads)


@pytest.mark.parametrize("back", [14, 10, 7, 3])
def test_zero_length_run_across_a_tile_edge(T, L, back):
    """3 L rows of length 0 between two rows of 7 bytes; the first of the
    two ends ``back - 7`` bytes before the edge of the first tile (0: the
    run sits on the edge; negative: the row itself straddles it)."""
    lens = [T - back, 7] + [0] * (3 * L) + [7, 40]
    run_copy(lens, [0, len(lens)], dst_align=(0,))
    run_copy(lens, [0, 2, len(lens)], dst_align=(2, 13))


def test_all_rows_empty():
    run_copy([0] * 100, [0, 40, 100], dst_align=(0, 3))
    run_copy([], [0], dst_align=())


def test_many_short_and_empty_ranges():
    rng = np.random.default_rng(7)
    lens, first = [], [0]
    for s in range(300):
        kind = s % 5
        if kind == 0:
            rows = []                                   # empty range
        elif kind == 1:
            rows = [0, 0]                               # rows, but no byte
        elif kind in (2, 3):
            total = 1 + (s // 5) % 15                   # 1..15 bytes
            a = int(rng.integers(0, total + 1))
            rows = [a, 0, total - a]
        else:
            rows = [int(x) for x in rng.integers(0, 400, 5)]
        lens += rows
        first.append(len(lens))
    run_copy(lens, first, dst_align=tuple(range(16)) + (5, 0, 11))


def test_wrapper_rejects_bad_tables(mod):
    cum = _i64([0, 8])
    src = _i64([cum.data_ptr()])
    seg_off = _i64([0, 8])
    dst_buf = torch.zeros(64, dtype=torch.uint8, device="cuda")
    seg_dst = _i64([dst_buf.data_ptr()])
    ok = [cum.data_ptr(), src.data_ptr(), 1, seg_off.data_ptr(),
          seg_dst.data_ptr(), 1, 8]
    for slot in (0, 1, 3, 4):
        args = list(ok)
        args[slot] = 0
        with pytest.raises(ValueError, match="null"):
            mod.varlen_copy(*args)
        args[slot] = ok[slot] + 4
        with pytest.raises(ValueError, match="misaligned"):
            mod.varlen_copy(*args)
    args = list(ok)
    args[2] = 1 << 31
    with pytest.raises(ValueError, match="row count"):
        mod.varlen_copy(*args)
    args = list(ok)
    args[5] = 1 << 31
    with pytest.raises(ValueError, match="range count"):
        mod.varlen_copy(*args)
    args = list(ok)
    args[6] = (1 << 31) * mod.varlen_copy_tile_bytes()
    with pytest.raises(ValueError, match="grid"):
        mod.varlen_copy(*args)
    torch.cuda.synchronize()
    assert int(dst_buf.sum()) == 0                      # nothing ran


def test_python_wrapper_checks_shapes():
    from sparkrdma_amd.ops.varlen import varlen_copy
    cum, src = _i64([0, 8]), _i64([0])
    first, dst = _i64([0, 1]), _i64([0])
    with pytest.raises(ValueError):
        varlen_copy(cum[:1], src, first, dst, total=8)
    with pytest.raises(ValueError):
        varlen_copy(cum, src, first, _i64([0, 0]), total=8)
    with pytest.raises(ValueError):
        varlen_copy(cum.to(torch.int32), src, first, dst, total=8)
    with pytest.raises(ValueError):
        varlen_copy(cum.cpu(), src, first, dst, total=8)
