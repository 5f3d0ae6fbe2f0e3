"""The segment table of an in-place reader (reader.build_record_segments,
reader.DeviceView) and the conf value that switches it on. No GPU."""

import pytest

from sparkrdma_amd.conf import ConfError, ShuffleConf
from sparkrdma_amd.reader import DeviceView, build_record_segments

W = 100


def test_sorts_and_merges_contiguous_neighbours():
    a, b = 0x10000, 0x90000
    ranges = [
        (30, 5, b),                  # out of order on purpose
        (0, 10, a),
        (10, 20, a + 10 * W),        # contiguous with the first: merges
        (35, 1, b + 5 * W),          # contiguous with (30, 5): merges
        (36, 4, b + 6 * W + 4),      # 4 bytes off: stays its own segment
    ]
    got = build_record_segments(ranges, W, 40)
    assert got == [(0, 30, a), (30, 6, b), (36, 4, b + 6 * W + 4)]


def test_adjacent_indices_apart_in_address_do_not_merge():
    got = build_record_segments([(0, 3, 5000), (3, 3, 1000)], W)
    assert got == [(0, 3, 5000), (3, 3, 1000)]


def test_empty_ranges_are_dropped():
    got = build_record_segments([(0, 0, 64), (0, 2, 128), (2, 0, 999)], W, 2)
    assert got == [(0, 2, 128)]
    assert build_record_segments([], W, 0) == []


def test_gap_raises():
    with pytest.raises(ValueError, match="no segment"):
        build_record_segments([(0, 10, 0x1000), (11, 5, 0x9000)], W)
    with pytest.raises(ValueError, match="no segment"):
        build_record_segments([(1, 10, 0x1000)], W)       # does not start at 0


def test_overlap_raises():
    with pytest.raises(ValueError, match="two segments"):
        build_record_segments([(0, 10, 0x1000), (9, 5, 0x9000)], W)
    with pytest.raises(ValueError, match="two segments"):
        build_record_segments([(0, 10, 0x1000), (0, 10, 0x1000)], W)


def test_total_is_checked():
    with pytest.raises(ValueError, match="expected 12"):
        build_record_segments([(0, 10, 0x1000)], W, 12)
    with pytest.raises(ValueError):
        build_record_segments([(0, -1, 0x1000)], W)


def test_device_view_slices_without_copying():
    v = DeviceView(0x4000, 1000, 300)
    assert len(v) == v.numel() == 1000 and v.data_ptr() == 0x4000
    s = v[100:400]
    assert (s.ptr, s.length, s.arena_off) == (0x4000 + 100, 300, 400)
    assert (v[900:2000].length, v[900:2000].ptr) == (100, 0x4000 + 900)
    t = s[50:60]
    assert (t.ptr, t.length, t.arena_off) == (0x4000 + 150, 10, 450)
    with pytest.raises(TypeError):
        v[3]
    with pytest.raises(ValueError):
        v[::2]


def test_conf_accepts_inplace_and_refuses_unknown():
    assert ShuffleConf().fused_record_fetch == "inplace"
    for mode in ("inplace", "local", "host", "off"):
        assert ShuffleConf(fused_record_fetch=mode).fused_record_fetch == mode
    assert ShuffleConf.from_dict(
        {"spark.shuffle.rdma.fusedRecordFetch": "local"}
    ).fused_record_fetch == "local"
    with pytest.raises(ConfError, match="inplace"):
        ShuffleConf(fused_record_fetch="in-place")
    with pytest.raises(ConfError):
        ShuffleConf(fused_record_fetch="")
