"""CPU: the numpy reference of the grouped projections (tests/gproject_ref.py) on hand-worked cases."""
import numpy as np
import pytest

from gproject_ref import group_ranges, reduce_groups


def test_uniform_groups_and_the_ragged_last_one():
    assert group_ranges(13, group_frames=4) == [(0, 4), (4, 8), (8, 12), (12, 13)]
    assert group_ranges(13, group_frames=13) == [(0, 13)]
    assert group_ranges(13, group_frames=16) == [(0, 13)]
    assert group_ranges(13, group_frames=1) == [(k, k + 1) for k in range(13)]
    assert group_ranges(0, group_frames=3) == []


def test_ragged_groups_are_clamped():
    n = 13
    assert group_ranges(n, starts=[0, n]) == [(0, 13)]
    assert group_ranges(n, starts=[0, 0, 5, 5, n]) == [(0, 0), (0, 5), (5, 5), (5, 13)]           # empty groups
    assert group_ranges(n, starts=[3, 9]) == [(3, 9)]                                            # unused frames
    assert group_ranges(n, starts=[0, 10, 5, n + 7]) == [(0, 10), (10, 10), (5, 13)]              # decreasing, above n
    assert group_ranges(n, starts=[20, 30, 2 ** 32 - 1]) == [(13, 13), (13, 13)]                  # entries above n
    assert group_ranges(n, starts=[0, 8, 4, 12]) == [(0, 8), (8, 8), (4, 12)]                     # overlapping ranges
    assert group_ranges(0, starts=[0, 5]) == [(0, 0)]


def test_exactly_one_form():
    with pytest.raises(ValueError):
        group_ranges(5)
    with pytest.raises(ValueError):
        group_ranges(5, group_frames=2, starts=[0, 5])
    with pytest.raises(ValueError):
        group_ranges(5, starts=[0])


def test_reductions_by_hand():
    # 5 frames of 2x3: frame f is f + 10 * column + 100 * row; frame 3 rejected
    frames = [np.array([[f, f + 10, f + 20], [f + 100, f + 110, f + 120]], np.uint8) for f in range(5)]
    frames[3] = None
    got = reduce_groups(frames, group_ranges(5, group_frames=2), 1, 0, 2, 2)
    assert got["counts"].tolist() == [2, 1, 1]
    assert got["max"][0].tolist() == [[11, 21], [111, 121]] and got["min"][0].tolist() == [[10, 20], [110, 120]]
    assert got["sum"][0].tolist() == [[21, 41], [221, 241]]
    assert got["sumsq"][0].tolist() == [[10 * 10 + 11 * 11, 20 * 20 + 21 * 21], [110 ** 2 + 111 ** 2, 120 ** 2 + 121 ** 2]]
    assert got["sum"][1].tolist() == [[12, 22], [112, 122]]          # frame 2 alone
    assert got["max"][2].tolist() == [[14, 24], [114, 124]]          # the last, shorter group: frame 4
    # a wholly rejected group and an empty one: the empty projection
    got = reduce_groups(frames, group_ranges(5, starts=[3, 4, 4, 9]), 0, 0, 3, 2)
    assert got["counts"].tolist() == [0, 0, 1]
    for k in (0, 1):
        assert (got["max"][k] == 0).all() and (got["min"][k] == 255).all()
        assert (got["sum"][k] == 0).all() and (got["sumsq"][k] == 0).all()
    assert got["sum"][2].tolist() == [[4, 14, 24], [104, 114, 124]]


def test_reductions_16_bit():
    frames = [np.full((2, 2), v, np.uint16) for v in (65535, 1, 65535)]
    got = reduce_groups(frames, group_ranges(3, starts=[0, 3, 1, 1]), 0, 0, 2, 2, pix=2)
    assert got["counts"].tolist() == [3, 0, 0]
    assert (got["sum"][0] == 2 * 65535 + 1).all() and (got["sumsq"][0] == 2 * 65535 ** 2 + 1).all()
    assert (got["min"][1] == 65535).all() and (got["max"][1] == 0).all()
    assert (got["min"][0] == 1).all()
