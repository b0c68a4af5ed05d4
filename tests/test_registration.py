"""CPU: dbde_video_cpp_amd.registration's host arithmetic on CPU tensors -- the common window and the origins of
origins_from_shifts, its max_shift form, the empty window, and shifts_from_centres' rounding.  No GPU, no codec."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dbde_video_cpp_amd import registration as reg   # noqa: E402


def inside(origins, W, H, rw, rh):
    o = origins.numpy()
    return (o[:, 0] >= 0).all() and (o[:, 0] <= W - rw).all() and (o[:, 1] >= 0).all() and (o[:, 1] <= H - rh).all()


def test_common_window_from_the_extrema():
    W, H = 77, 45
    shifts = np.array([(0, 0), (-3, 5), (4, -2), (1, 1)], np.int64)
    origins, rw, rh, at = reg.origins_from_shifts(shifts, W, H)
    assert at == (3, 2) and (rw, rh) == (W - 4 - 3, H - 5 - 2)
    assert origins.dtype == torch.int32 and origins.is_contiguous() and tuple(origins.shape) == (4, 2)
    assert origins.tolist() == [[3, 2], [0, 7], [7, 0], [4, 3]]
    assert inside(origins, W, H, rw, rh)
    # the defining property on one image: registered[Y][X] = frame[Y + dy][X + dx]
    rng = np.random.default_rng(5)
    template = rng.integers(0, 255, (H + 20, W + 20))
    for (dx, dy), (ox, oy) in zip(shifts, origins.tolist()):
        frame = template[10 - dy:10 - dy + H, 10 - dx:10 - dx + W]     # the template seen dx, dy further on
        assert np.array_equal(frame[oy:oy + rh, ox:ox + rw], template[10 + at[1]:10 + at[1] + rh, 10 + at[0]:10 + at[0] + rw])


def test_one_sided_and_zero_shifts():
    origins, rw, rh, at = reg.origins_from_shifts(torch.zeros((3, 2), dtype=torch.int32), 64, 48)
    assert (rw, rh, at) == (64, 48, (0, 0)) and not origins.any()
    origins, rw, rh, at = reg.origins_from_shifts([(2, 3), (5, 1)], 64, 48)       # only positive: X0 = Y0 = 0
    assert (rw, rh, at) == (59, 45, (0, 0)) and origins.tolist() == [[2, 3], [5, 1]]
    origins, rw, rh, at = reg.origins_from_shifts([(-2, -3), (-5, -1)], 64, 48)   # only negative
    assert (rw, rh, at) == (59, 45, (5, 3)) and origins.tolist() == [[3, 0], [0, 2]]
    origins, rw, rh, at = reg.origins_from_shifts(np.zeros((0, 2), np.int64), 64, 48)
    assert (rw, rh, at) == (64, 48, (0, 0)) and tuple(origins.shape) == (0, 2)


def test_random_shifts_stay_inside():
    rng = np.random.default_rng(11)
    for _ in range(20):
        W, H = int(rng.integers(40, 300)), int(rng.integers(40, 300))
        shifts = rng.integers(-16, 17, (50, 2))
        origins, rw, rh, at = reg.origins_from_shifts(shifts, W, H)
        assert inside(origins, W, H, rw, rh)
        assert rw == W - (max(0, shifts[:, 0].max()) + max(0, -shifts[:, 0].min()))
        assert rh == H - (max(0, shifts[:, 1].max()) + max(0, -shifts[:, 1].min()))
        o = origins.numpy()
        assert (o[:, 0] == rw - rw + at[0] + shifts[:, 0]).all() and (o[:, 1] == at[1] + shifts[:, 1]).all()
        assert o[:, 0].min() == 0 or shifts[:, 0].min() >= 0
        assert o[:, 0].max() == W - rw or shifts[:, 0].max() <= 0


def test_max_shift_fixes_the_window_without_looking():
    shifts = [(0, 0), (-16, 16), (40, -3)]            # the last one moved further than max_shift
    origins, rw, rh, at = reg.origins_from_shifts(shifts, 100, 80, max_shift=16)
    assert (rw, rh, at) == (68, 48, (16, 16))
    assert origins.tolist() == [[16, 16], [0, 32], [56, 13]]       # 56 > W - rw = 32: the kernel clamps it
    assert inside(origins[:2], 100, 80, rw, rh) and not inside(origins, 100, 80, rw, rh)
    assert reg.origins_from_shifts(shifts, 100, 80, max_shift=0)[1:3] == (100, 80)
    with pytest.raises(ValueError):
        reg.origins_from_shifts(shifts, 100, 80, max_shift=-1)


def test_empty_window_and_bad_shifts_raise():
    with pytest.raises(ValueError):
        reg.origins_from_shifts([(0, 0), (64, 0)], 64, 48)             # rw = 0
    with pytest.raises(ValueError):
        reg.origins_from_shifts([(0, -24), (0, 24)], 64, 48)           # rh = 0
    assert reg.origins_from_shifts([(0, -24), (0, 23)], 64, 48)[2] == 1
    with pytest.raises(ValueError):
        reg.origins_from_shifts([(0, 0)], 64, 48, max_shift=24)        # [24, 24) in y
    with pytest.raises(ValueError):
        reg.origins_from_shifts([(0.5, 0.0)], 64, 48)                  # not integers
    with pytest.raises(ValueError):
        reg.origins_from_shifts([0, 1, 2], 64, 48)                     # not (n, 2)


def test_shifts_from_centres_rounds_the_mean_to_nearest():
    c = torch.tensor([[[10.0, 20.0], [30.0, 40.0]],
                      [[10.4, 20.0], [30.4, 41.0]],        # mean + (0.4, 0.5) -> (0, 1): halves up
                      [[8.0, 17.0], [29.0, 37.9]],         # mean + (-1.5, -2.55) -> (-1, -3)
                      [[12.6, 20.0], [32.6, 40.0]]],       # mean + (2.6, 0) -> (3, 0)
                     dtype=torch.float64)
    s = reg.shifts_from_centres(c)
    assert s.dtype == torch.int64 and s.tolist() == [[0, 0], [0, 1], [-1, -3], [3, 0]]
    assert reg.shifts_from_centres(c, reference=(21.0, 31.0)).tolist() == [[-1, -1], [-1, 0], [-2, -4], [2, -1]]
    assert reg.shifts_from_centres(c[:, :1]).tolist() == [[0, 0], [0, 0], [-2, -3], [3, 0]]
    assert tuple(reg.shifts_from_centres(torch.zeros((0, 3, 2))).shape) == (0, 2)
    with pytest.raises(ValueError):
        reg.shifts_from_centres(torch.zeros((4, 2)))
    # the two halves of the chain agree: the shifts give origins inside the frame
    origins, rw, rh, at = reg.origins_from_shifts(s, 64, 48)
    assert inside(origins, 64, 48, rw, rh) and (rw, rh, at) == (64 - 4, 48 - 4, (1, 3))
