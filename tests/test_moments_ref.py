"""CPU: tests/moments_ref.py, the numpy reference of the patch moments, against the definition itself.

The vectorised reference is compared with a plain double loop over the patch on small cases, all four weights, both edge
modes, patches that leave the frame; the empty box; the sums beyond 64-bit floats' exact range stay exact (Python ints);
and moving a patch over a fixed image does not move the centroid in frame coordinates.
"""
from fractions import Fraction

import numpy as np
import pytest

import moments_ref as mr
import patch_ref as pr


@pytest.mark.parametrize("weight", (mr.COUNT, mr.VALUE, mr.ABOVE, mr.BELOW))
@pytest.mark.parametrize("dtype,top", ((np.uint8, 255), (np.uint16, 65535)))
def test_vectorised_equals_double_loop(weight, dtype, top):
    rng = np.random.default_rng(weight * 7 + top)
    W, H = 23, 17
    img = rng.integers(0, top + 1, size=(H, W)).astype(dtype)
    bands = [(0, top), (top // 4, 3 * top // 4), (top // 2, top // 2 - 1), (int(img[3, 4]), int(img[3, 4])), (top, top), (0, 0)]
    for pw, ph in ((1, 1), (5, 4), (9, 9), (23, 17), (30, 20)):
        for x, y in ((0, 0), (3, 2), (-2, -3), (W - 2, H - 1), (W, 0), (-pw, -ph), (2 ** 31 - 1, -2 ** 31), (7, 5)):
            for lo, hi in bands:
                for mode in (pr.FILL, pr.CLAMP):
                    if mode == pr.CLAMP and (pw > W or ph > H):
                        continue
                    a = mr.moments(img, W, H, pw, ph, x, y, mode, lo, hi, weight)
                    b = mr.moments_loops(img, W, H, pw, ph, x, y, mode, lo, hi, weight)
                    assert a == b, (pw, ph, x, y, lo, hi, mode)
                    assert all(type(v) is int for v in a[0])


def test_empty_selection_and_empty_box():
    img = np.full((10, 12), 7, np.uint8)
    for lo, hi in ((8, 255), (0, 6), (9, 3)):
        m, box, used = mr.moments(img, 12, 10, 5, 4, 2, 3, pr.CLAMP, lo, hi, mr.VALUE)
        assert m == [0] * 8 and box == (5, 4, -1, -1) and used == (2, 3)
    m, box, used = mr.moments(img, 12, 10, 5, 4, 40, 3, pr.FILL, 0, 255, mr.COUNT)   # wholly outside the frame
    assert m == [0] * 8 and box == (5, 4, -1, -1) and used == (40, 3)
    m, box, _ = mr.moments(img, 12, 10, 5, 4, 10, 8, pr.FILL, 0, 255, mr.COUNT)      # a 2 x 2 corner inside
    assert m[0] == 4 and box == (0, 0, 1, 1)


def test_sums_do_not_overflow():
    """A 505 x 512 patch of all 65535, weight VALUE, the largest sums there are: Syy = 65535 * 505 * sum(i^2) is about
    2^50.4 (far beyond 32 bits; the 2^62 of the header's bound takes 511^2 for every row) and exact."""
    W = H = 512
    img = np.full((H, W), 65535, np.uint16)
    m, box, _ = mr.moments(img, W, H, 505, 512, 0, 0, pr.CLAMP, 0, 65535, mr.VALUE)
    s2 = sum(i * i for i in range(512))
    assert m[6] == 65535 * 505 * s2 and 2 ** 50 < m[6] < 2 ** 63
    assert m[7] == 65535 ** 2 * 505 * 512 and box == (0, 0, 504, 511)
    assert 65535 * 511 ** 2 * 505 * 512 < 2 ** 63   # the header's bound


def test_expected_leaves_rejected_frames_and_dead_patches_untouched():
    img = np.arange(64, dtype=np.uint8).reshape(8, 8)
    org = np.zeros((3, 2, 2), np.int64)
    mom, box, used, live = mr.expected([img, None, img], 8, 8, 4, 4, org, [2, 2, 1], pr.CLAMP, 0, 255, mr.COUNT)
    assert live.tolist() == [[True, True], [False, False], [True, False]]
    assert (mom[1] == mr.UNTOUCHED).all() and (mom[2, 1] == mr.UNTOUCHED).all() and mom[0, 0, 0] == 16
    assert (box[1] == pr.UNTOUCHED_ORIGIN).all() and (used[2, 1] == pr.UNTOUCHED_ORIGIN).all()
    assert np.array([mr.UNTOUCHED], dtype=np.int64).view(np.uint8).tolist() == [0xEE] * 8


@pytest.mark.parametrize("weight", (mr.COUNT, mr.VALUE, mr.ABOVE))
def test_moving_the_patch_does_not_move_the_centroid(weight):
    """A blob well inside every patch: used + (Sx / S, Sy / S) is the same exact fraction wherever the patch sits."""
    rng = np.random.default_rng(3)
    W, H = 60, 50
    img = rng.integers(0, 20, size=(H, W)).astype(np.uint8)
    img[20:27, 25:34] = rng.integers(100, 250, size=(7, 9))
    seen = set()
    for dx in range(-6, 7, 3):
        for dy in range(-5, 6, 5):
            m, _, (ux, uy) = mr.moments(img, W, H, 32, 30, 12 + dx, 8 + dy, pr.FILL, 100, 255, weight)
            seen.add((ux + Fraction(m[2], m[1]), uy + Fraction(m[3], m[1])))
    assert len(seen) == 1
