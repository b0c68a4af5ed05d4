"""CPU: tests/patch_ref.py, the numpy reference the GPU patch tests compare with.

In CLAMP mode a patch is the crop tests/test_gpu_roi.py's check_windows compares decode_roi with (the origin clamped
into [0, W-pw] x [0, H-ph]); FILL mode is checked on hand-written cases.
"""
import numpy as np

import patch_ref as pr
from test_gpu_roi import clamp

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def image(W, H, dtype=np.uint8):
    return (np.arange(W * H).reshape(H, W) * 7 % 251 + 1).astype(dtype)   # never 0: the fill below is


def test_clamp_is_check_windows_crop():
    W, H = 37, 23
    img = image(W, H)
    rng = np.random.default_rng(1)
    for pw, ph in ((1, 1), (8, 8), (9, 5), (37, 23), (36, 1)):
        for _ in range(50):
            x, y = int(rng.integers(-50, W + 50)), int(rng.integers(-50, H + 50))
            got, used = pr.patch(img, W, H, pw, ph, x, y, pr.CLAMP)
            ox, oy = clamp(x, 0, W - pw), clamp(y, 0, H - ph)
            assert used == (ox, oy)
            assert np.array_equal(got, img[oy:oy + ph, ox:ox + pw])
    got, used = pr.patch(img, W, H, 8, 8, I32_MIN, I32_MAX, pr.CLAMP)
    assert used == (0, H - 8) and np.array_equal(got, img[H - 8:, :8])


def test_fill_hand_written():
    W, H = 5, 4
    img = image(W, H)
    # negative origin: the top-left 2 x 1 of the frame lands at the bottom-right of a 3 x 3 patch
    got, used = pr.patch(img, W, H, 3, 3, -1, -2, pr.FILL, 0)
    assert used == (-1, -2)
    assert np.array_equal(got, [[0, 0, 0], [0, 0, 0], [0, img[0, 0], img[0, 1]]])
    # across the right and bottom edges
    got, _ = pr.patch(img, W, H, 2, 3, 4, 2, pr.FILL, 9)
    assert np.array_equal(got, [[img[2, 4], 9], [img[3, 4], 9], [9, 9]])
    # wholly outside, on every side and at the ends of int32
    for x, y in ((-3, 0), (5, 0), (0, -3), (0, 4), (I32_MIN, I32_MAX), (I32_MAX, I32_MIN), (I32_MAX, 0), (0, I32_MIN)):
        got, used = pr.patch(img, W, H, 3, 3, x, y, pr.FILL, 200)
        assert (got == 200).all() and used == (x, y)
    # one pixel inside
    got, _ = pr.patch(img, W, H, 3, 3, -2, -2, pr.FILL, 0)
    assert got[2, 2] == img[0, 0] and np.count_nonzero(got) == 1
    # pw > W and ph > H: the whole frame inside the patch
    got, _ = pr.patch(img, W, H, 9, 6, -2, -1, pr.FILL, 0)
    want = np.zeros((6, 9), np.uint8)
    want[1:5, 2:7] = img
    assert np.array_equal(got, want)
    # inside the frame FILL and CLAMP agree
    assert np.array_equal(pr.patch(img, W, H, 3, 2, 1, 1, pr.FILL, 0)[0], pr.patch(img, W, H, 3, 2, 1, 1, pr.CLAMP)[0])


def test_expected_counts_rejected_frames_and_used():
    W, H = 16, 9
    frames = [image(W, H, np.uint16), None, image(W, H, np.uint16) + 1]
    org = np.array([[(0, 0), (20, 20), (-1, -1)]] * 3)
    out, used, live = pr.expected(frames, W, H, 4, 4, org, counts=[2, 3, 7], mode=pr.CLAMP, untouched=0xEEEE, dtype=np.uint16)
    assert live.tolist() == [[True, True, False], [False] * 3, [True] * 3]
    assert (out[0, 2] == 0xEEEE).all() and (out[1] == 0xEEEE).all()
    assert (used[0, 2] == pr.UNTOUCHED_ORIGIN).all() and (used[1] == pr.UNTOUCHED_ORIGIN).all()
    assert used[0, 1].tolist() == [12, 5] and used[2, 2].tolist() == [0, 0]
    assert np.array_equal(out[2, 1], frames[2][5:9, 12:16])
    _, used, _ = pr.expected(frames, W, H, 4, 4, org, mode=pr.FILL, fill=3, untouched=0xEEEE, dtype=np.uint16)
    assert used[0].tolist() == [[0, 0], [20, 20], [-1, -1]]
    assert np.array([pr.UNTOUCHED_ORIGIN], np.int32).view(np.uint8).tolist() == [0xEE] * 4
