"""CPU: the two computations of a binned decode's expected planes (tests/binned_ref.py) agree, and Binned.pixels /
Binned.mean() (pure host code) follow the geometry."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import binned_ref as br   # noqa: E402


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_reduceat_equals_the_loop_over_bins(dtype):
    rng = np.random.default_rng(11)
    for _ in range(30):
        W, H = int(rng.integers(1, 70)), int(rng.integers(1, 50))
        img = rng.integers(0, np.iinfo(dtype).max + 1, size=(H, W)).astype(dtype)
        for b in (2, 4, 8):
            x, y = int(rng.integers(0, W)) // b * b, int(rng.integers(0, H)) // b * b
            rw, rh = int(rng.integers(1, W - x + 1)), int(rng.integers(1, H - y + 1))
            a, c = br.binned_reduceat(img, x, y, rw, rh, b), br.binned_loop(img, x, y, rw, rh, b)
            for s in br.STATS:
                assert a[s].shape == br.out_shape(rw, rh, b) and (a[s] == c[s]).all(), (W, H, b, x, y, rw, rh, s)


def test_the_issue_example_shapes_and_corner_bins():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, size=(123, 200)).astype(np.uint8)
    for b, shape, corner in ((2, (57, 96), 1), (4, (29, 48), 3), (8, (15, 24), 7)):
        a, c = br.binned_reduceat(img, 8, 8, 191, 113, b), br.binned_loop(img, 8, 8, 191, 113, b)
        assert a["sum"].shape == shape and br.bin_pixels(191, 113, b)[-1, -1] == corner
        for s in br.STATS:
            assert (a[s] == c[s]).all()
        batch = br.binned_reduceat(np.stack([img, img]), 8, 8, 191, 113, b)
        assert (batch["max"][1] == a["max"]).all()


def test_windows_follow_the_rules():
    for W, H in ((4096, 3072), (1921, 1081), (200, 123), (1, 1), (8, 8), (9, 9), (4200, 24)):
        for b in (2, 4, 8):
            ws = br.windows(W, H, b)
            assert ws[0] == (0, 0, W, H) and len(ws) in (4, 5)
            for (x, y, rw, rh) in ws:
                assert x % b == 0 and y % b == 0 and rw >= 1 and rh >= 1 and x + rw <= W and y + rh <= H
            if len(ws) == 5:
                x, y, rw, rh = ws[1]
                assert rw % 2 == 1 and rh % 2 == 1 and (b == 8 or (x % 8 and y % 8))
            assert len(ws) == 5 or W < 12 or H < 12


def test_binned_pixels_and_mean():
    import torch
    import dbde_video_cpp_amd as dv
    for rw, rh, b in ((191, 113, 2), (191, 113, 4), (191, 113, 8), (1, 1, 8), (16, 8, 4)):
        px = dv.bin_pixels(rh, rw, b)
        assert px.dtype == torch.int32 and tuple(px.shape) == br.out_shape(rw, rh, b)
        assert (px.numpy() == br.bin_pixels(rw, rh, b)).all() and int(px.sum()) == rw * rh
    e = dv.Binned.empty(3, 5, 7, 4, ("sum", "min"), "cpu")
    assert e.max is None and e.sum.dtype == torch.int16 and e.min.dtype == torch.uint8 and e.bin == 4
    assert tuple(e.sum.shape) == (3, 2, 2) and e.pixels.tolist() == [[16, 12], [4, 3]]
    e16 = dv.Binned.empty(2, 8, 8, 2, ("sum", "max", "min"), "cpu", pix=2)
    assert e16.sum.dtype == torch.int32 and e16.max.dtype == torch.int16 and tuple(e16.min.shape) == (2, 4, 4)
    hand = dv.Binned(sum=torch.tensor([[[32, 24], [8, 9]]], dtype=torch.int16), bin=4, pixels=e.pixels)
    m = hand.mean()
    assert m.dtype == torch.float32 and m.tolist() == [[[2.0, 2.0], [2.0, 3.0]]]
    with pytest.raises(ValueError):
        dv.Binned.empty(1, 8, 8, 3, ("sum",), "cpu")
    with pytest.raises(ValueError):
        dv.Binned.empty(1, 8, 8, 2, ("mean",), "cpu")
