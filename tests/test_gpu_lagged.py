"""GPU: the noise, motion and autocorrelation images from the compressed stream -- lagged.noise_image,
mean_abs_difference, autocorrelation, peak_to_noise, lag_image and lag_file -- against numpy evaluations of the same
formulas and tests/lag_ref.py's two-pass autocorrelation over the decoded images.

Tolerance 1e-9 absolute, the one tests/test_gpu_correlation.py uses for the same kind of arithmetic: both sides are
float64 evaluations of exact integers (at n = 64 and 8 bits N^3 * 255^2 = 1.7e10 << 2^53), so they differ by a few ulps
of numbers of the order of 1 (autocorrelation) or 10 (noise levels)."""
from importlib import import_module

import numpy as np
import pytest

import crafted as cr
import lag_ref as lr
from test_gpu_project import Batch

pytestmark = pytest.mark.gpu

TOL = 1e-9
W, H, N = 100, 50, 64
SIGMA, RAMP = 4.0, 60.0                      # noise per pixel and frame; the ramp's rise over the N frames
FLAT, SLOW = (slice(5, 45), slice(5, 45)), (slice(5, 45), slice(55, 95))      # (rows, columns) of the two regions


@pytest.fixture(scope="module")
def lagged():
    return import_module("dbde_video_cpp_amd.lagged")


@pytest.fixture(scope="module")
def codec():
    import dbde_video_cpp_amd as m
    c = m.Codec(0)
    yield c
    c.close()


def scene(rng):
    """A fixed image plus independent N(0, SIGMA^2) noise per pixel and frame, rounded; the SLOW region also carries a
    linear ramp of RAMP grey levels over the N frames; pixel (0, 0) is constant."""
    base = rng.integers(60, 120, (H, W)).astype(np.float64)
    img = base[None] + rng.normal(0.0, SIGMA, (N, H, W))
    img[(slice(None),) + SLOW] += np.linspace(0.0, RAMP, N)[:, None, None]
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    img[:, 0, 0] = 77
    return img


@pytest.fixture(scope="module")
def batch(codec):
    import torch
    imgs = scene(np.random.default_rng(11))
    return Batch(codec, None, W, H, N, images=torch.from_numpy(imgs).cuda()), imgs


def args(b, n=N):
    return (b.buf, b.lead, b.total, b.offs, W, H, n)


def test_noise_image_ignores_a_slow_signal(lagged, codec, batch):
    """noise_image equals the numpy evaluation of sqrt(sqdiff / (2 P)) within 1e-9; the ramp region's mean noise level
    lies within the spread (minimum to maximum over the pixels) of the flat region's, while its standard deviation from
    project is at least twice the flat region's.  Both hold on the reference, asserted first."""
    b, imgs = batch
    x = imgs.astype(np.float64)
    ref_noise = np.sqrt(((x[1:] - x[:-1]) ** 2).sum(0) / (2.0 * (N - 1)))
    ref_std = x.std(0)
    assert ref_noise[FLAT].min() <= ref_noise[SLOW].mean() <= ref_noise[FLAT].max()
    assert abs(ref_noise[FLAT].mean() - SIGMA) < 0.1 * SIGMA            # it estimates the planted sigma
    assert ref_std[SLOW].mean() >= 2.0 * ref_std[FLAT].mean()
    lp, res = lagged.lag_image(codec, *args(b), lag=1, stats=("sqdiff", "absdiff"))
    pr, _ = codec.project(*args(b), stats=("sum", "sumsq"))
    codec.sync()
    got = lagged.noise_image(lp).cpu().numpy()
    assert got.dtype == np.float64 and got.shape == (H, W) and tuple(res.shape) == (N, 4)
    err = np.abs(got - ref_noise).max()
    print(f"noise_image: max |difference| = {err:.3e}")
    assert err <= TOL
    S, Q = pr.sum.cpu().numpy().astype(np.float64), pr.sumsq.cpu().numpy().astype(np.float64)
    std = np.sqrt(Q / N - (S / N) ** 2)
    assert got[FLAT].min() <= got[SLOW].mean() <= got[FLAT].max()
    assert std[SLOW].mean() >= 2.0 * std[FLAT].mean()
    assert got[0, 0] == 0
    mad = lagged.mean_abs_difference(lp).cpu().numpy()
    assert np.abs(mad - np.abs(x[1:] - x[:-1]).sum(0) / (N - 1)).max() <= TOL
    # peak to noise: (max - baseline) / noise, 0 where the noise is 0
    pm, _ = codec.project(*args(b), stats=("max",))
    pnr = lagged.peak_to_noise(pm.max, 60, lp).cpu().numpy()
    want = np.where(ref_noise > 0, (imgs.max(0).astype(np.float64) - 60) / np.where(ref_noise > 0, ref_noise, 1), 0)
    assert np.abs(pnr - want).max() <= 1e-9 * np.abs(want).max() and pnr[0, 0] == 0
    with pytest.raises(ValueError):
        lagged.autocorrelation(lp, pr)          # no product


@pytest.mark.parametrize("lag", (1, 3, 8))
def test_autocorrelation_matches_two_passes(lagged, codec, batch, lag):
    b, imgs = batch
    want = lr.autocorrelation_two_pass(list(imgs), lag, 0, 0, W, H)
    assert want[SLOW].mean() > 0.5 and abs(want[FLAT].mean()) < 0.1      # the ramp correlates, the noise does not
    lp, _ = lagged.lag_image(codec, *args(b), lag=lag, stats=("product", "pairsum"))
    pr, _ = codec.project(*args(b), stats=("sum", "sumsq"))
    codec.sync()
    got = lagged.autocorrelation(lp, pr).cpu().numpy()
    err = np.abs(got - want).max()
    print(f"autocorrelation lag {lag}: max |difference| = {err:.3e}")
    assert err <= TOL and got[0, 0] == 0 and np.isfinite(got).all()           # a zero-variance pixel gives 0
    # P = 0 (n <= lag): 0 everywhere
    lp0, _ = lagged.lag_image(codec, *args(b, lag), lag=lag, stats=("product", "pairsum", "sqdiff", "absdiff"))
    pr0, _ = codec.project(*args(b, lag), stats=("sum", "sumsq"))
    codec.sync()
    assert int(lp0.pairs.item()) == 0 and not lagged.autocorrelation(lp0, pr0).any()
    assert not lagged.noise_image(lp0).any() and not lagged.mean_abs_difference(lp0).any()


def test_lag_file_equals_one_call(lagged, codec, tmp_path):
    """A file written with FileWriter (45 frames of 72 x 40, one of them corrupted on disk) streamed in batches of 16 at
    lag 3: the planes and scalars equal lag_image of the same bytes bit for bit and tests/lag_ref.py; the results rows
    cover the 45 frames once."""
    import torch
    w, h, n, lag, broken = 72, 40, 45, 3, 20
    imgs = codec.synth_frames("mixed", 78, 0, n, w, h)
    path = str(tmp_path / "l.dbde")
    with codec.open_writer(path, w, h, frame_hz=30.0, batch_frames=4) as wtr:
        wtr.put(imgs, n)
    data = bytearray(open(path, "rb").read())
    T = cr.tiles(w, h)
    at = 28
    for _ in range(broken):
        at += 32 + 2 * T + 8 * int.from_bytes(data[at + 28 + 2 * T: at + 32 + 2 * T], "little")
    data[at + 24] = 9                           # a depth above 8: the frame is rejected, its size fields are intact
    open(path, "wb").write(data)
    host = [None if f == broken else im for f, im in enumerate(imgs.cpu().numpy())]
    buf = torch.from_numpy(np.frombuffer(bytes(data[28:]), np.uint8).copy()).cuda()
    offs, found = codec.index_stream(buf, 0, buf.numel(), w, h, n + 1)
    assert found == n
    for window in (None, (3, 5, 41, 27)):
        win = (0, 0, w, h) if window is None else window
        mem, mres = lagged.lag_image(codec, buf, 0, buf.numel(), offs, w, h, n, lag, lr.STATS, *win)
        codec.sync()
        want = lr.lag(host, lag, *win)
        assert want["pairs"] == n - lag - 2 and want["count"] == n - 1
        for batch in (16, 3, 64):
            got, res = lagged.lag_file(codec, path, lag=lag, stats=lr.STATS, batch=batch, window=window)
            codec.sync()
            for k in lr.STATS + ("pairs", "count"):
                assert torch.equal(getattr(got, k), getattr(mem, k)), (window, batch, k)
            assert tuple(res.shape) == (n, 4) and torch.equal(res, mres)
        for k in lr.STATS[:4]:
            assert np.array_equal(mem.__dict__[k].cpu().numpy().view(np.uint64), want[k]), k
        assert np.array_equal(mem.maxdiff.cpu().numpy(), want["maxdiff"])
        assert int(mem.pairs.item()) == want["pairs"] and int(mem.count.item()) == want["count"]
    with pytest.raises(ValueError):
        lagged.lag_file(codec, path, lag=3, batch=2)
