"""GPU: the local correlation image from the compressed stream -- correlation.local_correlation, correlation_image and
correlation_file -- against tests/pairs_ref.py's two-pass Pearson over the decoded images.

Tolerance 1e-9 absolute: both sides are float64 evaluations, and at these sizes every integer involved is exact
(N^2 * 2^32 << 2^53), so the difference is a few ulps of a number in [-1, 1]."""
from importlib import import_module

import numpy as np
import pytest

import pairs_ref as pref
import wproject_gpu as wg
from test_gpu_project import Batch
from test_gpu_roi16 import Batch16, images16
from test_oracle_u16 import o16   # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

TOL = 1e-9
WINDOWS = [(0, 0, 100, 50), (3, 5, 41, 27)]


@pytest.fixture(scope="module")
def cor():
    return import_module("dbde_video_cpp_amd.correlation")


@pytest.fixture(scope="module")
def codec():
    import dbde_video_cpp_amd as m
    c = m.Codec(0)
    yield c
    c.close()


def check(cor, codec, s, bits, what):
    project, project_pairs = (codec.project, codec.project_pairs) if bits == 8 else (codec.project16, codec.project_pairs16)
    N = sum(im is not None for im in s.images)
    for win in WINDOWS:
        for neighbours in (4, 8):
            want = pref.local_correlation(s.images, 3 if neighbours == 4 else 15, *win)
            assert np.abs(want).max() > 0.05, "the reference is not flat"
            args = (s.buf, s.lead, s.total, s.offs, s.W, s.H, s.n)
            img, count, res = cor.correlation_image(codec, *args, *win, neighbours=neighbours, bits=bits)
            codec.sync()
            got = img.cpu().numpy()
            assert got.dtype == np.float64 and got.shape == (win[3], win[2]) and int(count.item()) == N
            assert tuple(res.shape) == (s.n, 4)
            err = np.abs(got - want).max()
            print(f"{what} {win} neighbours={neighbours}: max |difference| = {err:.3e}")
            assert err <= TOL, (what, win, neighbours, err)
            pr, _ = project(*args, *win, stats=("sum", "sumsq"))
            pp, _ = project_pairs(*args, neighbours, *win)
            codec.sync()
            assert np.array_equal(cor.local_correlation(pp, pr).cpu().numpy(), got)


def test_matches_the_reference_8bit(cor, codec):
    b = Batch(codec, "mixed", 100, 50, 13)
    check(cor, codec, wg.Stream(b.buf, b.lead, b.total, b.offs, 100, 50, list(b.images.cpu().numpy())), 8, "8-bit")


def test_matches_the_reference_16bit(cor, codec, o16):   # noqa: F811
    b = Batch16(codec, o16, images16(np.random.default_rng(3), 13, 100, 50, "mixed"))
    check(cor, codec, wg.Stream(b.buf, b.lead, b.total, b.offs, 100, 50, b.full), 16, "16-bit")


def test_rejected_frames_take_no_part(cor, codec):
    s = wg.crafted_stream(np.random.default_rng(31), 100, 50, 13, 8, bad=(2, 3, 9))
    check(cor, codec, s, 8, "crafted 8-bit")


def planted(rng, n, W, H, rects):
    """Independent noise 40 + U{0..20} per pixel and frame; inside rectangle k every pixel also carries the same
    frames-long signal s_k ~ U{0..150}: two pixels of a rectangle correlate at var(s) / (var(s) + var(noise)) = 0.98,
    any other two at 0 +- 1 / sqrt(n)."""
    img = 40 + rng.integers(0, 21, (n, H, W))
    for x, y, w, h in rects:
        img[:, y:y + h, x:x + w] += rng.integers(0, 151, (n, 1, 1))
    return img.astype(np.uint8)


def test_a_planted_structure_stands_out(cor, codec):
    """Inside a rectangle (the pixels whose whole neighbourhood lies in it: a border pixel averages in neighbours
    outside, a corner has 5 of 8) the image is > 0.9, outside both |r| < 0.7.  The CPU reference alone meets both
    bounds, asserted first."""
    import torch
    rng = np.random.default_rng(2024)
    W, H, n = 100, 50, 64
    rects = [(10, 8, 20, 14), (55, 25, 30, 18)]
    imgs = planted(rng, n, W, H, rects)
    inside = np.zeros((H, W), bool)
    outside = np.ones((H, W), bool)
    for x, y, w, h in rects:
        inside[y + 1:y + h - 1, x + 1:x + w - 1] = True
        outside[y:y + h, x:x + w] = False
    want = pref.local_correlation(list(imgs), 15, 0, 0, W, H)
    assert want[inside].min() > 0.9 and np.abs(want[outside]).max() < 0.7
    b = Batch(codec, None, W, H, n, images=torch.from_numpy(imgs).cuda())
    for neighbours in (4, 8):
        got, _, _ = cor.correlation_image(codec, b.buf, b.lead, b.total, b.offs, W, H, n, neighbours=neighbours)
        codec.sync()
        got = got.cpu().numpy()
        assert got[inside].min() > 0.9 and np.abs(got[outside]).max() < 0.7, neighbours
    assert np.abs(got - want).max() <= TOL


def test_zero_variance_pixels_follow_the_rule(cor, codec):
    """A constant pixel takes part in no pair: it gives 0 itself and its neighbours average over the others; a
    constant block's interior and a pixel whose every neighbour is constant give 0."""
    import torch
    rng = np.random.default_rng(9)
    W, H, n = 40, 24, 13
    imgs = rng.integers(0, 256, (n, H, W)).astype(np.uint8)
    imgs[:, 5, 7] = 200                       # one constant pixel
    imgs[:, 10:16, 20:28] = 17                # a constant block
    imgs[:, 0:3, 0:3] = 0
    imgs[:, 1, 1] = np.arange(n)              # a varying pixel whose 8 neighbours are all constant
    b = Batch(codec, None, W, H, n, images=torch.from_numpy(imgs).cuda())
    for neighbours, mask in ((4, 3), (8, 15)):
        want = pref.local_correlation(list(imgs), mask, 0, 0, W, H)
        got, _, _ = cor.correlation_image(codec, b.buf, b.lead, b.total, b.offs, W, H, n, neighbours=neighbours)
        codec.sync()
        got = got.cpu().numpy()
        assert np.isfinite(got).all() and np.abs(got - want).max() <= TOL
        assert got[5, 7] == 0 and (got[11:15, 21:27] == 0).all() and got[1, 1] == 0 and got[0, 0] == 0
        assert got[5, 8] != 0 and got[9, 22] != 0
    # no frame at all: zeros, count 0
    img, count, _ = cor.correlation_image(codec, b.buf, b.lead, b.total, b.offs, W, H, 0)
    codec.sync()
    assert (img == 0).all() and int(count.item()) == 0
    for kw in (dict(neighbours=6), dict(bits=12)):
        with pytest.raises(ValueError):
            cor.correlation_image(codec, b.buf, b.lead, b.total, b.offs, W, H, n, **kw)
    pr, _ = codec.project(b.buf, b.lead, b.total, b.offs, W, H, n, stats=("sum",))
    pp, _ = codec.project_pairs(b.buf, b.lead, b.total, b.offs, W, H, n, 4)
    with pytest.raises(ValueError):
        cor.local_correlation(pp, pr)         # no sumsq


def test_correlation_file(cor, codec, tmp_path):
    """A written file of 13 frames of 72 x 40 in batches of 5 (three batches), 4 and 64: the one-call image bit for bit,
    since the planes are integers."""
    import torch
    W, H, n = 72, 40, 13
    imgs = codec.synth_frames("mixed", 77, 0, n, W, H)
    path = str(tmp_path / "c.dbde")
    with codec.open_writer(path, W, H, frame_hz=30.0, batch_frames=4) as wtr:
        wtr.put(imgs, n)
    b = Batch(codec, None, W, H, n, images=imgs)
    host = list(imgs.cpu().numpy())
    for window in (None, (3, 5, 41, 27)):
        win = (0, 0, W, H) if window is None else window
        for neighbours in (4, 8):
            mem, _, _ = cor.correlation_image(codec, b.buf, b.lead, b.total, b.offs, W, H, n, *win, neighbours=neighbours)
            codec.sync()
            for batch in (5, 4, 64):
                got, count, res = cor.correlation_file(codec, path, neighbours=neighbours, batch=batch, window=window)
                codec.sync()
                assert torch.equal(got, mem), (window, neighbours, batch)
                assert int(count.item()) == n and tuple(res.shape) == (n, 4) and res[:, 1].tolist() == list(range(n))
            want = pref.local_correlation(host, 3 if neighbours == 4 else 15, *win)
            assert np.abs(mem.cpu().numpy() - want).max() <= TOL
    with pytest.raises(ValueError):
        cor.correlation_file(codec, path, bits=16)
