"""GPU: exact per-pixel temporal quantiles from the compressed stream -- quantiles.temporal_quantile, temporal_median and
quantile_file -- against np.sort of the accepted decoded images (numpy's method="lower"), by equality."""
from importlib import import_module

import numpy as np
import pytest

import counts_ref as cref
import wproject_gpu as wg
from test_gpu_project import Batch
from test_gpu_roi16 import Batch16, images16
from test_oracle_u16 import o16   # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

QS = (0, 0.08, 0.5, 1)
WINDOWS = [(0, 0, 100, 50), (3, 5, 41, 27)]


@pytest.fixture(scope="module")
def qt():
    return import_module("dbde_video_cpp_amd.quantiles")


@pytest.fixture(scope="module")
def codec():
    import dbde_video_cpp_amd as m
    c = m.Codec(0)
    yield c
    c.close()


def check(qt, codec, s, bits, what):
    for win in WINDOWS if (s.W, s.H) == (100, 50) else [(0, 0, s.W, s.H), (3, 5, 41, 27)]:
        args = (codec, s.buf, s.lead, s.total, s.offs, s.W, s.H, s.n)
        many, count, res = qt.temporal_quantile(*args, QS, *win, bits=bits)
        codec.sync()
        N = sum(im is not None for im in s.images)
        assert int(count.item()) == N and tuple(res.shape) == (s.n, 4)
        assert tuple(many.shape) == (len(QS), win[3], win[2])
        got = many.cpu().numpy()
        got = got if bits == 8 else got.view(np.uint16)
        for i, q in enumerate(QS):
            want, _ = cref.order_statistic(s.images, q, *win)
            assert np.array_equal(got[i], want), (what, q, win)
            assert np.array_equal(want, np.quantile(cg_stack(s, win), q, axis=0, method="lower")), "the reference"
            one, c1, _ = qt.temporal_quantile(*args, q, *win, bits=bits)
            codec.sync()
            assert np.array_equal(one.cpu().numpy(), many[i].cpu().numpy()) and int(c1.item()) == N
        med, _, _ = qt.temporal_median(*args, *win, bits=bits)
        codec.sync()
        assert np.array_equal(med.cpu().numpy(), many[2].cpu().numpy())
        assert np.array_equal(got[2], np.sort(cg_stack(s, win), 0)[(N - 1) // 2])


def cg_stack(s, win):
    x, y, rw, rh = win
    return np.stack([im[y:y + rh, x:x + rw] for im in s.images if im is not None])


@pytest.mark.parametrize("n", [13, 70])
def test_quantiles_8bit(qt, codec, n):
    b = Batch(codec, "mixed", 100, 50, n)
    s = wg.Stream(b.buf, b.lead, b.total, b.offs, 100, 50, list(b.images.cpu().numpy()))
    check(qt, codec, s, 8, f"8-bit n={n}")


def test_quantiles_16bit(qt, codec, o16):   # noqa: F811
    imgs = images16(np.random.default_rng(3), 13, 100, 50, "mixed")
    imgs[:, 7, 9] = 0           # pixels constant at 0 and at the maximum, and one with only the two extremes
    imgs[:, 7, 10] = 65535
    imgs[::2, 7, 11], imgs[1::2, 7, 11] = 0, 65535
    b = Batch16(codec, o16, imgs)
    s = wg.Stream(b.buf, b.lead, b.total, b.offs, 100, 50, b.full)
    check(qt, codec, s, 16, "16-bit n=13")


@pytest.mark.parametrize("bits,bad", [(8, (1, 5, 6, 11)), (16, (0, 12)), (8, tuple(range(7)))])
def test_crafted_stream_with_rejected_frames(qt, codec, bits, bad):
    """Rejected frames take no part: N is the accepted count, the rank floor(q * (N - 1)); every frame rejected gives
    zeros and count 0."""
    n = 13 if len(bad) < 7 else 7
    s = wg.crafted_stream(np.random.default_rng(bits + len(bad)), 72, 40, n, bits, bad)
    if len(bad) < n:
        check(qt, codec, s, bits, f"crafted {bits}-bit")
        return
    vals, count, _ = qt.temporal_quantile(codec, s.buf, s.lead, s.total, s.offs, 72, 40, n, (0, 0.5, 1), 3, 5, 41, 27)
    codec.sync()
    assert int(count.item()) == 0 and (vals == 0).all() and tuple(vals.shape) == (3, 27, 41)


def test_quantile_file(qt, codec, tmp_path):
    """A written file of 13 frames of 72 x 40, read in batches of 4 and of 64: the in-memory result."""
    import torch
    W, H, n = 72, 40, 13
    imgs = codec.synth_frames("mixed", 77, 0, n, W, H)
    path = str(tmp_path / "q.dbde")
    with codec.open_writer(path, W, H, frame_hz=30.0, batch_frames=4) as wtr:
        wtr.put(imgs, n)
    b = Batch(codec, None, W, H, n, images=imgs)
    host = list(imgs.cpu().numpy())
    for window in (None, (3, 5, 41, 27)):
        win = (0, 0, W, H) if window is None else window
        mem, _, _ = qt.temporal_quantile(codec, b.buf, b.lead, b.total, b.offs, W, H, n, QS, *win)
        codec.sync()
        for batch in (4, 64):
            got, count, res = qt.quantile_file(codec, path, QS, batch=batch, window=window)
            codec.sync()
            assert torch.equal(got, mem), (window, batch)
            assert int(count.item()) == n and tuple(res.shape) == (n, 4) and res[:, 1].tolist() == list(range(n))
        for i, q in enumerate(QS):
            assert np.array_equal(mem[i].cpu().numpy(), cref.order_statistic(host, q, *win)[0])
    one, _, _ = qt.quantile_file(codec, path, 0.5, batch=5)
    assert torch.equal(one, qt.temporal_median(codec, b.buf, b.lead, b.total, b.offs, W, H, n)[0])
    with pytest.raises(ValueError):
        qt.quantile_file(codec, path, 0.5, bits=16)
