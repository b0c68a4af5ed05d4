"""GPU: weighted temporal projections -- dbde_hip_project_weighted (Codec.project_weighted).

Every plane is compared bit for bit (.view(int32)) with the defined value computed by tests/wproject_ref.py -- chains of
true single-rounding fused multiply-adds in frame order, per segment of the plan, combined in ascending segment order --
over the images dbde_hip_decode_frames writes for encoded batches and tests/crafted.py's numpy decoder writes for
crafted frames.  Nothing expected comes from the call itself.
"""
from importlib import import_module

import numpy as np
import pytest

import wproject_gpu as wg
import wproject_ref as wr
from test_gpu_project import Batch

pytestmark = pytest.mark.gpu

# edge tiles in both directions (72x40, 100x50) and a frame wider than one piece of 32 tiles (520 > 256 pixels)
SHAPES = [(72, 40), (100, 50), (520, 16)]
COUNTS = (1, 3, 4, 5, 13)       # the four-frame pipeline step's boundaries and tails
REGRESSORS = (1, 2, 3, 8)
NMAX = 13


def windows(W, H):
    """The full frame, an unaligned window (x = 3, y = 5, 41 x 27 where the frame has the rows), one pixel; for the
    wide frame a window across the boundary of the two pieces."""
    out = [(0, 0, W, H), (3, 5, 41, min(27, H - 5)), (W // 2 + 1, H - 2, 1, 1)]
    if W > 256:
        out.append((251, 1, 13, H - 2))
    return out


@pytest.fixture(scope="module")
def dv():
    import dbde_video_cpp_amd as m
    return m


@pytest.fixture(scope="module")
def codec(dv):
    c = dv.Codec(0)
    assert c.arch.startswith("gfx950")
    yield c
    c.close()


@pytest.fixture(scope="module")
def cus(codec):
    return wg.cus_of(codec)


def stream_of(codec, W, H, n, mode="mixed", images=None):
    b = Batch(codec, mode, W, H, n, images=images)
    return wg.Stream(b.buf, b.lead, b.total, b.offs, W, H, list(b.images.cpu().numpy())), b


@pytest.fixture(scope="module")
def streams(codec):
    cache = {}

    def get(W, H, n=NMAX, mode="mixed"):
        if (W, H, n, mode) not in cache:
            cache[(W, H, n, mode)] = stream_of(codec, W, H, n, mode)
        return cache[(W, H, n, mode)]
    return get


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("W,H", SHAPES)
def test_matches_the_reference_chain(dv, codec, cus, streams, W, H, n):
    """Every window x regressor count, the weight family cycling; small n has one segment, so the default call and the
    one_segment call are the same chain and both are checked."""
    import torch
    full, b = streams(W, H)
    s = full.first(n)
    rng = np.random.default_rng(W * 31 + n)
    i = 0
    for win in windows(W, H):
        for R in REGRESSORS:
            fam = wg.FAMILIES[i % len(wg.FAMILIES)]
            w = wg.family(rng, fam, R, n)
            _, res, p = wg.check(codec.project_weighted, dv.wproject_plan, cus, s, w, win, one_segment=bool(i & 1),
                                 what=fam)
            assert p["segments"] == 1
            assert torch.equal(res, b.results[:n])
            i += 1
    if W > 256:
        assert dv.wproject_plan(W, H, n)["pieces_x"] > 1


@pytest.mark.parametrize("mode", ["noise8", "flat", "smooth"])
def test_other_frame_contents(dv, codec, cus, streams, mode):
    W, H, n = 100, 50, 5
    s, _ = streams(W, H, n, mode)
    rng = np.random.default_rng(7)
    for win in windows(W, H)[:2]:
        wg.check(codec.project_weighted, dv.wproject_plan, cus, s, wg.family(rng, "normal", 3, n), win, what=mode)


@pytest.mark.parametrize("n,S", [(50, 2), (70, 3)])
def test_segments_combine_in_ascending_order(dv, codec, cus, streams, n, S):
    """A window of few workgroups and n >= 33 frames: the plan cuts S segments on this device (asserted, not assumed).
    The same inputs with one_segment=True give the pure chain, and the two references differ, so the order shows."""
    W, H = 72, 40
    s, _ = streams(W, H, 70)
    s = s.first(n)
    rng = np.random.default_rng(n)
    for win in [(0, 0, W, H), (3, 5, 41, 27)]:
        for R in (1, 3, 8):
            w = wg.family(rng, "normal", R, n)
            seg, _, p = wg.check(codec.project_weighted, dv.wproject_plan, cus, s, w, win, what="segments")
            assert p["segments"] == S and p["workspace_bytes"] > 0
            one, _, p1 = wg.check(codec.project_weighted, dv.wproject_plan, cus, s, w, win, one_segment=True,
                                  what="one segment")
            assert p1["segments"] == 1
            assert not np.array_equal(wr.bits(seg.out.cpu().numpy()), wr.bits(one.out.cpu().numpy()))
    # a crafted order: 2^24, then ones -- every +1 is lost inside one chain, but a later segment's sum of ones is not
    w = np.ones((1, n), np.float32)
    w[0, 0] = 2.0 ** 24
    seg, _, _ = wg.check(codec.project_weighted, dv.wproject_plan, cus, s, w, (0, 0, W, H), what="crafted order")
    one, _, _ = wg.check(codec.project_weighted, dv.wproject_plan, cus, s, w, (0, 0, W, H), one_segment=True)
    assert not np.array_equal(seg.out.cpu().numpy(), one.out.cpu().numpy())


def test_fma_witnesses_at_a_known_pixel_and_frame(dv, codec, cus):
    """Frames 0 and 1 hold 255 at (py, px); w = -1 then 1 + 2^-23: the chain passes through fmaf(w, 255, -255), where
    a multiply followed by an add gives 2^-15 and the fused operation 255 * 2^-23."""
    import torch
    W, H, n, py, px = 72, 40, 5, 13, 29
    ww, p, acc = wr.WITNESS_U8
    rng = np.random.default_rng(11)
    imgs = rng.integers(0, 256, (n, H, W)).astype(np.uint8)
    imgs[0, py, px] = imgs[1, py, px] = p
    s, _ = stream_of(codec, W, H, n, images=torch.from_numpy(imgs).cuda())
    for R in (1, 8):
        w = wg.family(rng, "normal", R, n)
        w[:, 0], w[:, 1] = -1.0, ww
        two = s.first(2)
        out, _, _ = wg.check(codec.project_weighted, dv.wproject_plan, cus, two, w[:, :2], (0, 0, W, H), what="witness")
        got = out.out[:, py, px].cpu().numpy()
        assert (got == wr.fmaf_libm(ww, p, acc)).all() and (got != wr.mul_then_add(ww, p, acc)).all()
        wg.check(codec.project_weighted, dv.wproject_plan, cus, s, w, (3, 5, 41, 27), what="witness in a longer chain")


def test_all_ones_equals_the_integer_sum(codec, streams):
    """n * 255 < 2^24: every partial sum is an exact integer in F32, so the plane equals Codec.project's sum."""
    import torch
    for W, H in SHAPES:
        s, _ = streams(W, H)
        for win in windows(W, H):
            w = torch.ones((2, s.n), dtype=torch.float32, device="cuda")
            out, _ = codec.project_weighted(s.buf, s.lead, s.total, s.offs, W, H, s.n, w, *win)
            pr, _ = codec.project(s.buf, s.lead, s.total, s.offs, W, H, s.n, *win, stats=("sum",))
            codec.sync()
            assert torch.equal(out.out[0].to(torch.int64), pr.sum) and torch.equal(out.out[1].to(torch.int64), pr.sum)
            assert torch.equal(out.count, pr.count)


def test_rejected_frames_add_nothing_and_their_weights_are_unused(dv, codec, cus):
    """Crafted frames with rejected ones in the middle of a run, NaN weights at the rejected frames: finite planes, the
    reference's bits, project's count and results."""
    import torch
    W, H, n = 72, 40, 13
    bad = (1, 5, 6, 11)
    s = wg.crafted_stream(np.random.default_rng(5), W, H, n, 8, bad)
    rng = np.random.default_rng(6)
    for win in windows(W, H):
        for R in (1, 3, 8):
            w = wg.family(rng, "normal", R, n)
            w[:, list(bad)] = np.nan
            out, res, _ = wg.check(codec.project_weighted, dv.wproject_plan, cus, s, w, win, what="crafted")
            assert torch.isfinite(out.out).all()
            pr, want_res = codec.project(s.buf, s.lead, s.total, s.offs, W, H, n, *win, stats=("sum",))
            codec.sync()
            assert torch.equal(res, want_res) and int(out.count.item()) == int(pr.count.item()) == n - len(bad)
            sums = dv.WeightedProjection.weight_sums(wg.strided(w), res).cpu().numpy()
            keep = [f for f in range(n) if f not in bad]
            assert np.allclose(sums, w[:, keep].astype(np.float64).sum(1), rtol=1e-12, atol=0)


def test_every_frame_rejected(dv, codec, cus):
    """accumulate=False: +0.0 planes and count 0; accumulate=True: the planes and the count stay as they were."""
    import torch
    W, H, n = 72, 40, 7
    s = wg.crafted_stream(np.random.default_rng(8), W, H, n, 8, bad=range(n))
    w = np.full((3, n), np.nan, np.float32)
    for win in windows(W, H)[:2]:
        out, _, _ = wg.check(codec.project_weighted, dv.wproject_plan, cus, s, w, win, what="all rejected")
        assert (out.out.view(torch.int32) == 0).all() and int(out.count.item()) == 0
        prior = torch.from_numpy(wg.family(np.random.default_rng(9), "e30", 3, win[2] * win[3])).cuda().view(3, win[3], win[2])
        out = dv.WeightedProjection(prior.clone(), torch.full((1,), 5, dtype=torch.int64, device="cuda"))
        codec.project_weighted(s.buf, s.lead, s.total, s.offs, W, H, n, wg.strided(w), *win, out=out, accumulate=True)
        codec.sync()
        assert torch.equal(out.out.view(torch.int32), prior.view(torch.int32)) and int(out.count.item()) == 5


@pytest.mark.parametrize("cut", [1, 4, 6])
def test_accumulate_continues_the_chain(dv, codec, cus, streams, cut):
    """Two consecutive calls: the second is prior + P_0 (+ P_1 ...), one F32 addition per segment -- the reference with
    prior.  n == 0 changes nothing."""
    import torch
    W, H, n = 100, 50, 13
    full, _ = streams(W, H)
    rng = np.random.default_rng(cut)
    win = (3, 5, 41, 27)
    for R in (2, 8):
        w = wg.family(rng, "normal", R, n)
        out, _, _ = wg.check(codec.project_weighted, dv.wproject_plan, cus, full.first(cut), w[:, :cut], win)
        prior = out.out.cpu().numpy().copy()
        codec.project_weighted(full.buf, full.lead, full.total, full.offs[cut:], W, H, n - cut, wg.strided(w[:, cut:]),
                               *win, out=out, accumulate=True)
        codec.sync()
        want, _ = wr.wproject(full.images[cut:], w[:, cut:], *win, accumulate=True, prior=prior)
        wg.assert_bits(out.out, want, f"accumulate after {cut}")
        assert int(out.count.item()) == n
        before = out.out.clone()
        codec.project_weighted(full.buf, full.lead, full.total, full.offs, W, H, 0, wg.strided(w), *win, out=out,
                               accumulate=True)
        codec.sync()
        assert torch.equal(out.out.view(torch.int32), before.view(torch.int32)) and int(out.count.item()) == n
        codec.project_weighted(full.buf, full.lead, full.total, full.offs, W, H, 0, wg.strided(w), *win, out=out)
        codec.sync()
        assert (out.out.view(torch.int32) == 0).all() and int(out.count.item()) == 0     # +0.0 planes, count 0


def test_accumulate_over_several_segments(dv, codec, cus, streams):
    W, H, n = 72, 40, 70
    s, _ = streams(W, H, 70)
    win = (3, 5, 41, 27)
    rng = np.random.default_rng(3)
    w = wg.family(rng, "normal", 3, n)
    out, _, _ = wg.check(codec.project_weighted, dv.wproject_plan, cus, s.first(13), w[:, :13], win)
    prior = out.out.cpu().numpy().copy()
    p = dv.wproject_plan(W, H, n, *win, regressors=3, n_cu=cus)
    assert p["segments"] == 3
    codec.project_weighted(s.buf, s.lead, s.total, s.offs, W, H, n, wg.strided(w), *win, out=out, accumulate=True)
    codec.sync()
    want, _ = wr.wproject(s.images, w, *win, segments=3, fps=p["frames_per_segment"], accumulate=True, prior=prior)
    wg.assert_bits(out.out, want, "accumulate, 3 segments")
    assert int(out.count.item()) == 13 + n


@pytest.mark.parametrize("n", [13, 70])
def test_guard_bands_and_more_than_eight_regressors(dv, codec, cus, streams, n):
    """The planes sit in a canvas of NaN-pattern sentinels: nothing in front of, behind or between ... the planes'
    extent is written (one and three segments).  R = 11 through the wrapper equals eleven one-row calls."""
    import torch
    W, H = 72, 40
    s, _ = streams(W, H, 70)
    s = s.first(n)
    win = (3, 5, 41, 27)
    rw, rh = win[2], win[3]
    R, G = 11, 64
    rng = np.random.default_rng(n)
    w = wg.family(rng, "normal", R, n)
    sent = int(np.array([wg.SENT_BITS], np.uint32).view(np.int32)[0])
    canvas = torch.full((G + R * rh * rw + G,), sent, dtype=torch.int32, device="cuda")
    planes = canvas[G: G + R * rh * rw].view(torch.float32).view(R, rh, rw)
    count = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    out = dv.WeightedProjection(planes, count[1:2])
    got, _ = codec.project_weighted(s.buf, s.lead, s.total, s.offs, W, H, n, wg.strided(w), *win, out=out)
    codec.sync()
    assert got is out
    assert (canvas[:G] == sent).all() and (canvas[-G:] == sent).all(), "wrote outside the planes"
    assert count.tolist() == [-7, n, -7]
    p = dv.wproject_plan(W, H, n, *win, regressors=8, n_cu=cus)
    want, _ = wr.wproject(s.images, w, *win, segments=p["segments"], fps=p["frames_per_segment"])
    wg.assert_bits(planes, want, "R = 11")
    for r in range(R):
        one, _ = codec.project_weighted(s.buf, s.lead, s.total, s.offs, W, H, n, wg.strided(w[r:r + 1]), *win)
        codec.sync()
        assert torch.equal(one.out[0].view(torch.int32), planes[r].view(torch.int32)), r
    # a call of 3 regressors into the middle of the canvas leaves the planes on either side alone
    canvas.fill_(sent)
    mid = dv.WeightedProjection(planes[4:7], count[1:2])
    codec.project_weighted(s.buf, s.lead, s.total, s.offs, W, H, n, wg.strided(w[4:7]), *win, out=mid)
    codec.sync()
    wg.assert_bits(planes[4:7], want[4:7], "planes 4..6")
    assert (canvas[:G + 4 * rh * rw] == sent).all() and (canvas[G + 7 * rh * rw:] == sent).all()


def test_argument_errors(dv, codec, streams):
    import torch
    W, H = 72, 40
    s, _ = streams(W, H)
    L, h = codec.L, codec.h
    w = torch.ones((9, 16), dtype=torch.float32, device="cuda")
    out = torch.zeros((9, H, W), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")

    def rc(n=13, x=0, y=0, rw=W, rh=H, wp=None, R=2, stride=16, acc=0, flags=0, op=None, cp=None):
        return L.dbde_hip_project_weighted(h, s.buf.data_ptr() + s.lead, s.total, s.offs.data_ptr(), W, H, n, x, y, rw, rh,
                                           w.data_ptr() if wp is None else wp, R, stride, acc, flags,
                                           out.data_ptr() if op is None else op, cnt.data_ptr() if cp is None else cp,
                                           None)
    assert rc() == dv.OK
    for kw in (dict(R=0), dict(R=9), dict(stride=12), dict(flags=2), dict(flags=-1), dict(wp=w.data_ptr() + 2),
               dict(op=out.data_ptr() + 1), dict(cp=cnt.data_ptr() + 4), dict(x=70, rw=8), dict(rh=0), dict(n=-1)):
        assert rc(**kw) == dv.ERR_ARG, kw
    for name in ("wp", "op", "cp"):
        fn = L.dbde_hip_project_weighted
        args = [h, s.buf.data_ptr() + s.lead, s.total, s.offs.data_ptr(), W, H, 13, 0, 0, W, H, w.data_ptr(), 2, 16, 0, 0,
                out.data_ptr(), cnt.data_ptr(), None]
        args[{"wp": 11, "op": 16, "cp": 17}[name]] = None
        assert fn(*args) == dv.ERR_ARG, name
    codec.sync()
    with pytest.raises(ValueError):
        codec.project_weighted(s.buf, s.lead, s.total, s.offs, W, H, 13, w[:, :5])                 # fewer columns than n
    with pytest.raises(ValueError):
        codec.project_weighted(s.buf, s.lead, s.total, s.offs, W, H, 13, w.t().contiguous().t())   # frames not unit-stride
    with pytest.raises(ValueError):
        codec.project_weighted(s.buf, s.lead, s.total, s.offs, W, H, 13, w, accumulate=True)       # nothing to continue


# ---- regressors.py ------------------------------------------------------------------------------------------

def test_pearson_against_numpy(dv, codec):
    """A float64 host formula on the kernels' sums, against numpy's float64 correlation to 1e-9 relative.  The tiny
    recording has small integer weights, so every F32 partial sum is an exact integer below 2^24 and the planes carry
    no rounding of their own; one frame is rejected and must not count."""
    import torch
    reg = import_module("dbde_video_cpp_amd.regressors")
    W, H, n = 72, 40, 24
    s = wg.crafted_stream(np.random.default_rng(2), W, H, n, 8, bad=(7,))
    win = (3, 5, 41, 27)
    w = np.random.default_rng(3).integers(-8, 9, (3, n)).astype(np.float32)
    w[2] = np.arange(n) - 11
    assert 8 * 255 * n < 2 ** 24
    wd = wg.strided(w)
    wp, res = codec.project_weighted(s.buf, s.lead, s.total, s.offs, W, H, n, wd, *win)
    pr, _ = codec.project(s.buf, s.lead, s.total, s.offs, W, H, n, *win, stats=("sum", "sumsq"))
    codec.sync()
    got = reg.pearson(wp, pr, wd, res).cpu().numpy()
    assert got.dtype == np.float64 and got.shape == (3, 27, 41)
    keep = [f for f in range(n) if s.images[f] is not None]
    assert len(keep) == n - 1
    px = np.stack([s.images[f][5:32, 3:44] for f in keep]).astype(np.float64)
    xm = px - px.mean(0)
    var = (xm * xm).sum(0)
    assert (var > 0).any()
    for r in range(3):
        wm = w[r, keep].astype(np.float64)
        wm = wm - wm.mean()
        with np.errstate(all="ignore"):
            want = np.einsum("f,fyx->yx", wm, xm) / np.sqrt((wm * wm).sum() * var)
        assert np.array_equal(np.isnan(got[r]), var == 0), "NaN exactly where a pixel never varies"
        ok = var > 0
        assert np.allclose(got[r][ok], want[ok], rtol=1e-9, atol=1e-12)
        assert np.abs(got[r][ok]).max() <= 1.0 + 1e-9
    const = torch.full((1, n), 3.0, dtype=torch.float32, device="cuda")        # a constant regressor: variance 0 -> NaN
    cw, cres = codec.project_weighted(s.buf, s.lead, s.total, s.offs, W, H, n, const, *win)
    codec.sync()
    assert torch.isnan(reg.pearson(cw, pr, const, cres)).all()


def test_regress_file_in_three_batches(dv, codec, tmp_path):
    """A written file of 13 frames in batches of 5: the planes are the reference chain with those batch boundaries
    (+0.0 planes, then one accumulating call per batch)."""
    import torch
    reg = import_module("dbde_video_cpp_amd.regressors")
    W, H, n, batch = 72, 40, 13, 5
    imgs = codec.synth_frames("mixed", 77, 0, n, W, H)
    path = str(tmp_path / "r.dbde")
    with codec.open_writer(path, W, H, frame_hz=30.0, batch_frames=4) as wtr:
        wtr.put(imgs, n)
    host = list(imgs.cpu().numpy())
    w = np.concatenate([reg.fourier(n, 6.5, 1).numpy(), reg.trend(n).numpy(), reg.ema(n, 0.2).numpy()])
    wd = torch.from_numpy(w).cuda()
    for window in (None, (3, 5, 41, 27)):
        win = (0, 0, W, H) if window is None else window
        out, res = reg.regress_file(codec, path, wd, batch=batch, window=window)
        want = np.zeros((4, win[3], win[2]), np.float32)
        for a in range(0, n, batch):
            want, _ = wr.wproject(host[a:a + batch], w[:, a:a + batch], *win, accumulate=True, prior=want)
        wg.assert_bits(out.out, want, f"regress_file {window}")
        assert int(out.count.item()) == n and tuple(res.shape) == (n, 4)
        assert res[:, 1].tolist() == list(range(n))
