"""GPU: weighted temporal projections of DBDE16 streams -- dbde16_hip_project_weighted (Codec.project_weighted16).

test_gpu_wproject.py's checks with U16 pixels: every plane bit for bit against tests/wproject_ref.py's chain over the
DBDE16 oracle's decode of encoded batches (Batch16 holds it equal to dbde16_hip_decode_frames') and over
tests/crafted.py's numpy decoder for crafted frames.
"""
import numpy as np
import pytest

import wproject_gpu as wg
import wproject_ref as wr
from test_gpu_roi16 import Batch16, images16
from test_oracle_u16 import o16   # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

# edge tiles in both directions, and a frame wider than one piece of 16 tiles (264 > 128 pixels)
SHAPES = [(72, 40), (100, 50), (264, 16)]
COUNTS = (1, 3, 4, 5, 13)
REGRESSORS = (1, 2, 3, 8)
NMAX = 13


def windows(W, H):
    out = [(0, 0, W, H), (3, 5, 41, min(27, H - 5)), (W // 2 + 1, H - 2, 1, 1)]
    if W > 128:
        out.append((123, 1, 13, H - 2))
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


def stream_of(codec, o16, imgs, shift=0):   # noqa: F811
    b = Batch16(codec, o16, imgs, shift=shift)
    assert all(np.array_equal(a, g) for a, g in zip(b.full, b.gpu_full))
    return wg.Stream(b.buf, b.lead, b.total, b.offs, b.W, b.H, b.full)


@pytest.fixture(scope="module")
def streams(codec, o16):   # noqa: F811
    cache = {}

    def get(W, H, n=NMAX, kind="mixed"):
        if (W, H, n, kind) not in cache:
            rng = np.random.default_rng(W * 7919 + H * 31 + n)
            cache[(W, H, n, kind)] = stream_of(codec, o16, images16(rng, n, W, H, kind), shift=len(cache) % 4)
        return cache[(W, H, n, kind)]
    return get


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("W,H", SHAPES)
def test_matches_the_reference_chain(dv, codec, cus, streams, W, H, n):
    s = streams(W, H).first(n)
    rng = np.random.default_rng(W * 31 + n + 16)
    i = 0
    for win in windows(W, H):
        for R in REGRESSORS:
            fam = wg.FAMILIES[(i + 2) % len(wg.FAMILIES)]
            _, res, p = wg.check(codec.project_weighted16, dv.wproject16_plan, cus, s, wg.family(rng, fam, R, n), win,
                                 one_segment=bool(i & 1), what=fam)
            assert p["segments"] == 1
            assert [r[1] for r in codec.parse_results(res)] == list(range(n))
            i += 1
    if W > 128:
        assert dv.wproject16_plan(W, H, n)["pieces_x"] > 1


@pytest.mark.parametrize("kind", ["full", "small", "depth0", "depth16"])
def test_other_frame_contents(dv, codec, cus, streams, kind):
    W, H, n = 100, 50, 5
    s = streams(W, H, n, kind)
    rng = np.random.default_rng(7)
    for win in windows(W, H)[:2]:
        wg.check(codec.project_weighted16, dv.wproject16_plan, cus, s, wg.family(rng, "normal", 3, n), win, what=kind)


@pytest.mark.parametrize("n,S", [(50, 2), (70, 3)])
def test_segments_combine_in_ascending_order(dv, codec, cus, streams, n, S):
    W, H = 72, 40
    s = streams(W, H, 70, "full").first(n)
    rng = np.random.default_rng(n)
    for win in [(0, 0, W, H), (3, 5, 41, 27)]:
        for R in (1, 3, 8):
            w = wg.family(rng, "normal", R, n)
            seg, _, p = wg.check(codec.project_weighted16, dv.wproject16_plan, cus, s, w, win, what="segments")
            assert p["segments"] == S and p["workspace_bytes"] > 0
            one, _, p1 = wg.check(codec.project_weighted16, dv.wproject16_plan, cus, s, w, win, one_segment=True)
            assert p1["segments"] == 1
            assert not np.array_equal(wr.bits(seg.out.cpu().numpy()), wr.bits(one.out.cpu().numpy()))


def test_fma_witnesses_at_a_known_pixel_and_frame(dv, codec, cus, o16):   # noqa: F811
    """Frames 0 and 1 hold 65535 at (py, px); w = -1 then 1 + 2^-23: fmaf(w, 65535, -65535) is 65535 * 2^-23, a multiply
    followed by an add gives 2^-7."""
    W, H, n, py, px = 72, 40, 5, 21, 66
    ww, p, acc = wr.WITNESS_U16
    rng = np.random.default_rng(12)
    imgs = rng.integers(0, 65536, (n, H, W)).astype(np.uint16)
    imgs[0, py, px] = imgs[1, py, px] = p
    s = stream_of(codec, o16, imgs)
    for R in (1, 8):
        w = wg.family(rng, "normal", R, n)
        w[:, 0], w[:, 1] = -1.0, ww
        out, _, _ = wg.check(codec.project_weighted16, dv.wproject16_plan, cus, s.first(2), w[:, :2], (0, 0, W, H))
        got = out.out[:, py, px].cpu().numpy()
        assert (got == wr.fmaf_libm(ww, p, acc)).all() and (got != wr.mul_then_add(ww, p, acc)).all()
        wg.check(codec.project_weighted16, dv.wproject16_plan, cus, s, w, (3, 5, 67, 27), what="witness, longer chain")


def test_all_ones_equals_the_integer_sum(codec, streams):
    """n * 65535 < 2^24 for n = 13: the plane equals Codec.project16's sum."""
    import torch
    for W, H in SHAPES:
        s = streams(W, H, NMAX, "full" if W == 72 else "mixed")
        assert s.n * 65535 < 2 ** 24
        for win in windows(W, H):
            w = torch.ones(s.n, dtype=torch.float32, device="cuda")          # 1-D: one regressor
            out, _ = codec.project_weighted16(s.buf, s.lead, s.total, s.offs, W, H, s.n, w, *win)
            pr, _ = codec.project16(s.buf, s.lead, s.total, s.offs, W, H, s.n, *win, stats=("sum",))
            codec.sync()
            assert tuple(out.out.shape) == (1, win[3], win[2])
            assert torch.equal(out.out[0].to(torch.int64), pr.sum) and torch.equal(out.count, pr.count)


def test_rejected_frames_add_nothing_and_their_weights_are_unused(dv, codec, cus):
    import torch
    W, H, n = 72, 40, 13
    bad = (0, 5, 6, 12)
    s = wg.crafted_stream(np.random.default_rng(15), W, H, n, 16, bad)
    rng = np.random.default_rng(16)
    for win in windows(W, H):
        for R in (1, 3, 8):
            w = wg.family(rng, "normal", R, n)
            w[:, list(bad)] = np.nan
            out, res, _ = wg.check(codec.project_weighted16, dv.wproject16_plan, cus, s, w, win, what="crafted")
            assert torch.isfinite(out.out).all()
            pr, want_res = codec.project16(s.buf, s.lead, s.total, s.offs, W, H, n, *win, stats=("sum",))
            codec.sync()
            assert torch.equal(res, want_res) and int(out.count.item()) == int(pr.count.item()) == n - len(bad)


def test_every_frame_rejected(dv, codec, cus):
    import torch
    W, H, n = 72, 40, 6
    s = wg.crafted_stream(np.random.default_rng(18), W, H, n, 16, bad=range(n))
    w = np.full((2, n), np.nan, np.float32)
    win = (3, 5, 41, 27)
    out, _, _ = wg.check(codec.project_weighted16, dv.wproject16_plan, cus, s, w, win, what="all rejected")
    assert (out.out.view(torch.int32) == 0).all() and int(out.count.item()) == 0
    prior = torch.from_numpy(wg.family(np.random.default_rng(9), "e30", 2, 41 * 27)).cuda().view(2, 27, 41)
    out = dv.WeightedProjection(prior.clone(), torch.full((1,), 5, dtype=torch.int64, device="cuda"))
    codec.project_weighted16(s.buf, s.lead, s.total, s.offs, W, H, n, wg.strided(w), *win, out=out, accumulate=True)
    codec.sync()
    assert torch.equal(out.out.view(torch.int32), prior.view(torch.int32)) and int(out.count.item()) == 5


def test_accumulate_and_guard_bands(dv, codec, cus, streams):
    """Two consecutive calls into planes inside a sentinel canvas, R = 11: the reference's prior + P chain, nothing
    outside the planes written, n == 0 a no-op."""
    import torch
    W, H, n, cut = 100, 50, 13, 5
    s = streams(W, H)
    win = (3, 5, 41, 27)
    rw, rh = win[2], win[3]
    R, G = 11, 64
    w = wg.family(np.random.default_rng(4), "normal", R, n)
    sent = int(np.array([wg.SENT_BITS], np.uint32).view(np.int32)[0])
    canvas = torch.full((G + R * rh * rw + G,), sent, dtype=torch.int32, device="cuda")
    planes = canvas[G: G + R * rh * rw].view(torch.float32).view(R, rh, rw)
    out = dv.WeightedProjection(planes, torch.zeros(1, dtype=torch.int64, device="cuda"))
    codec.project_weighted16(s.buf, s.lead, s.total, s.offs, W, H, cut, wg.strided(w[:, :cut]), *win, out=out)
    codec.sync()
    first, _ = wr.wproject(s.images[:cut], w[:, :cut], *win)
    wg.assert_bits(planes, first, "first call")
    codec.project_weighted16(s.buf, s.lead, s.total, s.offs[cut:], W, H, n - cut, wg.strided(w[:, cut:]), *win, out=out,
                             accumulate=True)
    codec.sync()
    want, _ = wr.wproject(s.images[cut:], w[:, cut:], *win, accumulate=True, prior=first)
    wg.assert_bits(planes, want, "second call")
    assert int(out.count.item()) == n
    assert (canvas[:G] == sent).all() and (canvas[-G:] == sent).all(), "wrote outside the planes"
    codec.project_weighted16(s.buf, s.lead, s.total, s.offs, W, H, 0, wg.strided(w), *win, out=out, accumulate=True)
    codec.sync()
    wg.assert_bits(planes, want, "n == 0")
    assert int(out.count.item()) == n
