"""GPU: temporal projections -- dbde_hip_project (Codec.project).

Expected values are int64 reductions over the images the decoders write for the same frames: dbde_hip_decode_frames
on the device for encoded batches, the numpy decoder of tests/crafted.py for crafted frames (frames no encoder writes:
wrapping minima, broken rules).  Results rows are compared with what dbde_hip_decode_frames reports.
"""
import numpy as np
import pytest

import crafted as cr
from family_refs import reduce_numpy   # noqa: F401  (used here and imported from here)

pytestmark = pytest.mark.gpu

MODES = ("noise8", "mixed", "flat", "smooth")
SEED = 0x9E0_2016
ALL = ("max", "min", "sum", "sumsq")
GUARD = 40
SENTINEL = 0x5A


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


class Batch:
    """n synthetic (or given) frames encoded on the device, and dbde_hip_decode_frames' images of them."""

    def __init__(self, codec, mode, W, H, n, slot_stride=0, misalign=0, images=None):
        import torch
        imgs = codec.synth_frames(mode, SEED, 0, n, W, H) if images is None else images
        buf, lead, cap = codec.alloc_stream(W, H, n, slot_stride=slot_stride, lead=48)
        lead += misalign
        buf.fill_(0xA5)
        offs, sizes = codec.encode_frames(imgs, W, H, n, buf, lead, cap, slot_stride=slot_stride)
        codec.sync()
        o, s = offs.cpu().numpy(), sizes.cpu().numpy()
        self.total = int(o[-1] + s[-1])
        self.images, self.results = codec.decode_frames(buf, lead, self.total, offs, W, H, n)
        codec.sync()
        assert torch.equal(self.images, imgs)
        self.buf, self.lead, self.offs = buf, lead, offs
        self.W, self.H, self.n = W, H, n


def reduce_images(images, x, y, rw, rh, keep=None):
    """int64 reductions of the window over the frames (torch, on the images' device); keep: frames that count."""
    import torch
    win = images[:, y:y + rh, x:x + rw]
    if keep is not None:
        win = win[torch.as_tensor(np.asarray(keep, bool), device=win.device)]
    if win.shape[0] == 0:
        z = torch.zeros((rh, rw), dtype=torch.int64, device=images.device)
        return dict(max=z.clone(), min=z + 255, sum=z.clone(), sumsq=z.clone(), count=0)
    w = win.to(torch.int64)
    return dict(max=w.amax(0), min=w.amin(0), sum=w.sum(0), sumsq=(w * w).sum(0), count=int(win.shape[0]))


def assert_projection(pr, want, stats=ALL, what=""):
    import torch
    assert int(pr.count.item()) == want["count"], (what, int(pr.count.item()), want["count"])
    for s in ALL:
        got = getattr(pr, s)
        if s not in stats:
            assert got is None, (what, s)
            continue
        exp = want[s]
        exp = exp if isinstance(exp, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(exp)).to(got.device)
        g = got.to(torch.int64)
        if not torch.equal(g, exp.to(torch.int64)):
            bad = (g != exp).nonzero()[0].tolist()
            raise AssertionError(f"{what}: {s} differs at {bad}: {int(g[tuple(bad)])} != {int(exp[tuple(bad)])}")


def windows(W, H):
    """Full frame, an unaligned interior window, 1x1, one column, one row, the last row and the last column."""
    out = [(0, 0, W, H), (W // 2, H - 1, 1, 1), (W - 1, 0, 1, H), (0, H // 3, W, 1), (0, H - 1, W, 1)]
    if W > 3 and H > 3:
        out.append((1 + W // 7, 1 + H // 5, max(1, W // 2 - 1), max(1, H // 2 - 3)))
    return out


SHAPES = [(4096, 3072, 16), (1921, 1081, 5), (200, 123, 7), (8, 8, 9), (9, 9, 9), (4200, 24, 5), (8, 262152, 2)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W,H,n", SHAPES)
def test_projection_matches_decoded_images(dv, codec, mode, W, H, n):
    import torch
    b = Batch(codec, mode, W, H, n)
    for (x, y, rw, rh) in windows(W, H):
        pr, res = codec.project(b.buf, b.lead, b.total, b.offs, W, H, n, x, y, rw, rh)
        codec.sync()
        assert_projection(pr, reduce_images(b.images, x, y, rw, rh), what=f"{mode} {W}x{H} {(x, y, rw, rh)}")
        assert torch.equal(res, b.results)


@pytest.mark.parametrize("stats", [("max",), ("min",), ("sum",), ("sumsq",), ("max", "min"), ALL])
@pytest.mark.parametrize("odd", [0, 1, 3])
def test_statistic_subsets_touch_only_their_buffers(dv, codec, stats, odd):
    """Every output sits in a guard canvas; the requested ones are written inside their window only, the others are
    never touched.  U8 outputs at odd byte offsets."""
    import torch
    W, H, n = 200, 123, 7
    b = Batch(codec, "mixed", W, H, n)
    x, y, rw, rh = 5, 3, 131, 77
    P = rw * rh
    canv = {s: torch.full((2 * GUARD + odd + (8 if s in ("sum", "sumsq") else 1) * P,), SENTINEL, dtype=torch.uint8,
                          device="cuda") for s in ALL}
    views = {}
    for s in ALL:
        if s in ("max", "min"):
            views[s] = canv[s][GUARD + odd: GUARD + odd + P].view(rh, rw)
        else:
            views[s] = canv[s][GUARD: GUARD + 8 * P].view(torch.int64).view(rh, rw)
    count = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    out = dv.Projection(*[views[s] if s in stats else None for s in ALL], count=count[1:2])
    pr, _ = codec.project(b.buf, b.lead, b.total, b.offs, W, H, n, x, y, rw, rh, out=out)
    codec.sync()
    assert pr is out
    assert count[0].item() == -7 and count[2].item() == -7
    assert_projection(pr, reduce_images(b.images, x, y, rw, rh), stats, what=str(stats))
    for s in ALL:
        c = canv[s].cpu().numpy()
        if s not in stats:
            assert (c == SENTINEL).all(), f"{s} was not requested but written"
        else:
            lo = GUARD + (odd if s in ("max", "min") else 0)
            hi = lo + (8 if s in ("sum", "sumsq") else 1) * P
            assert (c[:lo] == SENTINEL).all() and (c[hi:] == SENTINEL).all(), f"{s}: wrote outside its window"


@pytest.mark.parametrize("slot,misalign", [(0, 1), (0, 3), (0, 6), (4096 * 3 + 5, 0), (20000, 2)])
def test_layouts(dv, codec, slot, misalign):
    """Concatenated streams at misaligned leads and slot layouts; stream_bytes ends exactly at the last frame."""
    import torch
    W, H, n = 100, 75, 11
    b = Batch(codec, "mixed", W, H, n, slot_stride=slot, misalign=misalign)
    for (x, y, rw, rh) in [(0, 0, W, H), (3, 2, 95, 70)]:
        pr, res = codec.project(b.buf, b.lead, b.total, b.offs, W, H, n, x, y, rw, rh)
        codec.sync()
        assert_projection(pr, reduce_images(b.images, x, y, rw, rh), what=f"slot {slot} misalign {misalign}")
        assert torch.equal(res, b.results)


class Crafted:
    """Crafted frames (wrapping minima, random headers) with one-rule breaks mixed in, laid out in one device buffer."""

    def __init__(self, rng, W, H, n, how="concat", bad_every=3):
        import torch
        T = cr.tiles(W, H)
        self.frames, self.images = [], []
        for f in range(n):
            fr = cr.craft(rng, W, H, 8, cr.DEPTHS[f % len(cr.DEPTHS)], cr.MINIMA[f % len(cr.MINIMA)],
                          cr.PAYLOADS[f % len(cr.PAYLOADS)])
            if bad_every and f % bad_every == 1:
                fr = cr.break_rule(fr, cr.BREAKS[(f // bad_every) % len(cr.BREAKS)], 8, tile=int(rng.integers(0, T)))
            _, _, img = cr.decode_frame(fr, W, H)
            self.frames.append(fr)
            self.images.append(img)
        slot = max(len(fr) for fr in self.frames) + 13 if how == "slots" else 0
        buf, self.lead, offs, self.total = cr.layout(self.frames, how, lead=32, slot=slot)
        self.buf = torch.from_numpy(buf).cuda()
        self.offs = torch.from_numpy(offs).cuda()
        self.W, self.H, self.n = W, H, n

    def accepted(self, lo=0, hi=None):
        return [im for im in self.images[lo:hi] if im is not None]


@pytest.mark.parametrize("W,H,n,how", [(64, 48, 40, "concat"), (200, 123, 23, "residues"), (1921, 17, 9, "slots"),
                                       (8, 8, 70, "offsets"), (4200, 9, 7, "concat")])
def test_crafted_and_rejected_frames(dv, codec, W, H, n, how):
    import torch
    rng = np.random.default_rng(W * 7919 + H)
    s = Crafted(rng, W, H, n, how)
    assert any(im is None for im in s.images) and any(im is not None for im in s.images)
    _, want_res = codec.decode_frames(s.buf, s.lead, s.total, s.offs, W, H, n)
    for (x, y, rw, rh) in windows(W, H):
        pr, res = codec.project(s.buf, s.lead, s.total, s.offs, W, H, n, x, y, rw, rh)
        codec.sync()
        assert_projection(pr, reduce_numpy(s.accepted(), x, y, rw, rh), what=f"crafted {W}x{H} {(x, y, rw, rh)}")
        assert torch.equal(res, want_res)


def test_wrapping_minima_reduce_as_decoded_bytes(dv, codec):
    """Every tile at the maximum minimum with a full payload: min + value wraps modulo 256 in nearly every pixel."""
    rng = np.random.default_rng(5)
    W, H, n = 40, 24, 6
    frames = [cr.craft(rng, W, H, 8, "max", "max" if f % 2 else "boundary", "ones" if f % 3 else "random",
                       header=(2, f, 0)) for f in range(n)]
    images = [cr.decode_frame(fr, W, H)[2] for fr in frames]
    assert all(im is not None for im in images)
    buf, lead, offs, total = cr.layout(frames, "concat", lead=32)
    import torch
    b, o = torch.from_numpy(buf).cuda(), torch.from_numpy(offs).cuda()
    pr, _ = codec.project(b, lead, total, o, W, H, n)
    codec.sync()
    assert_projection(pr, reduce_numpy(images, 0, 0, W, H), what="wrapping minima")
    assert int(pr.max.max()) == 255 and int(pr.min.min()) < 200


@pytest.mark.parametrize("W,H,n,win", [(200, 123, 40, (3, 5, 190, 110)), (64, 64, 1000, (0, 0, 64, 64)),
                                       (1921, 1081, 12, (0, 0, 1921, 1081))])
def test_accumulation_splits_equal_one_call(dv, codec, W, H, n, win):
    import torch
    x, y, rw, rh = win
    b = Batch(codec, "noise8", W, H, n)
    one, _ = codec.project(b.buf, b.lead, b.total, b.offs, W, H, n, x, y, rw, rh)
    for cuts in ([1, 8], [n // 2]):
        acc = None
        bounds = [0] + cuts + [n]
        for lo, hi in zip(bounds, bounds[1:]):
            acc, _ = codec.project(b.buf, b.lead, b.total, b.offs[lo:hi], W, H, hi - lo, x, y, rw, rh, out=acc,
                                   accumulate=acc is not None)
        codec.sync()
        for s in ALL + ("count",):
            assert torch.equal(getattr(acc, s), getattr(one, s)), (cuts, s)
    # accumulate=False after accumulating starts again
    again, _ = codec.project(b.buf, b.lead, b.total, b.offs[:3], W, H, 3, x, y, rw, rh, out=acc)
    codec.sync()
    assert_projection(again, reduce_images(b.images[:3], x, y, rw, rh), what="reset")
    assert_projection(one, reduce_images(b.images, x, y, rw, rh), what="one call")


def test_zero_frames(dv, codec):
    import torch
    W, H = 200, 123
    b = Batch(codec, "mixed", W, H, 4)
    pr, _ = codec.project(b.buf, b.lead, b.total, b.offs, W, H, 4, 7, 9, 50, 60)
    codec.sync()
    before = {s: getattr(pr, s).clone() for s in ALL + ("count",)}
    codec.project(b.buf, b.lead, b.total, b.offs, W, H, 0, 7, 9, 50, 60, out=pr, accumulate=True)
    codec.sync()
    for s in ALL + ("count",):
        assert torch.equal(getattr(pr, s), before[s]), s
    codec.project(b.buf, b.lead, b.total, b.offs, W, H, 0, 7, 9, 50, 60, out=pr)
    codec.sync()
    assert_projection(pr, reduce_images(b.images, 7, 9, 50, 60, keep=[False] * 4), what="empty")


def test_sums_beyond_u32(dv, codec):
    """70,000 frames of 8x8, all 255: every sum of squares is 70,000 * 65,025 = 4,551,750,000 > 2^32."""
    import torch
    n, W, H = 70000, 8, 8
    imgs = torch.full((n, H, W), 255, dtype=torch.uint8, device="cuda")
    b = Batch(codec, None, W, H, n, images=imgs)
    pr, _ = codec.project(b.buf, b.lead, b.total, b.offs, W, H, n)
    codec.sync()
    assert int(pr.count.item()) == n
    assert (pr.sumsq == 4_551_750_000).all() and 4_551_750_000 > 2 ** 32
    assert (pr.sum == 17_850_000).all()
    assert (pr.max == 255).all() and (pr.min == 255).all()


def test_long_random_batch(dv, codec):
    """More than 65,536 random 16x16 frames (several segments and the combine) against the decoded images."""
    import torch
    n, W, H = 66000, 16, 16
    assert dv.project_plan(W, H, n)["segments"] > 1
    g = torch.Generator(device="cuda").manual_seed(11)
    imgs = torch.randint(0, 256, (n, H, W), dtype=torch.uint8, device="cuda", generator=g)
    b = Batch(codec, None, W, H, n, images=imgs)
    for win in [(0, 0, W, H), (3, 5, 9, 10)]:
        pr, _ = codec.project(b.buf, b.lead, b.total, b.offs, W, H, n, *win)
        codec.sync()
        assert_projection(pr, reduce_images(b.images, *win), what=f"long {win}")
    pr, _ = codec.project(b.buf, b.lead, b.total, b.offs, W, H, n, stats=("sum", "sumsq"))
    codec.sync()
    f = b.images.to(torch.float64)
    assert torch.allclose(pr.mean(), f.mean(0)) and torch.allclose(pr.std(), f.std(0, unbiased=False))


def test_two_codecs_at_once(dv):
    """Two contexts on their own streams, each projecting its own batch, queued together."""
    import torch
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    c1, c2 = dv.Codec(0, stream=s1), dv.Codec(0, stream=s2)
    try:
        with torch.cuda.stream(s1):
            b1 = Batch(c1, "mixed", 640, 480, 64)
        with torch.cuda.stream(s2):
            b2 = Batch(c2, "noise8", 333, 222, 200)
        torch.cuda.synchronize()
        for _ in range(3):
            with torch.cuda.stream(s1):
                p1, _ = c1.project(b1.buf, b1.lead, b1.total, b1.offs, 640, 480, 64)
            with torch.cuda.stream(s2):
                p2, _ = c2.project(b2.buf, b2.lead, b2.total, b2.offs, 333, 222, 200, 10, 10, 300, 200)
            torch.cuda.synchronize()
            assert_projection(p1, reduce_images(b1.images, 0, 0, 640, 480), what="codec 1")
            assert_projection(p2, reduce_images(b2.images, 10, 10, 300, 200), what="codec 2")
    finally:
        c1.close()
        c2.close()


def test_argument_errors(dv, codec):
    import torch
    b = Batch(codec, "flat", 64, 64, 2)
    with pytest.raises(dv.DbdeError):   # no statistic
        codec.project(b.buf, b.lead, b.total, b.offs, 64, 64, 2, out=dv.Projection(count=torch.zeros(1, dtype=torch.int64,
                                                                                                    device="cuda")))
    with pytest.raises(dv.DbdeError):   # window outside the frame
        codec.project(b.buf, b.lead, b.total, b.offs, 64, 64, 2, 60, 0, 8, 8)
    with pytest.raises(ValueError):     # accumulate without a projection to continue
        codec.project(b.buf, b.lead, b.total, b.offs, 64, 64, 2, accumulate=True)
