"""GPU: DBDE16 temporal projections -- dbde16_hip_project (Codec.project16).

Expected values are int64 reductions over two decodes of the same frames: the DBDE16 oracle's
(dbde16_oracle_unpack_image, test_oracle_u16.unpack16) and dbde16_hip_decode_frames'.  Crafted frames (tests/crafted.py,
bits=16: wrapping U16 minima, rejected frames) are reduced from the numpy decoder's images, and their results rows are
compared with what dbde16_hip_decode_frames reports.
"""
import numpy as np
import pytest

import crafted as cr
from family_refs import reduce16
from test_gpu_roi16 import KINDS, Batch16, images16
from test_oracle_u16 import o16, unpack16   # noqa: F401  (fixture + helper)

pytestmark = pytest.mark.gpu

ALL = ("max", "min", "sum", "sumsq")
GUARD = 40          # bytes of 0x5A on either side of every output
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


def values(t):
    """A projection output as int64 numpy: max / min int16 tensors hold U16 bits."""
    import torch
    a = t.cpu()
    if a.dtype == torch.int16:
        return a.numpy().view(np.uint16).astype(np.int64)
    return a.numpy().astype(np.int64)


def assert_projection(pr, want, stats=ALL, what=""):
    assert int(pr.count.item()) == want["count"], (what, int(pr.count.item()), want["count"])
    for s in ALL:
        got = getattr(pr, s)
        if s not in stats:
            assert got is None, (what, s)
            continue
        g, e = values(got), np.asarray(want[s], np.int64)
        if not np.array_equal(g, e):
            bad = tuple(np.argwhere(g != e)[0])
            raise AssertionError(f"{what}: {s} differs at {bad}: {g[bad]} != {e[bad]}")


def project(codec, b, x, y, rw, rh, **kw):
    pr, res = codec.project16(b.buf, b.lead, kw.pop("stream_bytes", b.total), kw.pop("offs", b.offs), b.W, b.H,
                              kw.pop("n", b.n), x, y, rw, rh, **kw)
    codec.sync()
    return pr, res


def check_both(codec, b, x, y, rw, rh, what):
    pr, res = project(codec, b, x, y, rw, rh)
    assert_projection(pr, reduce16(b.full, x, y, rw, rh), what=f"{what} vs oracle")
    assert_projection(pr, reduce16(b.gpu_full, x, y, rw, rh), what=f"{what} vs decode_frames16")
    assert codec.parse_results(res) == [(2, b.first + f, 0, len(b.packed[f])) for f in range(b.n)]


def windows16(W, H):
    out = [(0, 0, W, H), (W - 1, H - 1, 1, 1), (W // 2, 0, 1, H), (0, H // 3, W, 1)]
    if W > 3 and H > 3:
        out.append((1 + W // 7, 1 + H // 5, max(1, W // 2 - 1), max(1, H // 2 - 1)))
    if W > 20 and H > 10:
        out.append((3, 5, W - 9, H - 7))
    return out


GEOMETRIES = [(1, 1, 3), (10, 10, 3), (33, 31, 3), (200, 123, 2), (7, 300, 2), (1024, 40, 2), (4104, 16, 2),
              (4096, 3072, 2)]


@pytest.mark.parametrize("W,H,n", GEOMETRIES)
def test_kinds_and_geometries(codec, o16, W, H, n):
    rng = np.random.default_rng(W * 7919 + H * 31 + n)
    for i, kind in enumerate(KINDS):
        b = Batch16(codec, o16, images16(rng, n, W, H, kind), first=3 + i, shift=i)
        wins = windows16(W, H)
        if W > 4096:   # across the 512-tile index piece boundary
            wins.append((4090, 1, W - 4090, H - 1))
        for k, win in enumerate(wins):
            if k < 2 or k % len(KINDS) == i or W * H < 100000:
                check_both(codec, b, *win, what=f"{kind} {W}x{H} {win}")


@pytest.mark.parametrize("stats", [("max",), ("min",), ("sum",), ("sumsq",), ("max", "min"), ("min", "sumsq"), ALL])
def test_statistic_subsets_touch_only_their_buffers(dv, codec, o16, stats):
    """Every output sits in a 0x5A5A guard canvas, the U16 ones at 2 mod 4 byte addresses; requested outputs are
    written inside their window only, the others never."""
    import torch
    W, H, n = 200, 123, 4
    b = Batch16(codec, o16, images16(np.random.default_rng(17), n, W, H, "mixed"), shift=5)
    x, y, rw, rh = 5, 3, 131, 77
    P = rw * rh
    size = {"max": 2, "min": 2, "sum": 8, "sumsq": 8}
    canv = {s: torch.full((2 * GUARD + 2 + size[s] * P,), SENTINEL, dtype=torch.uint8, device="cuda") for s in ALL}
    views = {}
    for s in ALL:
        lo = GUARD + (2 if size[s] == 2 else 0)   # U16 outputs at 2 mod 4 (the canvases are 256-byte aligned)
        assert (canv[s].data_ptr() + lo) % 4 == (2 if size[s] == 2 else 0)
        views[s] = canv[s][lo: lo + size[s] * P].view(torch.int16 if size[s] == 2 else torch.int64).view(rh, rw)
    count = torch.full((3,), -7, dtype=torch.int64, device="cuda")
    out = dv.Projection(*[views[s] if s in stats else None for s in ALL], count=count[1:2])
    pr, _ = codec.project16(b.buf, b.lead, b.total, b.offs, W, H, n, x, y, rw, rh, out=out)
    codec.sync()
    assert pr is out
    assert count[0].item() == -7 and count[2].item() == -7
    assert_projection(pr, reduce16(b.full, x, y, rw, rh), stats, what=str(stats))
    for s in ALL:
        c = canv[s].cpu().numpy()
        if s not in stats:
            assert (c == SENTINEL).all(), f"{s} was not requested but written"
        else:
            lo = GUARD + (2 if size[s] == 2 else 0)
            hi = lo + size[s] * P
            assert (c[:lo] == SENTINEL).all() and (c[hi:] == SENTINEL).all(), f"{s}: wrote outside its window"


@pytest.mark.parametrize("slot", [False, True])
@pytest.mark.parametrize("shift", range(16))
def test_layouts_and_stream_bases(codec, o16, slot, shift):
    """Concatenated and slotted streams whose base sits at every residue mod 16; stream_bytes ends exactly at the last
    frame's last byte, with junk behind it."""
    W, H, n = 203, 45, 3
    rng = np.random.default_rng(500 + shift + 50 * slot)
    stride = 0
    if slot:
        stride = (int(codec.L.dbde16_hip_max_frame_bytes(W, H)) + 255) // 256 * 256 + 24
    b = Batch16(codec, o16, images16(rng, n, W, H, "full" if shift % 2 else "mixed"), first=1, slot_stride=stride,
                shift=shift, junk=0x5A + shift)
    for win in [(0, 0, W, H), (3, 5, 197, 33), (W - 9, H - 3, 9, 3)]:
        check_both(codec, b, *win, what=f"slot={slot} shift={shift} {win}")


class Crafted16:
    """Crafted DBDE16 frames (wrapping minima, arbitrary headers) with one-rule breaks mixed in, in one device buffer."""

    def __init__(self, rng, W, H, n, how="concat", bad_every=3, only_bad=False):
        import torch
        T = cr.tiles(W, H)
        self.frames, self.images = [], []
        for f in range(n):
            fr = cr.craft(rng, W, H, 16, cr.DEPTHS[f % len(cr.DEPTHS)], cr.MINIMA[f % len(cr.MINIMA)],
                          cr.PAYLOADS[f % len(cr.PAYLOADS)])
            if only_bad or (bad_every and f % bad_every == 1):
                fr = cr.break_rule(fr, cr.BREAKS[(f // max(bad_every, 1)) % len(cr.BREAKS)], 16,
                                   tile=int(rng.integers(0, T)))
            _, _, img = cr.decode_frame(fr, W, H, 16)
            self.frames.append(fr)
            self.images.append(img)
        slot = max(len(fr) for fr in self.frames) + 13 if how == "slots" else 0
        buf, self.lead, offs, self.total = cr.layout(self.frames, how, lead=32, slot=slot)
        self.buf = torch.from_numpy(buf).cuda()
        self.offs = torch.from_numpy(offs).cuda()
        self.W, self.H, self.n = W, H, n

    def accepted(self):
        return [im for im in self.images if im is not None]


@pytest.mark.parametrize("W,H,n,how", [(64, 48, 30, "concat"), (200, 123, 23, "residues"), (1921, 17, 9, "slots"),
                                       (8, 8, 70, "offsets")])
def test_crafted_and_rejected_frames(codec, W, H, n, how):
    import torch
    rng = np.random.default_rng(W * 7919 + H + 16)
    s = Crafted16(rng, W, H, n, how)
    assert any(im is None for im in s.images) and any(im is not None for im in s.images)
    _, want_res = codec.decode_frames16(s.buf, s.lead, s.total, s.offs, W, H, n)
    for win in windows16(W, H):
        pr, res = project(codec, s, *win)
        assert_projection(pr, reduce16(s.accepted(), *win), what=f"crafted {W}x{H} {win}")
        assert torch.equal(res, want_res)


def test_wrapping_minima_reduce_as_decoded_values(codec):
    """Every tile at a maximal or boundary minimum with a full payload: min + value wraps modulo 2^16."""
    import torch
    rng = np.random.default_rng(6)
    W, H, n = 40, 24, 6
    frames = [cr.craft(rng, W, H, 16, "max", "max" if f % 2 else "boundary", "ones" if f % 3 else "random",
                       header=(2, f, 0)) for f in range(n)]
    images = [cr.decode_frame(fr, W, H, 16)[2] for fr in frames]
    assert all(im is not None for im in images)
    buf, lead, offs, total = cr.layout(frames, "concat", lead=32)
    b, o = torch.from_numpy(buf).cuda(), torch.from_numpy(offs).cuda()
    pr, _ = codec.project16(b, lead, total, o, W, H, n)
    codec.sync()
    assert_projection(pr, reduce16(images, 0, 0, W, H), what="wrapping minima")
    assert values(pr.max).max() == 65535 and values(pr.min).min() < 60000


def test_every_frame_rejected_is_the_empty_projection(codec):
    import torch
    rng = np.random.default_rng(8)
    W, H, n = 61, 37, 7
    s = Crafted16(rng, W, H, n, "offsets", only_bad=True)
    assert all(im is None for im in s.images)
    _, want_res = codec.decode_frames16(s.buf, s.lead, s.total, s.offs, W, H, n)
    for win in [(0, 0, W, H), (5, 3, 17, 30)]:
        pr, res = project(codec, s, *win)
        assert_projection(pr, reduce16([], *win[:2], *win[2:]), what="all rejected")
        assert torch.equal(res, want_res)


@pytest.mark.parametrize("W,H,n,win", [(200, 123, 40, (3, 5, 190, 110)), (64, 64, 700, (0, 0, 64, 64)),
                                       (1031, 45, 12, (0, 0, 1031, 45))])
def test_accumulation_splits_equal_one_call(codec, o16, W, H, n, win):
    import torch
    x, y, rw, rh = win
    b = Batch16(codec, o16, images16(np.random.default_rng(n), n, W, H, "full"))
    one, _ = project(codec, b, x, y, rw, rh)
    for cuts in ([1, 8], [n // 2]):
        acc = None
        bounds = [0] + cuts + [n]
        for lo, hi in zip(bounds, bounds[1:]):
            acc, _ = codec.project16(b.buf, b.lead, b.total, b.offs[lo:hi], W, H, hi - lo, x, y, rw, rh, out=acc,
                                     accumulate=acc is not None)
        codec.sync()
        for s in ALL + ("count",):
            assert torch.equal(getattr(acc, s), getattr(one, s)), (cuts, s)
    assert_projection(one, reduce16(b.full, x, y, rw, rh), what="one call")
    again, _ = codec.project16(b.buf, b.lead, b.total, b.offs[:3], W, H, 3, x, y, rw, rh, out=acc)
    codec.sync()
    assert_projection(again, reduce16(b.full[:3], x, y, rw, rh), what="reset")


def test_zero_frames(codec, o16):
    import torch
    W, H = 200, 123
    b = Batch16(codec, o16, images16(np.random.default_rng(2), 4, W, H, "mixed"))
    pr, _ = project(codec, b, 7, 9, 50, 60)
    before = {s: getattr(pr, s).clone() for s in ALL + ("count",)}
    codec.project16(b.buf, b.lead, b.total, b.offs, W, H, 0, 7, 9, 50, 60, out=pr, accumulate=True)
    codec.sync()
    for s in ALL + ("count",):
        assert torch.equal(getattr(pr, s), before[s]), s
    codec.project16(b.buf, b.lead, b.total, b.offs, W, H, 0, 7, 9, 50, 60, out=pr)
    codec.sync()
    assert_projection(pr, reduce16([], 7, 9, 50, 60), what="empty")


def test_multi_segment_launch(dv, codec, o16):
    """Many small frames: several segments and the combine kernel, with and without accumulation."""
    import torch
    W, H, n = 24, 16, 3000
    p = dv.project16_plan(W, H, n, n_cu=codec_cus(codec))
    assert p["segments"] > 1 and p["combine_grid"] > 0, p
    g = torch.Generator(device="cuda").manual_seed(21)
    imgs = torch.randint(-32768, 32768, (n, H, W), dtype=torch.int16, device="cuda", generator=g)
    b = encoded(codec, imgs)
    host = imgs.cpu().numpy().view(np.uint16)
    for win in [(0, 0, W, H), (3, 5, 9, 10)]:
        pr, _ = project(codec, b, *win)
        assert_projection(pr, reduce16(host, *win), what=f"segments {win}")
    acc, _ = project(codec, b, 0, 0, W, H, n=1000)
    codec.project16(b.buf, b.lead, b.total, b.offs[1000:], W, H, n - 1000, out=acc, accumulate=True)
    codec.sync()
    assert_projection(acc, reduce16(host, 0, 0, W, H), what="segments, accumulated")
    pr, _ = project(codec, b, 0, 0, W, H, stats=("sum", "sumsq"))
    f = torch.from_numpy(host.astype(np.float64))
    assert torch.allclose(pr.mean().cpu(), f.mean(0)) and torch.allclose(pr.std().cpu(), f.std(0, unbiased=False))


def codec_cus(codec):
    import torch
    return torch.cuda.get_device_properties(codec.device).multi_processor_count


class encoded:
    """Frames (int16 device tensor (n, H, W) of U16 bits) encoded with encode_frames16, concatenated."""

    def __init__(self, codec, imgs):
        import torch
        n, H, W = imgs.shape
        maxf = int(codec.L.dbde16_hip_max_frame_bytes(W, H))
        self.buf = torch.full((64 + n * maxf + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        self.lead = 64
        self.offs, sizes = codec.encode_frames16(imgs, W, H, n, self.buf, self.lead, n * maxf)
        codec.sync()
        self.total = int(self.offs[-1].item() + sizes[-1].item())
        self.W, self.H, self.n = W, H, n


def test_sumsq_beyond_u32(codec):
    """Two full-scale frames: 2 * 65,535^2 > 2^32 in every pixel's sum of squares."""
    import torch
    W, H, n = 40, 24, 2
    imgs = torch.full((n, H, W), -1, dtype=torch.int16, device="cuda")   # 65535
    imgs[:, 0::8, 0::8] = 0                                              # depth 16 in every tile
    b = encoded(codec, imgs)
    pr, _ = project(codec, b, 0, 0, W, H)
    host = imgs.cpu().numpy().view(np.uint16)
    assert_projection(pr, reduce16(host, 0, 0, W, H), what="two full-scale frames")
    assert int(values(pr.sumsq).max()) == 2 * 65535 ** 2 > 2 ** 32


def test_sum_beyond_u32_in_one_call(dv, codec):
    """More than 65,536 flat 65535 frames of 8x8: the sums pass 2^32 (several U32 segments), the sums of squares 2^48."""
    import torch
    W, H, n = 8, 8, 66000
    assert dv.project16_plan(W, H, n)["segments"] > 1
    imgs = torch.full((n, H, W), -1, dtype=torch.int16, device="cuda")
    b = encoded(codec, imgs)
    pr, _ = project(codec, b, 0, 0, W, H)
    assert int(pr.count.item()) == n
    assert (pr.sum == n * 65535).all() and n * 65535 > 2 ** 32
    assert (pr.sumsq == n * 65535 ** 2).all()
    assert (values(pr.max) == 65535).all() and (values(pr.min) == 65535).all()


def test_two_codecs_at_once(dv, o16):
    import torch
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    c1, c2 = dv.Codec(0, stream=s1), dv.Codec(0, stream=s2)
    try:
        with torch.cuda.stream(s1):
            b1 = Batch16(c1, o16, images16(np.random.default_rng(1), 16, 640, 480, "mixed"))
        with torch.cuda.stream(s2):
            b2 = Batch16(c2, o16, images16(np.random.default_rng(2), 40, 333, 222, "full"))
        torch.cuda.synchronize()
        for _ in range(2):
            with torch.cuda.stream(s1):
                p1, _ = c1.project16(b1.buf, b1.lead, b1.total, b1.offs, 640, 480, 16)
            with torch.cuda.stream(s2):
                p2, _ = c2.project16(b2.buf, b2.lead, b2.total, b2.offs, 333, 222, 40, 10, 10, 300, 200)
            torch.cuda.synchronize()
            assert_projection(p1, reduce16(b1.full, 0, 0, 640, 480), what="codec 1")
            assert_projection(p2, reduce16(b2.full, 10, 10, 300, 200), what="codec 2")
    finally:
        c1.close()
        c2.close()


def test_argument_errors(dv, codec, o16):
    import torch
    W, H = 64, 64
    b = Batch16(codec, o16, images16(np.random.default_rng(3), 2, W, H, "mixed"))
    count = torch.zeros(1, dtype=torch.int64, device="cuda")
    with pytest.raises(dv.DbdeError):   # no statistic
        codec.project16(b.buf, b.lead, b.total, b.offs, W, H, 2, out=dv.Projection(count=count))
    with pytest.raises(dv.DbdeError):   # window outside the frame
        codec.project16(b.buf, b.lead, b.total, b.offs, W, H, 2, 60, 0, 8, 8)
    with pytest.raises(ValueError):     # accumulate without a projection to continue
        codec.project16(b.buf, b.lead, b.total, b.offs, W, H, 2, accumulate=True)
    L, h = codec.L, codec.h
    raw = torch.full((8 * W * H + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
    ptr = b.buf.data_ptr() + b.lead
    odd = raw.data_ptr() + 1
    for mx, mn in [(odd, None), (None, odd), (raw.data_ptr(), odd)]:   # U16 outputs not 2-byte aligned
        assert L.dbde16_hip_project(h, ptr, b.total, b.offs.data_ptr(), W, H, 2, 0, 0, 8, 8, 0, mx, mn, None, None,
                                    count.data_ptr(), None) == dv.ERR_ARG
    assert L.dbde16_hip_project(h, ptr, b.total, b.offs.data_ptr(), W, H, 2, 0, 0, 8, 8, 0, None, None,
                                raw.data_ptr() + 4, None, count.data_ptr(), None) == dv.ERR_ARG   # U64 unaligned
    assert L.dbde16_hip_project(h, ptr, b.total, b.offs.data_ptr(), W, H, 2, 0, 0, 8, 8, 0, None, None, None, None,
                                count.data_ptr(), None) == dv.ERR_ARG                              # no statistic
    assert L.dbde16_hip_project(h, ptr, b.total, b.offs.data_ptr(), W, H, 2, 0, 0, 8, 8, 0, raw.data_ptr(), None,
                                None, None, None, None) == dv.ERR_ARG                              # no count
    codec.sync()
    assert (raw.cpu().numpy() == SENTINEL).all()
