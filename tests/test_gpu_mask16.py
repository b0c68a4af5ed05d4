"""GPU: threshold mask decode of DBDE16 streams -- dbde16_hip_decode_mask (Codec.decode_mask16).

As tests/test_gpu_mask.py with U16 pixels: expected values are tests/mask_ref.py's definition over the images
dbde16_hip_decode_frames writes for the same frames (for crafted frames: crafted.decode_image's), compared exactly, in
guarded outputs whose words start at 8 mod 16.
"""
import numpy as np
import pytest

import crafted as cr
import mask_ref as mr
from test_gpu_mask import SHAPES, Out, Stream, compare, dev, edge_thresholds, mask_windows, maps_for, run
from test_gpu_project16 import Crafted16
from test_gpu_roi16 import images16

pytestmark = pytest.mark.gpu

CALL = "decode_mask16"
TOP = 65535


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


class Batch16:
    """n DBDE16 frames encoded on the device and dbde16_hip_decode_frames' images and results of them."""

    def __init__(self, codec, kind, W, H, n, seed=0):
        import torch
        imgs_h = images16(np.random.default_rng(W * 31 + H + n + seed), n, W, H, kind)
        cap = n * int(codec.L.dbde16_hip_max_frame_bytes(W, H))
        self.lead = 48 + 3
        self.buf = torch.full((self.lead + cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        imgs = torch.from_numpy(imgs_h.view(np.int16)).cuda()
        self.offs, sizes = codec.encode_frames16(imgs, W, H, n, self.buf, self.lead, cap)
        codec.sync()
        self.total = int((self.offs[-1] + sizes[-1]).item())
        back, self.results = codec.decode_frames16(self.buf, self.lead, self.total, self.offs, W, H, n)
        codec.sync()
        self.dev_images = back
        self.images = back.cpu().numpy().view(np.uint16)
        assert np.array_equal(self.images, imgs_h)


@pytest.mark.parametrize("kind", ("mixed", "full"))
@pytest.mark.parametrize("W,H,n", SHAPES)
def test_windows_scalars_and_maps_in_both_modes(dv, codec, kind, W, H, n):
    import torch
    b = Batch16(codec, kind, W, H, n)
    lo_map, hi_map = maps_for(b.images, W + H, TOP)
    d_lo, d_hi = dev(lo_map), dev(hi_map)
    s_lo, s_hi = (300, 40000) if kind == "full" else (int(np.percentile(b.images, 30)), int(np.percentile(b.images, 70)))
    for k, win in enumerate(mask_windows(W, H)):
        outside = bool(k & 1)
        what = f"{kind} {W}x{H} window {win}"
        got, res = run(dv, codec, b, W, H, n, win, s_lo, s_hi, outside, call=CALL, what=what + " scalars")
        compare(got, b.images, win, s_lo, s_hi, outside, what=what + " scalars")
        assert torch.equal(res, b.results)
        got, res = run(dv, codec, b, W, H, n, win, d_lo, d_hi, not outside, call=CALL, what=what + " maps")
        compare(got, b.images, win, lo_map, hi_map, not outside, what=what + " maps")
        assert torch.equal(res, b.results)


def test_one_map_and_one_scalar(dv, codec):
    W, H, n = 200, 123, 4
    b = Batch16(codec, "mixed", W, H, n)
    lo_map, hi_map = maps_for(b.images, 3, TOP)
    for win in mask_windows(W, H)[:3] + [(67, 11, 129, 40)]:
        for lo, hi in ((lo_map, 50000), (700, hi_map), (lo_map, None), (None, hi_map)):
            for outside in (False, True):
                what = f"{win} lo {type(lo).__name__} hi {type(hi).__name__} outside {outside}"
                got, _ = run(dv, codec, b, W, H, n, win, lo, hi, outside, call=CALL, what=what)
                compare(got, b.images, win, 0 if lo is None else lo, TOP if hi is None else hi, outside, what=what)


@pytest.mark.parametrize("kind", ("mixed", "full"))
def test_wide_frame_pieces_and_seams(dv, codec, kind):
    """4200 x 24, window (3, 1, 4190, 20): 66 words in 5 pieces of 14 (128 threads), seams inside tiles (x0 = 3)."""
    W, H, n = 4200, 24, 2
    plan = dv.mask16_plan(W, H, n, 3, 1, 4190, 20)
    assert plan["pieces_x"] == 5 and plan["threads"] == 128
    b = Batch16(codec, kind, W, H, n)
    lo_map, hi_map = maps_for(b.images, 42, TOP)
    s_lo, s_hi = int(np.percentile(b.images, 25)), int(np.percentile(b.images, 75))
    for win in ((3, 1, 4190, 20), (0, 0, W, H), (8, 0, 4096, 24), (5, 3, 2049, 9)):
        for outside in (False, True):
            got, _ = run(dv, codec, b, W, H, n, win, s_lo, s_hi, outside, call=CALL)
            compare(got, b.images, win, s_lo, s_hi, outside, what=f"{kind} {win} scalars")
            got, _ = run(dv, codec, b, W, H, n, win, lo_map, hi_map, outside, call=CALL)
            compare(got, b.images, win, lo_map, hi_map, outside, what=f"{kind} {win} maps")
    org = np.array([[3, 1], [-7, 9]], np.int32)
    got, _ = run(dv, codec, b, W, H, n, (0, 0, 4190, 20), lo_map, 40000, False, origins=org, call=CALL)
    compare(got, b.images, (0, 0, 4190, 20), lo_map, 40000, False, origins=org, what="4200x24 origins")


@pytest.mark.parametrize("W,H,n,rw,rh", [(200, 123, 9, 61, 37), (200, 123, 9, 129, 20), (1921, 1081, 8, 700, 9)])
def test_per_frame_origins(dv, codec, W, H, n, rw, rh):
    import torch
    rng = np.random.default_rng(W + rw + 16)
    b = Batch16(codec, "mixed", W, H, n)
    lo_map, hi_map = maps_for(b.images, 23, TOP)
    org = np.stack([rng.integers(-9, W + 9, n), rng.integers(-9, H + 9, n)], 1).astype(np.int32)
    org[:8, 0] = np.minimum(np.arange(8) + 8 * rng.integers(0, 4, 8), W - rw)
    org[0] = (-5, H + 100)
    org[1] = (W + 50, -3)
    s_lo, s_hi = int(np.percentile(b.images, 30)), int(np.percentile(b.images, 70))
    for lo, hi, outside in ((lo_map, hi_map, False), (s_lo, s_hi, True), (lo_map, TOP, True)):
        got, res = run(dv, codec, b, W, H, n, (0, 0, rw, rh), lo, hi, outside, origins=org, call=CALL)
        compare(got, b.images, (0, 0, rw, rh), lo, hi, outside, origins=org, what=f"{W}x{H} origins {rw}x{rh}")
        assert torch.equal(res, b.results)


def test_decided_tile_edges_on_every_depth_and_boundary_minimum(dv, codec):
    rng = np.random.default_rng(2026)
    W, H = 320, 280
    T = cr.tiles(W, H)
    frames = [cr.all_pairs_frame(rng, "ones", perm="random", T=T, bits=16),
              cr.all_pairs_frame(rng, "zeros", perm="random", T=T, bits=16),
              cr.all_pairs_frame(rng, "random", perm="random", T=T, bits=16),
              cr.craft(rng, W, H, 16, "random", "boundary", "ones", header=(2, 3, 0)),
              cr.craft(rng, W, H, 16, "random", "boundary", "zeros", header=(2, 4, 0))]
    s = Stream(frames, W, H, 16)
    n = len(frames)
    assert (s.minima + (1 << s.depths) - 1 > TOP).any()
    win = (0, 0, W, H)
    for t in edge_thresholds(s, rng, TOP):
        for lo, hi in ((t, TOP), (0, t)):
            for outside in (False, True):
                what = f"all pairs lo {lo} hi {hi} outside {outside}"
                got, _ = run(dv, codec, s, W, H, n, win, lo, hi, outside, call=CALL, what=what)
                compare(got, s.images, win, lo, hi, outside, what=what)
    for lo, hi, win in ((40000, 100, (0, 0, W, H)), (1, 0, (5, 3, 300, 100)), (TOP, 0, (9, 9, 65, 9)), (256, 511, (3, 0, 317, 280))):
        for outside in (False, True):
            got, _ = run(dv, codec, s, W, H, n, win, lo, hi, outside, call=CALL)
            compare(got, s.images, win, lo, hi, outside, what=f"lo {lo} hi {hi} outside {outside} {win}")
            if lo > hi:
                assert (got[1] == (0 if not outside else win[2] * win[3])).all()


def test_band_from_background_is_the_absolute_difference(dv, codec):
    import torch
    W, H, n = 200, 123, 4
    b = Batch16(codec, "full", W, H, n)
    img = b.dev_images.int() & 0xFFFF
    bg16 = b.dev_images[0].clone()
    bg16[:7, :] = 0
    bg16[-7:, :] = -1      # 65535: clamping at both ends
    bg = bg16.int() & 0xFFFF
    for below, above in ((300, None), (0, None), (1000, 20), (70000, 70000)):
        lo, hi = dv.band_from_background(bg16, below, above)
        assert lo.dtype == torch.int16 and hi.dtype == torch.int16
        m, _ = codec.decode_mask16(b.buf, b.lead, b.total, b.offs, W, H, n, lo=lo, hi=hi, outside=True)
        codec.sync()
        diff = img - bg
        want = (diff < -below) | (diff > (below if above is None else above))
        if above is None:
            assert torch.equal(want, diff.abs() > below)
        assert torch.equal(m.unpack(), want) and torch.equal(m.counts.long(), want.sum((1, 2)))


@pytest.mark.parametrize("W,H,n,how", [(64, 48, 30, "concat"), (200, 123, 23, "residues"), (1921, 17, 9, "slots"),
                                       (8, 8, 70, "offsets")])
def test_crafted_and_rejected_frames(dv, codec, W, H, n, how):
    import torch
    rng = np.random.default_rng(W * 7919 + H + 16)
    s = Crafted16(rng, W, H, n, how)
    keep = [im is not None for im in s.images]
    assert any(keep) and not all(keep)
    canvas = torch.full((n, H, W), 0x3333, dtype=torch.int16, device="cuda")
    images, want_res = codec.decode_frames16(s.buf, s.lead, s.total, s.offs, W, H, n, images=canvas)
    codec.sync()
    images = images.cpu().numpy().view(np.uint16)
    assert all((images[f] == s.images[f]).all() for f in range(n) if keep[f])
    lo_map, hi_map = maps_for(np.stack([im for im in s.images if im is not None]), H, TOP)
    for k, win in enumerate(mask_windows(W, H)[:7]):
        what = f"crafted {how} {W}x{H} {win}"
        lo, hi = ((lo_map, hi_map), (16000, 50000), (lo_map, TOP))[k % 3]
        got, res = run(dv, codec, s, W, H, n, win, lo, hi, bool(k & 1), call=CALL, what=what)
        compare(got, images, win, lo, hi, bool(k & 1), keep=keep, what=what)
        assert torch.equal(res, want_res)


def test_output_subsets_zero_frames_and_errors(dv, codec):
    import torch
    W, H, n = 200, 123, 5
    b = Batch16(codec, "mixed", W, H, n)
    win = (5, 3, 131, 77)
    s_lo, s_hi = int(np.percentile(b.images, 30)), int(np.percentile(b.images, 70))
    for bits, counts, boxes in ((False, True, False), (False, False, True), (True, False, False)):
        got, _ = run(dv, codec, b, W, H, n, win, s_lo, s_hi, False, call=CALL, bits=bits, counts=counts, boxes=boxes)
        compare(got, b.images, win, s_lo, s_hi, False, what=f"subset {bits} {counts} {boxes}")
    m, _ = codec.decode_mask16(b.buf, b.lead, b.total, b.offs, W, H, n, *win, lo=s_lo, hi=s_hi, boxes=True)
    codec.sync()
    up = m.unpack()
    want = mr.verdicts(b.images, *win, s_lo, s_hi)
    assert np.array_equal(up.cpu().numpy(), want) and (up.sum((1, 2)) == m.counts).all()
    assert np.array_equal(m.boxes.cpu().numpy(), mr.boxes(want))
    o = Out(dv, n, 41, 30)
    codec.decode_mask16(b.buf, b.lead, b.total, b.offs, W, H, 0, 5, 3, 41, 30, mask=o.mask)
    codec.sync()
    assert (o.read()[0] == np.uint64(0x5A5A5A5A5A5A5A5A)).all(), "n == 0 wrote the words"
    good = torch.zeros((H, W), dtype=torch.int16, device="cuda")
    for kw in (dict(lo=65536), dict(hi=good.to(torch.uint8)), dict(lo=good[:, :-1])):
        with pytest.raises(dv.DbdeError):
            codec.decode_mask16(b.buf, b.lead, b.total, b.offs, W, H, n, **kw)
    m, res = codec.decode_mask16(b.buf, b.lead, b.total, b.offs, W, H, n, lo=good, hi=65535)
    codec.sync()
    assert (m.counts == W * H).all() and torch.equal(res, b.results)


def test_full_size_frames_on_the_device(dv, codec):
    """4096 x 3072, 2 frames, compared on the device with torch."""
    import torch
    W, H, n = 4096, 3072, 2
    b = Batch16(codec, "mixed", W, H, n)
    img = b.dev_images.int() & 0xFFFF
    s_lo, s_hi = int(np.percentile(b.images[0, ::16, ::16], 30)), int(np.percentile(b.images[0, ::16, ::16], 70))
    lo_map, hi_map = dv.band_from_background(b.dev_images[0], 40, 90)
    for (x, y, rw, rh), lo, hi, outside in (((0, 0, W, H), s_lo, s_hi, False), ((5, 3, 4090, 3000), s_lo, s_hi, True),
                                            ((0, 0, W, H), lo_map, hi_map, True)):
        m, res = codec.decode_mask16(b.buf, b.lead, b.total, b.offs, W, H, n, x, y, rw, rh, lo=lo, hi=hi, outside=outside)
        codec.sync()
        p = img[:, y:y + rh, x:x + rw]
        L = (lo[y:y + rh, x:x + rw].int() & 0xFFFF) if isinstance(lo, torch.Tensor) else lo
        Hh = (hi[y:y + rh, x:x + rw].int() & 0xFFFF) if isinstance(hi, torch.Tensor) else hi
        want = (p >= L) & (p <= Hh)
        want = ~want if outside else want
        assert torch.equal(m.unpack(), want), (x, y, rw, rh)
        assert torch.equal(m.counts.long(), want.sum((1, 2))) and torch.equal(res, b.results)
