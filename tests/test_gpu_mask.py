"""GPU: threshold mask decode -- dbde_hip_decode_mask (Codec.decode_mask).

Expected values are tests/mask_ref.py's definition over the images dbde_hip_decode_frames writes for the same frames (for
crafted frames: crafted.decode_image's), compared exactly: every word, count and box.  The maps are never constant, so a
kernel that indexed them by window coordinates would fail.  Every output sits in a sentinel-filled buffer whose guards
are checked; the words start at an 8-byte but not 16-byte aligned address.  Results rows are compared with what
dbde_hip_decode_frames reports.
"""
import numpy as np
import pytest

import crafted as cr
import mask_ref as mr
from test_gpu_project import Batch, Crafted

pytestmark = pytest.mark.gpu

GUARD = 5          # words in front of the mask: 40 bytes, so the mask starts at 8 mod 16
SENT64 = 0x5A5A5A5A5A5A5A5A
SENT32 = 0x5A5A5A5A
SHAPES = [(1, 1, 5), (8, 8, 9), (9, 9, 9), (63, 5, 4), (64, 5, 4), (65, 5, 4), (200, 123, 7), (1921, 1081, 2)]


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


class Out:
    """The three outputs of a mask decode, each inside a sentinel-filled buffer with guards on both sides."""

    def __init__(self, dv, n, rw, rh, bits=True, counts=True, boxes=True):
        import torch
        self.n, self.rw, self.rh, self.words = n, rw, rh, (rw + 63) // 64
        self.nw = n * rh * self.words
        self.wbuf = torch.full((2 * GUARD + self.nw,), SENT64, dtype=torch.int64, device="cuda")
        self.cbuf = torch.full((2 * GUARD + n,), SENT32, dtype=torch.int32, device="cuda")
        self.bbuf = torch.full((2 * GUARD + 4 * n,), SENT32, dtype=torch.int32, device="cuda")
        w = self.wbuf[GUARD:GUARD + self.nw].view(n, rh, self.words)
        assert self.wbuf.data_ptr() % 256 == 0 and (self.nw == 0 or w.data_ptr() % 16 == 8)
        self.mask = dv.Mask(w if bits else None, self.cbuf[GUARD:GUARD + n] if counts else None,
                            self.bbuf[GUARD:GUARD + 4 * n].view(n, 4) if boxes else None)
        self.has = (bits, counts, boxes)

    def read(self, what=""):
        """(words uint64 (n, rh, words), counts uint32 (n,), boxes int32 (n, 4)) after checking the guards; an output
        that was not asked for must still be all sentinel and reads as None."""
        out = []
        for buf, cnt, sent, has, shape, dt in ((self.wbuf, self.nw, SENT64, self.has[0], (self.n, self.rh, self.words), np.uint64),
                                               (self.cbuf, self.n, SENT32, self.has[1], (self.n,), np.uint32),
                                               (self.bbuf, 4 * self.n, SENT32, self.has[2], (self.n, 4), np.int32)):
            h = buf.cpu().numpy()
            assert (h[:GUARD] == sent).all(), f"{what}: wrote in front of an output"
            assert (h[GUARD + cnt:] == sent).all(), f"{what}: wrote behind an output"
            if not has:
                assert (h == sent).all(), f"{what}: wrote an output that was not asked for"
            out.append(h[GUARD:GUARD + cnt].view(dt).reshape(shape) if has else None)
        return out


def dev(a):
    """A map (numpy (H, W) uint8 / uint16), a scalar or None as Codec.decode_mask / decode_mask16 takes it."""
    import torch
    if isinstance(a, np.ndarray):
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()
    return a


def run(dv, codec, src, W, H, n, win, lo, hi, outside=False, origins=None, call="decode_mask", what="", **outs):
    """src: anything with .buf, .lead, .total, .offs.  -> ((words, counts, boxes), results)."""
    import torch
    x, y, rw, rh = win
    o = Out(dv, n, rw, rh, **outs)
    org = None if origins is None else torch.from_numpy(np.asarray(origins, np.int32).reshape(n, 2)).cuda()
    m, res = getattr(codec, call)(src.buf, src.lead, src.total, src.offs, W, H, n, x, y, rw, rh, lo=dev(lo), hi=dev(hi),
                                  outside=outside, origins=org, mask=o.mask)
    codec.sync()
    assert m is o.mask and m.rw == rw
    return o.read(what), res


def compare(got, images, win, lo, hi, outside=False, origins=None, keep=None, what=""):
    """got against mask_ref over `images` ((n, H, W), rows of rejected frames arbitrary)."""
    x, y, rw, rh = win
    words, counts, boxes = mr.expected(images, x, y, rw, rh, lo, hi, mr.OUTSIDE if outside else mr.INSIDE, origins)
    gw, gc, gb = got
    for f in range(len(images)):
        if keep is not None and not keep[f]:
            assert gw is None or (gw[f] == np.uint64(SENT64)).all(), f"{what}: rejected frame {f}'s words were written"
            assert gc is None or gc[f] == 0, f"{what}: rejected frame {f}'s count {gc[f]}"
            assert gb is None or (gb[f] == [rw, rh, -1, -1]).all(), f"{what}: rejected frame {f}'s box {gb[f]}"
            continue
        if gw is not None and not np.array_equal(gw[f], words[f]):
            r, w = np.argwhere(gw[f] != words[f])[0]
            raise AssertionError(f"{what}: frame {f} row {r} word {w}: {int(gw[f][r, w]):#018x} != "
                                 f"{int(words[f][r, w]):#018x} ({int((gw[f] != words[f]).sum())} of {gw[f].size} words)")
        assert gc is None or gc[f] == counts[f], f"{what}: frame {f} count {gc[f]} != {counts[f]}"
        assert gb is None or (gb[f] == boxes[f]).all(), f"{what}: frame {f} box {gb[f]} != {boxes[f]}"


def mask_windows(W, H):
    """The full frame, then windows whose x runs through every residue mod 8 and several mod 64, with rw 1, 63, 64, 65
    and 129 in turn (cut to the frame)."""
    out = [(0, 0, W, H)]
    for k, x in enumerate(list(range(8)) + [31, 63, 64, 65, 70, 127, 1000, W]):
        rw = min((1, 63, 64, 65, 129)[k % 5], W)
        x = min(x, W - rw)
        y = min(k % 9, H - 1)
        rh = max(1, min(H - y, 1 + (k * 5) % 19))
        if (x, y, rw, rh) not in out:
            out.append((x, y, rw, rh))
    return out


def maps_for(images, seed, top=255):
    """A band around frame 0 whose width changes from pixel to pixel: never constant, and both verdicts occur."""
    rng = np.random.default_rng(seed)
    base = images[0].astype(np.int64)
    shape = base.shape
    lo = np.clip(base - rng.integers(0, 1 + top // 8, shape), 0, top).astype(images.dtype)
    hi = np.clip(base + rng.integers(0, 1 + top // 8, shape), 0, top).astype(images.dtype)
    if lo.size > 1:
        lo.flat[0], lo.flat[-1] = 0, top // 2
        hi.flat[0], hi.flat[-1] = top, top // 2 + 1
    return lo, hi


@pytest.mark.parametrize("mode", ("mixed", "noise8"))
@pytest.mark.parametrize("W,H,n", SHAPES)
def test_windows_scalars_and_maps_in_both_modes(dv, codec, mode, W, H, n):
    import torch
    bt = Batch(codec, mode, W, H, n)
    images = bt.images.cpu().numpy()
    lo_map, hi_map = maps_for(images, W + H)
    d_lo, d_hi = dev(lo_map), dev(hi_map)
    for k, win in enumerate(mask_windows(W, H)):
        outside = bool(k & 1)
        what = f"{mode} {W}x{H} window {win}"
        got, res = run(dv, codec, bt, W, H, n, win, 96, 160, outside, what=what + " scalars")
        compare(got, images, win, 96, 160, outside, what=what + " scalars")
        assert torch.equal(res, bt.results)
        got, res = run(dv, codec, bt, W, H, n, win, d_lo, d_hi, not outside, what=what + " maps")
        compare(got, images, win, lo_map, hi_map, not outside, what=what + " maps")
        assert torch.equal(res, bt.results)


def test_one_map_and_one_scalar(dv, codec):
    W, H, n = 200, 123, 5
    bt = Batch(codec, "mixed", W, H, n)
    images = bt.images.cpu().numpy()
    lo_map, hi_map = maps_for(images, 3)
    for win in mask_windows(W, H)[:4] + [(67, 11, 129, 40)]:
        for lo, hi in ((lo_map, 200), (40, hi_map), (lo_map, None), (None, hi_map)):
            for outside in (False, True):
                what = f"{win} lo {type(lo).__name__} hi {type(hi).__name__} outside {outside}"
                got, _ = run(dv, codec, bt, W, H, n, win, lo, hi, outside, what=what)
                compare(got, images, win, 0 if lo is None else lo, 255 if hi is None else hi, outside, what=what)
    # a map indexed by window coordinates would give another mask: the test can tell
    win = (67, 11, 129, 40)
    right = mr.expected(images, *win, lo_map, hi_map)[0]
    wrong = mr.pack(np.stack([(im[11:51, 67:196] >= lo_map[:40, :129]) & (im[11:51, 67:196] <= hi_map[:40, :129])
                              for im in images]))
    assert not np.array_equal(right, wrong)


@pytest.mark.parametrize("mode", ("mixed", "noise8"))
def test_wide_frame_pieces_and_seams(dv, codec, mode):
    """4200 x 24, window (3, 1, 4190, 20): 66 words in 3 pieces of 22, whose seams fall inside tiles (x0 = 3)."""
    W, H, n = 4200, 24, 3
    assert dv.mask_plan(W, H, n, 3, 1, 4190, 20)["pieces_x"] == 3
    bt = Batch(codec, mode, W, H, n)
    images = bt.images.cpu().numpy()
    lo_map, hi_map = maps_for(images, 42)
    for win in ((3, 1, 4190, 20), (0, 0, W, H), (8, 0, 4096, 24), (5, 3, 2049, 9)):
        for outside in (False, True):
            got, _ = run(dv, codec, bt, W, H, n, win, 100, 150, outside, what=f"{mode} {win}")
            compare(got, images, win, 100, 150, outside, what=f"{mode} {win} scalars")
            got, _ = run(dv, codec, bt, W, H, n, win, lo_map, hi_map, outside, what=f"{mode} {win}")
            compare(got, images, win, lo_map, hi_map, outside, what=f"{mode} {win} maps")
    org = np.array([[3, 1], [-7, 9], [6, 2]], np.int32)
    got, _ = run(dv, codec, bt, W, H, n, (0, 0, 4190, 20), lo_map, 180, False, origins=org)
    compare(got, images, (0, 0, 4190, 20), lo_map, 180, False, origins=org, what="4200x24 origins")


@pytest.mark.parametrize("W,H,n,rw,rh", [(200, 123, 9, 61, 37), (200, 123, 9, 129, 20), (64, 48, 8, 64, 48),
                                         (1921, 1081, 8, 700, 9)])
def test_per_frame_origins(dv, codec, W, H, n, rw, rh):
    """x mod 8 differs from frame to frame; some origins are clamped from outside the frame; the maps stay in frame
    coordinates."""
    import torch
    rng = np.random.default_rng(W + rw)
    bt = Batch(codec, "mixed", W, H, n)
    images = bt.images.cpu().numpy()
    lo_map, hi_map = maps_for(images, 23)
    org = np.stack([rng.integers(-9, W + 9, n), rng.integers(-9, H + 9, n)], 1).astype(np.int32)
    org[:8, 0] = np.minimum(np.arange(8) + 8 * rng.integers(0, 4, 8), W - rw)   # every residue the window allows
    org[0] = (-5, H + 100)
    org[1] = (W + 50, -3)
    org[2] = (W - rw, H - rh)
    for lo, hi, outside in ((lo_map, hi_map, False), (90, 170, True), (lo_map, 255, True)):
        what = f"{W}x{H} origins window {rw}x{rh}"
        got, res = run(dv, codec, bt, W, H, n, (0, 0, rw, rh), lo, hi, outside, origins=org, what=what)
        compare(got, images, (0, 0, rw, rh), lo, hi, outside, origins=org, what=what)
        assert torch.equal(res, bt.results)


class Stream:
    """Crafted frames in one device buffer."""

    def __init__(self, frames, W, H, bits=8):
        import torch
        self.images = np.stack([cr.decode_frame(fr, W, H, bits)[2] for fr in frames])
        buf, self.lead, offs, self.total = cr.layout(frames, "concat", lead=32)
        self.buf, self.offs = torch.from_numpy(buf).cuda(), torch.from_numpy(offs).cuda()
        T = cr.tiles(W, H)
        self.depths = np.stack([fr[24:24 + T].astype(np.int64) for fr in frames])
        mb = 1 if bits == 8 else 2
        mins = [fr[28 + T:28 + T + mb * T] for fr in frames]
        self.minima = np.stack([(m if mb == 1 else m.view("<u2")).astype(np.int64) for m in mins])


def edge_thresholds(s, rng, top, samples=6):
    """0, the pixel maximum and, for sampled tiles (depth d, minimum m) -- wrapping ones and others -- m - 1, m,
    m + 2^d - 1 and m + 2^d: the exact edges of the decided-tile rule."""
    out = {0, top}
    d, m = s.depths.ravel(), s.minima.ravel()
    wraps = m + (1 << d) - 1 > top
    for sel in (np.nonzero(wraps & (d > 0))[0], np.nonzero(~wraps & (d > 0))[0]):
        for i in rng.choice(sel, min(samples // 2, len(sel)), replace=False):
            out.update((m[i] - 1, m[i], m[i] + (1 << d[i]) - 1, m[i] + (1 << d[i])))
    return sorted(int(t) for t in out if 0 <= t <= top)


def test_decided_tile_edges_on_every_depth_and_minimum(dv, codec):
    """crafted.all_pairs_frame (every depth x minimum, wrapping ones included) and boundary minima with all-ones and
    all-zeros payloads: scalar thresholds at the exact edges of the tiles' ranges, as lo and as hi, in both modes."""
    rng = np.random.default_rng(2025)
    W = H = 384
    frames = [cr.all_pairs_frame(rng, "ones", perm="random"), cr.all_pairs_frame(rng, "zeros", perm="random"),
              cr.all_pairs_frame(rng, "random", perm="random"),
              cr.craft(rng, W, H, 8, "random", "boundary", "ones", header=(2, 3, 0)),
              cr.craft(rng, W, H, 8, "random", "boundary", "zeros", header=(2, 4, 0))]
    s = Stream(frames, W, H)
    n = len(frames)
    assert (s.minima + (1 << s.depths) - 1 > 255).any()
    win = (0, 0, W, H)
    for t in edge_thresholds(s, rng, 255):
        for lo, hi in ((t, 255), (0, t)):
            for outside in (False, True):
                what = f"all pairs lo {lo} hi {hi} outside {outside}"
                got, _ = run(dv, codec, s, W, H, n, win, lo, hi, outside, what=what)
                compare(got, s.images, win, lo, hi, outside, what=what)
    for lo, hi, win in ((200, 100, (0, 0, W, H)), (1, 0, (5, 3, 300, 100)), (255, 0, (9, 9, 65, 9)), (16, 31, (3, 0, 381, 384))):
        for outside in (False, True):
            got, _ = run(dv, codec, s, W, H, n, win, lo, hi, outside)
            compare(got, s.images, win, lo, hi, outside, what=f"lo {lo} hi {hi} outside {outside} {win}")
            if lo > hi:   # the empty band
                want = 0 if not outside else win[2] * win[3]
                assert (got[1] == want).all()


def test_band_from_background_is_the_absolute_difference(dv, codec):
    import torch
    W, H, n = 200, 123, 6
    bt = Batch(codec, "mixed", W, H, n)
    bg = bt.images[0].clone()
    bg[:7, :] = 0
    bg[-7:, :] = 255       # clamping at both ends
    for below, above in ((3, None), (0, None), (10, 2), (300, 300)):
        lo, hi = dv.band_from_background(bg, below, above)
        assert lo.dtype == torch.uint8 and hi.dtype == torch.uint8
        m, _ = codec.decode_mask(bt.buf, bt.lead, bt.total, bt.offs, W, H, n, lo=lo, hi=hi, outside=True, boxes=True)
        codec.sync()
        diff = bt.images.int() - bg.int()
        want = (diff < -below) | (diff > (below if above is None else above))
        if above is None:
            assert torch.equal(want, diff.abs() > below)
        assert torch.equal(m.unpack(), want)
        assert torch.equal(m.counts.long(), want.sum((1, 2)))


@pytest.mark.parametrize("W,H,n,how", [(64, 48, 40, "concat"), (200, 123, 23, "residues"), (1921, 17, 9, "slots"),
                                       (8, 8, 70, "offsets"), (4200, 9, 7, "concat")])
def test_crafted_and_rejected_frames(dv, codec, W, H, n, how):
    """Every depth, wrapping minima, random payload, frames with one rule broken among good ones: a rejected frame's
    words keep the sentinel, its count is 0, its box empty; results are decode_frames'."""
    import torch
    rng = np.random.default_rng(W * 7919 + H)
    s = Crafted(rng, W, H, n, how)
    keep = [im is not None for im in s.images]
    assert any(keep) and not all(keep)
    canvas = torch.full((n, H, W), 0x33, dtype=torch.uint8, device="cuda")
    images, want_res = codec.decode_frames(s.buf, s.lead, s.total, s.offs, W, H, n, images=canvas)
    codec.sync()
    images = images.cpu().numpy()
    assert all((images[f] == s.images[f]).all() for f in range(n) if keep[f])
    lo_map, hi_map = maps_for(np.stack([im for im in s.images if im is not None]), H)
    for k, win in enumerate(mask_windows(W, H)[:7]):
        what = f"crafted {how} {W}x{H} {win}"
        lo, hi = ((lo_map, hi_map), (64, 200), (lo_map, 255))[k % 3]
        got, res = run(dv, codec, s, W, H, n, win, lo, hi, bool(k & 1), what=what)
        compare(got, images, win, lo, hi, bool(k & 1), keep=keep, what=what)
        assert torch.equal(res, want_res)


def test_output_subsets(dv, codec):
    """d_mask NULL with counts only, boxes only, words only: what is not asked for is not written."""
    W, H, n = 200, 123, 7
    bt = Batch(codec, "mixed", W, H, n)
    images = bt.images.cpu().numpy()
    win = (5, 3, 131, 77)
    for bits, counts, boxes in ((False, True, False), (False, False, True), (True, False, False), (False, True, True),
                                (True, True, False)):
        got, _ = run(dv, codec, bt, W, H, n, win, 80, 200, False, bits=bits, counts=counts, boxes=boxes)
        assert [g is not None for g in got] == [bits, counts, boxes]
        compare(got, images, win, 80, 200, False, what=f"subset {bits} {counts} {boxes}")
    # the Python defaults: words and counts, no boxes; counts equal the unpacked mask's sums
    m, _ = codec.decode_mask(bt.buf, bt.lead, bt.total, bt.offs, W, H, n, *win, lo=80, hi=200)
    codec.sync()
    assert m.boxes is None and tuple(m.bits.shape) == (n, 77, 3) and m.rw == 131
    up = m.unpack()
    assert tuple(up.shape) == (n, 77, 131) and (up.sum((1, 2)) == m.counts).all()
    assert np.array_equal(up.cpu().numpy(), mr.verdicts(images, *win, 80, 200))


def test_full_size_frames_on_the_device(dv, codec):
    """4096 x 3072, 2 frames: the aligned full frame (2 pieces of 32 words), an unaligned window (3 pieces) and maps,
    compared on the device with torch."""
    import torch
    W, H, n = 4096, 3072, 2
    bt = Batch(codec, "mixed", W, H, n)

    def boxes_of(b):
        out = []
        for f in range(b.shape[0]):
            xs, ys = b[f].any(0).nonzero().flatten(), b[f].any(1).nonzero().flatten()
            out.append([b.shape[2], b.shape[1], -1, -1] if xs.numel() == 0 else
                       [int(xs[0]), int(ys[0]), int(xs[-1]), int(ys[-1])])
        return torch.tensor(out, dtype=torch.int32, device=b.device)

    bg = bt.images[0]
    lo_map, hi_map = dv.band_from_background(bg, 5, 9)
    for (x, y, rw, rh), lo, hi, outside in (((0, 0, W, H), 100, 180, False), ((5, 3, 4090, 3000), 100, 180, True),
                                            ((0, 0, W, H), lo_map, hi_map, True), ((1027, 9, 2000, 2001), lo_map, 200, False)):
        m, res = codec.decode_mask(bt.buf, bt.lead, bt.total, bt.offs, W, H, n, x, y, rw, rh, lo=lo, hi=hi,
                                   outside=outside, boxes=True)
        codec.sync()
        p = bt.images[:, y:y + rh, x:x + rw].int()
        L = lo[y:y + rh, x:x + rw].int() if isinstance(lo, torch.Tensor) else lo
        Hh = hi[y:y + rh, x:x + rw].int() if isinstance(hi, torch.Tensor) else hi
        want = (p >= L) & (p <= Hh)
        want = ~want if outside else want
        assert torch.equal(m.unpack(), want), (x, y, rw, rh)
        assert torch.equal(m.counts.long(), want.sum((1, 2))) and torch.equal(m.boxes, boxes_of(want))
        assert torch.equal(res, bt.results)
        if rw % 64:   # the bits at and beyond rw are 0
            assert int((m.bits[:, :, -1] >> (rw % 64)).abs().sum()) == 0


def test_zero_frames_defaults_and_timing_slots(dv, codec):
    import torch
    W, H, n = 200, 123, 4
    bt = Batch(codec, "mixed", W, H, n)
    o = Out(dv, n, 191, 113)
    codec.decode_mask(bt.buf, bt.lead, bt.total, bt.offs, W, H, 0, 8, 8, 191, 113, lo=3, mask=o.mask)
    codec.sync()
    for g, sent in zip(o.read(), (SENT64, SENT32, SENT32)):
        assert (g.view(np.uint64 if sent == SENT64 else np.uint32) == sent).all(), "n == 0 wrote an output"
    m, res = codec.decode_mask(bt.buf, bt.lead, bt.total, bt.offs, W, H, 0)
    assert tuple(m.bits.shape) == (0, H, 4) and tuple(m.counts.shape) == (0,) and tuple(res.shape) == (0, 4)
    with pytest.raises(dv.DbdeError):   # a bad window is the same error with no frames as with some
        codec.decode_mask(bt.buf, bt.lead, bt.total, bt.offs, W, H, 0, 8, 8, 193, 113)
    with pytest.raises(dv.DbdeError):
        codec.decode_mask(bt.buf, bt.lead, bt.total, bt.offs, W, H, n, 8, 8, 193, 113)
    # defaults: the whole frame, the band [0, 255]: every bit set
    m, res = codec.decode_mask(bt.buf, bt.lead, bt.total, bt.offs, W, H, n, boxes=True)
    codec.sync()
    assert (m.counts == W * H).all() and m.unpack().all() and torch.equal(res, bt.results)
    assert (m.boxes.cpu() == torch.tensor([0, 0, W - 1, H - 1], dtype=torch.int32)).all()
    e = dv.Mask.empty(3, 10, 65, "cuda", boxes=True)
    assert tuple(e.bits.shape) == (3, 10, 2) and e.bits.dtype == torch.int64 and e.counts.dtype == torch.int32
    assert tuple(e.boxes.shape) == (3, 4) and e.rw == 65 and not e.unpack().any()
    codec.timing(True)
    codec.timing_read(reset=True)
    codec.decode_mask(bt.buf, bt.lead, bt.total, bt.offs, W, H, n, lo=100)
    t = codec.timing_read(reset=True)
    codec.timing(False)
    assert [t[k][1] for k in ("encode", "decode_index", "decode", "scan")] == [0, 1, 1, 0]


def test_argument_errors_leave_the_codec_usable(dv, codec):
    import torch
    W, H, n = 64, 48, 2
    bt = Batch(codec, "mixed", W, H, n)
    args = (bt.buf, bt.lead, bt.total, bt.offs, W, H, n)
    good = torch.zeros((H, W), dtype=torch.uint8, device="cuda")
    for kw in (dict(lo=256), dict(hi=-1), dict(lo=1.5), dict(lo=torch.zeros((H, W + 1), dtype=torch.uint8, device="cuda")),
               dict(hi=good.to(torch.int16)), dict(hi=torch.zeros((H, W), dtype=torch.uint8)),
               dict(lo=torch.zeros((H, 2 * W), dtype=torch.uint8, device="cuda")[:, ::2]),
               dict(mask=dv.Mask(torch.zeros((n, H, 1), dtype=torch.int32, device="cuda"))),
               dict(mask=dv.Mask(torch.zeros((n, H - 1, 1), dtype=torch.int64, device="cuda"))),
               dict(mask=dv.Mask(None, torch.zeros(n, dtype=torch.int64, device="cuda"))), dict(mask=dv.Mask())):
        with pytest.raises(dv.DbdeError):
            codec.decode_mask(*args, **kw)
    for kw in (dict(x=1, rw=64), dict(rw=65), dict(rh=0), dict(x=60, rw=8)):
        with pytest.raises(dv.DbdeError):
            codec.decode_mask(*args, **kw)
    raw = torch.zeros(8 * n * H + 64, dtype=torch.uint8, device="cuda")
    L, ptr, base = codec.L, bt.buf.data_ptr() + bt.lead, raw.data_ptr()

    def c_call(mode=0, lo_map=None, lo0=0, hi_map=None, hi0=255, mask=base, counts=None, boxes=None, fn="dbde_hip_decode_mask"):
        return getattr(L, fn)(codec.h, ptr, bt.total, bt.offs.data_ptr(), W, H, n, 0, 0, W, H, None, mode, lo_map, lo0,
                              hi_map, hi0, mask, counts, boxes, None)
    for bad in (2, -1, 99):
        assert c_call(mode=bad) == dv.ERR_ARG                          # unknown mode
    assert c_call(lo0=256) == dv.ERR_ARG and c_call(hi0=256) == dv.ERR_ARG and c_call(hi0=0xFFFFFFFF) == dv.ERR_ARG
    assert c_call(mask=None) == dv.ERR_ARG                             # no output requested
    assert c_call(mask=base + 4) == dv.ERR_ARG and c_call(mask=base + 1) == dv.ERR_ARG   # misaligned mask
    assert c_call(counts=base + 2) == dv.ERR_ARG and c_call(mask=None, boxes=base + 1) == dv.ERR_ARG
    assert c_call(fn="dbde16_hip_decode_mask", lo_map=good.data_ptr() + 1) == dv.ERR_ARG   # misaligned 16-bit map
    assert c_call(fn="dbde16_hip_decode_mask", hi0=65536) == dv.ERR_ARG
    with pytest.raises(dv.DbdeError):
        codec._check(c_call(mode=7), "dbde_hip_decode_mask")
    codec.sync()
    assert (raw == 0).all()
    # the next valid calls on the same codec succeed: a U8 map at an odd address is fine, counts at 4 mod 8 too
    odd = torch.zeros(H * W + 1, dtype=torch.uint8, device="cuda")
    assert c_call(lo_map=odd.data_ptr() + 1, hi0=200, counts=base + 8 * n * H + 4) == dv.OK
    codec.sync()
    want = (bt.images <= 200)
    got = raw[:8 * n * H].view(torch.int64).view(n, H, 1)
    assert torch.equal(dv.Mask(got, rw=W).unpack(), want)
    assert torch.equal(raw[8 * n * H + 4: 8 * n * H + 4 + 4 * n].view(torch.int32).long(), want.sum((1, 2)))
