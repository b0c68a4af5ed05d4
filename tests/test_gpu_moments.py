"""GPU: patch moments -- dbde_hip_patch_moments (Codec.patch_moments): eight thresholded sums and a box per patch.

Every comparison is exact integer equality with tests/moments_ref.py over the oracle's decode of the whole frame (for
crafted frames: crafted.decode_frame's).  The moments, boxes and used origins are written into 0xEE canvases with guard
bands in front of and behind them, so "untouched" and "nothing outside" are checked; rejections are compared with what
dbde_hip_decode_frames reports for the same batch.
"""
import numpy as np
import pytest

import moments_ref as mr
import patch_ref as pr
from test_gpu_patches import GEOMETRIES, origins_for, sizes_for
from test_gpu_project import Crafted
from test_gpu_roi import MODES, Batch

pytestmark = pytest.mark.gpu

GUARD = 64


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


def run_moments(codec, buf, lead, total, offs, W, H, n, pw, ph, origins, lo, hi, weight, counts=None, mode=pr.CLAMP, bits=8):
    """Runs into 0xEE canvases with guard bands; checks the guards -> (moments (n, K, 8) int64, boxes (n, K, 4), used
    (n, K, 2), results tensor)."""
    import torch
    origins = np.asarray(origins, np.int64).reshape(n, -1, 2)
    K = origins.shape[1]
    d_org = torch.from_numpy(origins.astype(np.int32)).cuda()
    d_cnt = None if counts is None else torch.from_numpy(np.asarray(counts, np.int64).astype(np.uint32).view(np.int32)).cuda()
    spec = ((8, torch.int64, mr.UNTOUCHED, "moments"), (4, torch.int32, pr.UNTOUCHED_ORIGIN, "boxes"),
            (2, torch.int32, pr.UNTOUCHED_ORIGIN, "used origins"))
    canvases = [torch.full((per * n * K + 2 * GUARD,), fillv, dtype=dt, device="cuda") for per, dt, fillv, _ in spec]
    views = [c[GUARD: c.numel() - GUARD] for c in canvases]
    fn = codec.patch_moments if bits == 8 else codec.patch_moments16
    _, res = fn(buf, lead, total, offs, W, H, n, pw, ph, d_org, lo, hi, weight=mr.WEIGHTS[weight], counts=d_cnt,
                edge="clamp" if mode == pr.CLAMP else "fill", out=views[0], bbox=views[1], used=views[2])
    codec.sync()
    got = []
    for c, (per, _, fillv, what) in zip(canvases, spec):
        h = c.cpu().numpy()
        assert (h[:GUARD] == fillv).all(), f"wrote in front of the {what}"
        assert (h[-GUARD:] == fillv).all(), f"wrote behind the {what}"
        got.append(h[GUARD:-GUARD].reshape(n, K, per))
    return got[0], got[1], got[2], res


def check_moments(codec, src, frames, W, H, pw, ph, origins, lo, hi, weight, counts=None, mode=pr.CLAMP, bits=8,
                  stream=None, what=""):
    """src: anything with buf, lead, total, offs.  frames: the expected images, None for rejected frames."""
    n = len(frames)
    buf, lead, total, offs = stream if stream is not None else (src.buf, src.lead, src.total, src.offs)
    mom, box, used, res = run_moments(codec, buf, lead, total, offs, W, H, n, pw, ph, origins, lo, hi, weight, counts, mode, bits)
    want, want_box, want_used, _ = mr.expected(frames, W, H, pw, ph, origins, counts, mode, lo, hi, weight)
    want = np.array(want.tolist(), dtype=np.int64)
    where = f"{what} {W}x{H} patch {pw}x{ph} mode {mode} band [{lo}, {hi}] weight {mr.WEIGHTS[weight]}"
    if not np.array_equal(mom, want):
        f, k, s = np.argwhere(mom != want)[0]
        o = np.asarray(origins).reshape(n, -1, 2)[f, k]
        raise AssertionError(f"{where}: frame {f} patch {k} origin {tuple(o)}: {int((mom != want).any(axis=2).sum())} "
                             f"patches differ, first in {mr.SLOTS[s]}: got {mom[f, k].tolist()} want {want[f, k].tolist()}")
    if not np.array_equal(box, want_box):
        f, k, _ = np.argwhere(box != want_box)[0]
        raise AssertionError(f"{where}: frame {f} patch {k}: box {box[f, k].tolist()} want {want_box[f, k].tolist()}")
    assert np.array_equal(used, want_used), f"{where}: used origins"
    return res


def tile_ranges(img):
    """(minimum, maximum) of every whole or cut 8 x 8 tile of the image."""
    H, W = img.shape
    return [(int(img[y:y + 8, x:x + 8].min()), int(img[y:y + 8, x:x + 8].max())) for y in range(0, H, 8) for x in range(0, W, 8)]


def bands_for(rng, frames, top, tiles=6):
    """The fixed bands, and for a few tiles of the frames their own minimum and maximum and the neighbours +-1, as lo
    and as hi: the off-by-one sites of the header shortcut."""
    bands = [(0, top), (top // 2, top // 2 - 1), (top, 0)]
    ranges = [r for im in frames if im is not None for r in tile_ranges(im)]
    mid = ranges[len(ranges) // 2][0]
    bands += [(mid, mid)]
    for t in rng.choice(len(ranges), size=min(tiles, len(ranges)), replace=False):
        mn, mx = ranges[t]
        for v in (mn - 1, mn, mn + 1, mx - 1, mx, mx + 1):
            v = min(max(v, 0), top)
            bands += [(v, top), (0, v)]
        bands += [(mn, mx), (min(mn + 1, top), max(mx - 1, 0))]
    return bands


@pytest.mark.parametrize("W,H,n", GEOMETRIES)
def test_moments_match_moments_ref(codec, oracle, W, H, n):
    rng = np.random.default_rng(W * 7919 + H + 1)
    batches = [Batch(codec, oracle, mode, W, H, n, first=3 + i, misalign=(0, 1, 3, 6)[i]) for i, mode in enumerate(MODES)]
    bands = [bands_for(rng, b.full, 255) for b in batches]
    for j, (pw, ph) in enumerate(sizes_for(W, H) + [(3, 512)]):
        b, bd = batches[j % len(batches)], bands[j % len(batches)]   # the sizes are dealt round-robin over the content modes
        org = origins_for(rng, W, H, pw, ph, n)
        K = org.shape[1]
        counts = [None, [K] * n, [0] * n, [K + 5, 1, K // 2, 0][:n], None][j % 5]
        lo, hi = bd[(3 * j) % len(bd)]
        res = check_moments(codec, b, b.full, W, H, pw, ph, org, lo, hi, j % 4, counts, pr.FILL, what=f"fill {MODES[j % 4]}")
        assert all(r == (2, b.first + f, 0, len(b.packed[f])) for f, r in enumerate(codec.parse_results(res)))
        if pw <= W and ph <= H:
            lo, hi = bd[(3 * j + 1) % len(bd)]
            check_moments(codec, b, b.full, W, H, pw, ph, org, lo, hi, (j + 1) % 4, counts, pr.CLAMP, what=f"clamp {MODES[j % 4]}")


@pytest.mark.parametrize("mode", MODES)
def test_threshold_sites_of_the_header_shortcut(codec, oracle, mode):
    """Every band of bands_for (the tiles' own minima and maxima and their neighbours), all four weights."""
    W, H, n = 72, 41, 2
    rng = np.random.default_rng(len(mode))
    b = Batch(codec, oracle, mode, W, H, n, first=1, misalign=5)
    org = np.array([[(x, y) for x in (-3, 0, 21, 45) for y in (-2, 7, 15)]] * n)
    for i, (lo, hi) in enumerate(bands_for(rng, b.full, 255, tiles=8)):
        check_moments(codec, b, b.full, W, H, 32, 30, org, lo, hi, i % 4, None, pr.FILL, what=f"sites {mode}")


def known_tiles(fr, W, H, pix, rng, every_depth=True):
    """(m, d) of some tiles of a crafted frame: the first of every depth it has (every_depth), up to three that wrap,
    two more."""
    fr = np.frombuffer(bytes(fr), np.uint8)
    T = ((W + 7) // 8) * ((H + 7) // 8)
    depths = fr[24:24 + T].astype(np.int64)
    mraw = fr[28 + T: 28 + T + pix * T].astype(np.int64)
    minima = mraw if pix == 1 else mraw[0::2] | (mraw[1::2] << 8)
    top = 255 if pix == 1 else 65535
    picked = {int(np.flatnonzero(depths == d)[0]) for d in np.unique(depths)} if every_depth else set()
    wraps = np.flatnonzero(minima + (1 << depths) - 1 > top)
    picked.update(int(t) for t in wraps[:3])
    picked.update(int(t) for t in rng.integers(0, T, 2))
    return [(int(minima[t]), int(depths[t])) for t in sorted(picked)]


def crafted_bands(s, W, H, pix, rng):
    """For tiles of known (m, d) of good frames (the first, of random depths: every depth; the second: its wrapping
    tiles): m - 1, m, m + 2^d - 1 and m + 2^d as lo and as hi."""
    top = 255 if pix == 1 else 65535
    bands = []
    good = [f for f in range(s.n) if s.images[f] is not None]
    for i, f in enumerate(good[:2]):
        for m, d in known_tiles(s.frames[f], W, H, pix, rng, every_depth=i == 0):
            for v in (m - 1, m, m + (1 << d) - 1, m + (1 << d)):
                v %= top + 1   # (a wrapping tile's top lies below its minimum)
                bands += [(v, top), (0, v)]
    return bands


@pytest.mark.parametrize("W,H,n,how", [(64, 48, 13, "concat"), (200, 123, 8, "residues"), (1921, 17, 7, "slots")])
def test_crafted_and_rejected_frames(codec, W, H, n, how):
    """Every depth 0..8 at every payload byte alignment, wrapping minima, frames with one rule broken between good
    ones: a rejected frame's entries keep the canvas, results are decode_frames', neighbours exact."""
    import torch
    rng = np.random.default_rng(W * 7919 + H)
    s = Crafted(rng, W, H, n, how)
    assert any(im is None for im in s.images) and any(im is not None for im in s.images)
    _, want_res = codec.decode_frames(s.buf, s.lead, s.total, s.offs, W, H, n)
    pw, ph = 32, min(H, 32)
    org = np.array([[(x, y) for x in (-5, 19, W - 9) for y in (-3, 0, H - 6)]] * n)
    for i, (lo, hi) in enumerate(crafted_bands(s, W, H, 1, rng)):
        res = check_moments(codec, s, s.images, W, H, pw, ph, org, lo, hi, i % 4, None, pr.FILL if i % 3 else pr.CLAMP,
                            what=f"crafted {how}")
        assert torch.equal(res, want_res)
    for j, (pw, ph) in enumerate(((9, 9), (min(W, 505), 3), (58, min(H, 58)))):
        org = origins_for(rng, W, H, pw, ph, n)
        for m in (pr.CLAMP, pr.FILL):
            check_moments(codec, s, s.images, W, H, pw, ph, org, (0, 100, 37)[j], (255, 200, 37)[j], (j + m) % 4, None, m,
                          what=f"crafted {how}")


@pytest.mark.parametrize("W,H,n,mode", [(64, 64, 3, "noise8"), (1921, 17, 2, "mixed"), (10, 10, 4, "smooth")])
def test_moments_read_nothing_past_stream_bytes(codec, oracle, W, H, n, mode):
    """stream_bytes ends exactly at the last frame's end, at every residue mod 16, with junk behind it; one byte short
    rejects the last frame only, whose entries stay untouched."""
    import torch
    b = Batch(codec, oracle, mode, W, H, n, first=3)
    pw, ph = min(W, 33), min(H, 9)
    org = np.array([[(W - pw, H - ph), (W - 3, H - 2), (0, 0), (W - pw - 1, H - ph)]] * n)
    for pad in range(16):
        junk = (0xA5, 0x00, 0xFF)[pad % 3]
        t = torch.full((pad + b.total + 48,), junk, dtype=torch.uint8, device="cuda")
        t[pad:pad + b.total] = b.buf[b.lead:b.lead + b.total]
        for m in (pr.CLAMP, pr.FILL):
            check_moments(codec, b, b.full, W, H, pw, ph, org, 0, 255, pad % 4, None, m, stream=(t, pad, b.total, b.offs))
            res = check_moments(codec, b, b.full[:-1] + [None], W, H, pw, ph, org, 1, 254, (pad + 1) % 4, None, m,
                                stream=(t, pad, b.total - 1, b.offs))
            assert codec.parse_results(res)[-1][0] == 0xFFFFFFFF


def test_count_equals_decode_mask_and_clamp_equals_decode_roi(codec, oracle):
    import torch
    W, H, n = 200, 123, 3
    b = Batch(codec, oracle, "mixed", W, H, n, first=2)
    whole = np.zeros((n, 1, 2), np.int64)
    for lo, hi in ((0, 255), (40, 180), (200, 100), (int(b.full[0][5, 5]), int(b.full[0][5, 5]))):
        mom, box, _, _ = run_moments(codec, b.buf, b.lead, b.total, b.offs, W, H, n, W, H, whole, lo, hi, mr.COUNT)
        mask, _ = codec.decode_mask(b.buf, b.lead, b.total, b.offs, W, H, n, lo=lo, hi=hi, counts=True, boxes=True)
        codec.sync()
        assert np.array_equal(mom[:, 0, 0], mask.counts.cpu().numpy().view(np.uint32).astype(np.int64)), (lo, hi)
        mb = mask.boxes.cpu().numpy().reshape(n, 4)
        assert np.array_equal(box[:, 0], mb), (lo, hi)
    rng = np.random.default_rng(11)
    for j, (pw, ph) in enumerate(((32, 32), (58, 58), (7, 97))):
        org = origins_for(rng, W, H, pw, ph, n)[:, ::4]
        mom, box, used, _ = run_moments(codec, b.buf, b.lead, b.total, b.offs, W, H, n, pw, ph, org, 30, 220, j + 1)
        for k in range(org.shape[1]):
            d_o = torch.from_numpy(org[:, k].astype(np.int32)).cuda()
            win, _ = codec.decode_roi(b.buf, b.lead, b.total, b.offs, W, H, n, 0, 0, pw, ph, origins=d_o)
            codec.sync()
            for f in range(n):
                m, bx, _ = mr.moments(win[f].cpu().numpy(), pw, ph, pw, ph, 0, 0, pr.CLAMP, 30, 220, j + 1)
                assert mom[f, k].tolist() == m and tuple(box[f, k]) == bx, (pw, ph, f, k)


def test_timing_hook_zero_frames_and_argument_errors(codec, oracle, dv):
    import torch
    W, H, n = 300, 200, 2
    b = Batch(codec, oracle, "mixed", W, H, n)
    org = torch.zeros((n, 3, 2), dtype=torch.int32, device="cuda")
    codec.timing(True)
    codec.timing_read(reset=True)
    codec.patch_moments(b.buf, b.lead, b.total, b.offs, W, H, n, 32, 32, org, 10, 200)
    t = codec.timing_read(reset=True)
    codec.timing(False)
    assert t["decode_index"][1] == 1 and t["decode"][1] == 1 and t["encode"][1] == 0
    out = torch.full((n * 3 * 8 + 1,), mr.UNTOUCHED, dtype=torch.int64, device="cuda")
    box = torch.full((n * 3 * 4,), pr.UNTOUCHED_ORIGIN, dtype=torch.int32, device="cuda")
    usd = torch.full((n * 3 * 2 + 1,), pr.UNTOUCHED_ORIGIN, dtype=torch.int32, device="cuda")

    def call(n_frames=n, pw=8, ph=8, K=3, origins=org, edge=0, lo=0, hi=255, weight=0, moments=out, bbox=box, used=usd):
        ptr = lambda v: v.data_ptr() if torch.is_tensor(v) else v   # noqa: E731
        return codec.L.dbde_hip_patch_moments(codec.h, b.buf.data_ptr() + b.lead, b.total, b.offs.data_ptr(), W, H, n_frames,
                                              pw, ph, K, ptr(origins), None, edge, lo, hi, weight, ptr(moments), ptr(bbox),
                                              ptr(used), None)

    assert call(n_frames=0) == dv.OK
    bad = [dict(pw=506), dict(pw=0), dict(ph=0), dict(pw=301), dict(ph=201), dict(edge=2), dict(ph=513, edge=1), dict(lo=256),
           dict(hi=256), dict(hi=65535), dict(weight=4), dict(weight=-1), dict(K=0), dict(origins=None), dict(moments=None),
           dict(moments=out.data_ptr() + 4), dict(bbox=box.data_ptr() + 2), dict(used=usd.data_ptr() + 2),
           dict(used=usd.data_ptr() + 1), dict(n_frames=-1)]
    for kw in bad:
        assert call(**kw) == dv.ERR_ARG, kw
    codec.sync()
    assert (out == mr.UNTOUCHED).all() and (box == pr.UNTOUCHED_ORIGIN).all() and (usd == pr.UNTOUCHED_ORIGIN).all()
    assert call(used=None) == dv.OK and (usd == pr.UNTOUCHED_ORIGIN).all()   # the used origins are optional
    assert call() == dv.OK and call(lo=200, hi=100) == dv.OK and call(ph=200, pw=300) == dv.OK
    codec.sync()
    for kw in (dict(pw=506), dict(ph=513, edge="fill"), dict(lo=256), dict(weight=7), dict(edge=2)):
        a = dict(pw=8, ph=8, edge="clamp", lo=0, weight="above")
        a.update(kw)
        with pytest.raises(dv.DbdeError, match="patch_moments"):
            codec.patch_moments(b.buf, b.lead, b.total, b.offs, W, H, n, a["pw"], a["ph"], org, a["lo"], 255,
                                weight=a["weight"], edge=a["edge"])
    with pytest.raises(dv.DbdeError, match="patch_moments"):
        codec.patch_moments(b.buf, b.lead, b.total, b.offs, W, H, 0, 8, 513, org[:0], 0, 255)
    # the scalars are refused for any n (also n = 0, where the C call is not made), and nothing wraps modulo 2^32
    for nn in (n, 0):
        for kw in (dict(lo=256), dict(hi=256), dict(lo=-1), dict(lo=2 ** 32), dict(hi=2 ** 32 + 100), dict(weight=4),
                   dict(weight=-1), dict(weight=2 ** 32)):
            a = dict(lo=0, hi=255, weight="above")
            a.update(kw)
            with pytest.raises(dv.DbdeError, match="patch_moments"):
                codec.patch_moments(b.buf, b.lead, b.total, b.offs, W, H, nn, 8, 8, org[:nn], a["lo"], a["hi"], weight=a["weight"])
    with pytest.raises(dv.DbdeError, match="dbde16_hip_patch_moments"):
        codec.patch_moments16(b.buf, b.lead, b.total, b.offs, W, H, 0, 8, 8, org[:0], 0, 65536)
    pm, _ = codec.patch_moments(b.buf, b.lead, b.total, b.offs, W, H, 0, 8, 8, org[:0], 0, 255)
    assert tuple(pm.moments.shape) == (0, 3, 8)
    for wrong in (org.to(torch.int64), org[:, :, :1], org.permute(1, 0, 2), org[:1]):
        with pytest.raises(ValueError, match="origins"):
            codec.patch_moments(b.buf, b.lead, b.total, b.offs, W, H, n, 8, 8, wrong, 0, 255)
    with pytest.raises(ValueError, match="weight"):
        codec.patch_moments(b.buf, b.lead, b.total, b.offs, W, H, n, 8, 8, org, 0, 255, weight="mass")
    # pw > W is legal in fill mode
    check_moments(codec, b, b.full, W, H, 400, 3, np.array([[(-50, 100), (0, 199), (-99, -1)]] * n), 0, 255, mr.VALUE, None, pr.FILL)


def ellipse_image(W, H, cx, cy, a, bb, theta, level=200, dark=10):
    """A uniformly filled ellipse of semi-axes a >= bb, major axis at angle theta, on a dark level."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    u = (xx - cx) * np.cos(theta) + (yy - cy) * np.sin(theta)
    v = -(xx - cx) * np.sin(theta) + (yy - cy) * np.cos(theta)
    img = np.full((H, W), dark, np.uint8)
    img[(u / a) ** 2 + (v / bb) ** 2 <= 1.0] = level
    return img


def test_patch_moments_quantities_against_numpy(codec, dv):
    """centroid, covariance and orientation: against the same quantities from numpy over the patch's pixels to 1e-12
    relative, and against the ellipse's known centre, angle and axes to what an ellipse cut out of pixels allows."""
    import torch
    from test_gpu_project import Batch as ImageBatch
    W, H = 200, 123
    cx, cy, a, bb, theta = 97.0, 61.0, 30.0, 12.0, 0.4
    img = ellipse_image(W, H, cx, cy, a, bb, theta)
    b = ImageBatch(codec, "flat", W, H, 1, images=torch.from_numpy(img[None]).cuda())
    org = torch.tensor([[[50, 20], [45, 17], [150, 100], [-300, 5]]], dtype=torch.int32, device="cuda")
    pm, _ = codec.patch_moments(b.buf, b.lead, b.total, b.offs, W, H, 1, 96, 90, org, 100, 255, weight="count", edge="fill",
                                bbox=True)
    codec.sync()
    ys, xs = np.nonzero(img >= 100)
    want_c = np.array([xs.mean(), ys.mean()])
    cov = np.cov(np.stack([xs, ys]).astype(np.float64), bias=True)
    ev, evec = np.linalg.eigh(cov)
    want_ang = np.arctan2(evec[1, 1], evec[0, 1])   # the major axis' eigenvector, as an angle in (-pi/2, pi/2]
    want_ang += np.pi if want_ang <= -np.pi / 2 else (-np.pi if want_ang > np.pi / 2 else 0.0)
    cen, cv = pm.centroid().cpu().numpy()[0], pm.covariance().cpu().numpy()[0]
    ang, major, minor = (t.cpu().numpy()[0] for t in pm.orientation())
    for k in (0, 1):   # two patches that hold the whole ellipse: the same object in frame coordinates
        assert np.allclose(cen[k], want_c, rtol=1e-12, atol=0)
        assert np.allclose(cv[k], cov, rtol=1e-12, atol=1e-12 * cov.max())
        assert np.isclose(major[k], 2 * np.sqrt(ev[1]), rtol=1e-12) and np.isclose(minor[k], 2 * np.sqrt(ev[0]), rtol=1e-12)
        assert np.isclose(ang[k], want_ang, rtol=1e-12)
        # the known ellipse: centre to 0.05 px, axes to 1 %, angle to 0.01 rad (the pixel grid's own error)
        assert np.allclose(cen[k], (cx, cy), atol=0.05) and abs(ang[k] - theta) < 0.01
        assert abs(major[k] / a - 1) < 0.01 and abs(minor[k] / bb - 1) < 0.01
    assert int(pm.count()[0, 0]) == len(xs) and int(pm.mass()[0, 0]) == len(xs)
    assert pm.bbox.cpu().numpy()[0, 0].tolist() == [xs.min() - 50, ys.min() - 20, xs.max() - 50, ys.max() - 20]
    for k in (2, 3):   # nothing selected / wholly outside the frame
        assert int(pm.count()[0, k]) == 0 and np.isnan(cen[k]).all() and np.isnan(cv[k]).all() and np.isnan(ang[k])
        assert pm.bbox.cpu().numpy()[0, k].tolist() == [96, 90, -1, -1]


def test_follow_equals_its_numpy_restatement(codec, dv):
    """3 blobs move by at most 2 pixels a frame over 12 frames of 200 x 123; one leaves the frame, one frame is rejected
    (a depth byte of 9).  The centres equal the same recurrence in numpy float64 exactly."""
    import torch
    from dbde_video_cpp_amd import tracking
    from test_gpu_project import Batch as ImageBatch
    W, H, n, pw, ph, lo, hi = 200, 123, 12, 24, 20, 60, 255
    rng = np.random.default_rng(2024)
    imgs = rng.integers(5, 30, size=(n, H, W)).astype(np.uint8)
    start = np.array([(40.0, 30.0), (120.0, 80.0), (188.0, 60.0)])
    step = np.array([(1.5, 1.0), (-2.0, 0.5), (2.0, -1.0)])   # the third walks out of the frame
    yy, xx = np.mgrid[0:H, 0:W]
    for f in range(n):
        for (x0, y0), (dx, dy) in zip(start, step):
            x, y = x0 + f * dx, y0 + f * dy
            blob = (xx - x) ** 2 + (yy - y) ** 2 <= 9.5
            imgs[f][blob] = 100 + ((xx + 2 * yy)[blob] % 50)
    b = ImageBatch(codec, "flat", W, H, n, images=torch.from_numpy(imgs).cuda())
    bad = 5
    b.buf[b.lead + int(b.offs[bad]) + 24] = 9   # frame 5's first depth byte: rejected
    _, res = codec.decode_frames(b.buf, b.lead, b.total, b.offs, W, H, n)
    rejected = [r[0] == 0xFFFFFFFF for r in codec.parse_results(res)]
    assert rejected == [f == bad for f in range(n)]
    # No host synchronisation: with the centres already on the device, the whole call runs with torch's synchronisation
    # debug mode set to raise (a tensor built from host data, an .item() or a blocking copy would).
    d_start = torch.from_numpy(start).cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        centres, pm = tracking.follow(codec, b.buf, b.lead, b.total, b.offs, W, H, n, d_start, pw, ph, lo, hi)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    again, _ = tracking.follow(codec, b.buf, b.lead, b.total, b.offs, W, H, n, start, pw, ph, lo, hi)   # host centres
    assert torch.equal(again, centres)
    codec.sync()
    c = start.copy()
    want = np.empty((n, 3, 2))
    for f in range(n):
        org = dv.origins_from_centres(c[None], pw, ph)[0]
        assert np.array_equal(pm.used.cpu().numpy()[f], org)
        for k in range(3):
            m = [0] * 8 if f == bad else mr.moments(imgs[f], W, H, pw, ph, org[k, 0], org[k, 1], pr.FILL, lo, hi, mr.ABOVE)[0]
            assert pm.moments.cpu().numpy()[f, k].tolist() == m, (f, k)
            if m[1]:
                c[k] = (np.float64(org[k, 0]) + np.float64(m[2]) / np.float64(m[1]),
                        np.float64(org[k, 1]) + np.float64(m[3]) / np.float64(m[1]))
        want[f] = c
    got = centres.cpu().numpy()
    assert got.dtype == np.float64 and np.array_equal(got, want)
    assert np.abs(got[4, :2] - (start + 4 * step)[:2]).max() < 1.0 and np.array_equal(got[bad], got[bad - 1])
    assert int(pm.count()[-1, 2]) == 0 and np.array_equal(got[-1, 2], got[-2, 2])   # gone: it keeps its last centre
