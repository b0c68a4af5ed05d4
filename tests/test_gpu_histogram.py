"""GPU: per-frame histograms -- dbde_hip_histogram (Codec.histogram).

Expected values are exact integer counts: torch.bincount of dbde_hip_decode_frames' images cut to the window, with
v >> shift clamped into the last bin.  Crafted frames (tests/crafted.py: wrapping minima, rejected frames) are binned
from the numpy decoder's images; their results rows are compared with what dbde_hip_decode_frames reports.
"""
import numpy as np
import pytest

import crafted as cr
from family_refs import hist_expect as expect
from test_gpu_project import Batch, Crafted

pytestmark = pytest.mark.gpu

MODES = ("noise8", "mixed", "flat", "smooth")
GUARD = 64
SENTINEL = 0x5A5A5A5A


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


def check(h, want, what=""):
    import torch
    got = h.counts.to(torch.int64).cpu()
    want = want.cpu()
    if not torch.equal(got, want):
        bad = (got != want).nonzero()[0].tolist()
        raise AssertionError(f"{what}: counts differ at {bad}: {int(got[tuple(bad)])} != {int(want[tuple(bad)])}")


def windows(W, H):
    out = [(0, 0, W, H), (W // 2, H - 1, 1, 1), (W - 1, 0, 1, H), (0, H // 3, W, 1)]
    if W > 3 and H > 3:
        out.append((1 + W // 7, 1 + H // 5, max(1, W // 2 - 1), max(1, H // 2 - 3)))
    return out


SHAPES = [(4096, 3072, 3), (1921, 1081, 3), (200, 123, 7), (1, 1, 5), (8, 8, 9), (9, 9, 9), (4200, 24, 3)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W,H,n", SHAPES)
def test_histograms_match_bincount(dv, codec, mode, W, H, n):
    import torch
    b = Batch(codec, mode, W, H, n)
    for k, (x, y, rw, rh) in enumerate(windows(W, H)):
        for shift, bins in ((0, None), (2, 64), (3, 20), (0, 1), (7, 2)):
            if k > 1 and (shift, bins) not in ((0, None), (3, 20)):
                continue
            h, res = codec.histogram(b.buf, b.lead, b.total, b.offs, W, H, n, x, y, rw, rh, shift=shift, bins=bins,
                                     total=True)
            codec.sync()
            nb = 256 >> shift if bins is None else bins
            want = expect(b.images, x, y, rw, rh, shift, nb)
            check(h, want, what=f"{mode} {W}x{H} {(x, y, rw, rh)} shift {shift} bins {nb}")
            assert torch.equal(h.counts.to(torch.int64).sum(1).cpu(), torch.full((n,), rw * rh, dtype=torch.int64))
            assert torch.equal(h.total.cpu(), want.sum(0).cpu()) and int(h.count.item()) == n
            assert torch.equal(res, b.results)


@pytest.mark.parametrize("slot,misalign", [(0, 1), (0, 3), (4096 * 3 + 5, 0), (20000, 2)])
def test_layouts(dv, codec, slot, misalign):
    """Concatenated streams at misaligned leads and slot layouts; stream_bytes ends exactly at the last frame."""
    W, H, n = 100, 75, 11
    b = Batch(codec, "mixed", W, H, n, slot_stride=slot, misalign=misalign)
    for (x, y, rw, rh) in [(0, 0, W, H), (3, 2, 95, 70)]:
        h, _ = codec.histogram(b.buf, b.lead, b.total, b.offs, W, H, n, x, y, rw, rh)
        codec.sync()
        check(h, expect(b.images, x, y, rw, rh, 0, 256), what=f"slot {slot} misalign {misalign}")


@pytest.mark.parametrize("W,H,n,how", [(64, 48, 40, "concat"), (200, 123, 23, "residues"), (1921, 17, 9, "slots"),
                                       (8, 8, 70, "offsets")])
def test_rejected_frames_keep_their_rows(dv, codec, W, H, n, how):
    import torch
    rng = np.random.default_rng(W * 7919 + H)
    s = Crafted(rng, W, H, n, how)
    keep = [im is not None for im in s.images]
    assert any(keep) and not all(keep)
    _, want_res = codec.decode_frames(s.buf, s.lead, s.total, s.offs, W, H, n)
    imgs = [im if im is not None else np.zeros((H, W), np.uint8) for im in s.images]
    for (x, y, rw, rh) in windows(W, H)[:3]:
        for shift, bins in ((0, 256), (4, 9)):
            out = dv.Histograms(torch.full((n, bins), -7, dtype=torch.int32, device="cuda"),
                                torch.full((bins,), 99, dtype=torch.int64, device="cuda"),
                                torch.full((1,), 99, dtype=torch.int64, device="cuda"))
            h, res = codec.histogram(s.buf, s.lead, s.total, s.offs, W, H, n, x, y, rw, rh, shift=shift, bins=bins,
                                     total=True, out=out)
            codec.sync()
            want = expect(imgs, x, y, rw, rh, shift, bins, keep=keep)
            got = h.counts.to(torch.int64).cpu()
            for f in range(n):
                if keep[f]:
                    assert torch.equal(got[f], want[f]), (how, f, (x, y, rw, rh))
                else:
                    assert (got[f] == -7).all(), f"rejected frame {f}'s row was written"
            assert torch.equal(h.total.cpu(), want.sum(0)) and int(h.count.item()) == sum(keep)
            assert torch.equal(res, want_res)


def test_wrapping_minima_bin_as_decoded_bytes(dv, codec):
    rng = np.random.default_rng(5)
    W, H, n = 40, 24, 6
    frames = [cr.craft(rng, W, H, 8, "max", "max" if f % 2 else "boundary", "ones" if f % 3 else "random",
                       header=(2, f, 0)) for f in range(n)]
    images = [cr.decode_frame(fr, W, H)[2] for fr in frames]
    assert all(im is not None for im in images)
    buf, lead, offs, total = cr.layout(frames, "concat", lead=32)
    import torch
    bb, o = torch.from_numpy(buf).cuda(), torch.from_numpy(offs).cuda()
    for shift, bins in ((0, 256), (5, 8), (1, 100)):
        h, _ = codec.histogram(bb, lead, total, o, W, H, n, shift=shift, bins=bins)
        codec.sync()
        check(h, expect(images, 0, 0, W, H, shift, bins), what=f"wrapping minima shift {shift}")


@pytest.mark.parametrize("W,H,n,win", [(200, 123, 40, (3, 5, 190, 110)), (64, 64, 600, (0, 0, 64, 64))])
def test_accumulation_splits_equal_one_call(dv, codec, W, H, n, win):
    import torch
    x, y, rw, rh = win
    b = Batch(codec, "noise8", W, H, n)
    one, _ = codec.histogram(b.buf, b.lead, b.total, b.offs, W, H, n, x, y, rw, rh, total=True)
    for cuts in ([1, 8], [n // 2]):
        acc = None
        bounds = [0] + cuts + [n]
        for lo, hi in zip(bounds, bounds[1:]):
            acc, _ = codec.histogram(b.buf, b.lead, b.total, b.offs[lo:hi], W, H, hi - lo, x, y, rw, rh,
                                     per_frame=False, total=True, out=acc, accumulate=acc is not None)
        codec.sync()
        assert torch.equal(acc.total, one.total) and torch.equal(acc.count, one.count), cuts
    check(one, expect(b.images, x, y, rw, rh, 0, 256), what="one call")


def test_zero_frames(dv, codec):
    import torch
    W, H = 200, 123
    b = Batch(codec, "mixed", W, H, 4)
    h, _ = codec.histogram(b.buf, b.lead, b.total, b.offs, W, H, 4, 7, 9, 50, 60, total=True)
    codec.sync()
    before = (h.total.clone(), h.count.clone())
    codec.histogram(b.buf, b.lead, b.total, b.offs, W, H, 0, 7, 9, 50, 60, per_frame=False, total=True, out=h,
                    accumulate=True)
    codec.sync()
    assert torch.equal(h.total, before[0]) and torch.equal(h.count, before[1])
    codec.histogram(b.buf, b.lead, b.total, b.offs, W, H, 0, 7, 9, 50, 60, per_frame=False, total=True, out=h)
    codec.sync()
    assert int(h.total.abs().sum()) == 0 and int(h.count.item()) == 0


@pytest.mark.parametrize("outputs", [(True, False), (False, True), (True, True)])
def test_guards_around_every_output(dv, codec, outputs):
    """Every output sits in a guard canvas; requested outputs are written inside their extent only."""
    import torch
    W, H, n, bins = 200, 123, 5, 50
    b = Batch(codec, "smooth", W, H, n)
    per_frame, total = outputs
    rows = torch.full((2 * GUARD + n * bins,), SENTINEL, dtype=torch.int32, device="cuda")
    tot = torch.full((2 * GUARD + bins + 1,), SENTINEL, dtype=torch.int64, device="cuda")
    out = dv.Histograms(rows[GUARD:GUARD + n * bins].view(n, bins) if per_frame else None,
                        tot[GUARD:GUARD + bins] if total else None, tot[GUARD + bins:GUARD + bins + 1] if total else None)
    h, _ = codec.histogram(b.buf, b.lead, b.total, b.offs, W, H, n, 5, 3, 131, 77, shift=2, bins=bins,
                           per_frame=per_frame, total=total, out=out)
    codec.sync()
    want = expect(b.images, 5, 3, 131, 77, 2, bins)
    r, t = rows.cpu(), tot.cpu()
    assert (r[:GUARD] == SENTINEL).all() and (r[GUARD + n * bins:] == SENTINEL).all()
    assert (t[:GUARD] == SENTINEL).all() and (t[GUARD + bins + 1:] == SENTINEL).all()
    if per_frame:
        check(h, want, what="guarded")
    else:
        assert (r == SENTINEL).all()
    if total:
        assert torch.equal(h.total.cpu(), want.sum(0).cpu()) and int(h.count.item()) == n
    else:
        assert (t == SENTINEL).all()


@pytest.mark.parametrize("mode", ("mixed", "smooth"))
def test_quantiles_equal_kthvalue(dv, codec, mode):
    import torch
    W, H, n = 1921, 1081, 4
    b = Batch(codec, mode, W, H, n)
    x, y, rw, rh = 3, 5, 1000, 700
    h, _ = codec.histogram(b.buf, b.lead, b.total, b.offs, W, H, n, x, y, rw, rh, total=True)
    codec.sync()
    win = b.images[:, y:y + rh, x:x + rw].reshape(n, -1).to(torch.int64).cpu()
    N = rw * rh
    for q in (0.0, 0.01, 0.5, 0.99, 1.0):
        k = int(np.floor(q * (N - 1))) + 1
        want = torch.kthvalue(win, k, dim=1).values
        assert torch.equal(h.quantile(q).cpu(), want), q
        allv = win.reshape(-1)
        kt = int(np.floor(q * (n * N - 1))) + 1
        assert int(h.total_quantile(q)) == int(torch.kthvalue(allv, kt).values), q
    empty = dv.Histograms(torch.zeros((2, 256), dtype=torch.int32), shift=0, bins=256)
    assert empty.quantile(0.5).tolist() == [-1, -1]


def test_argument_errors(dv, codec):
    W, H, n = 64, 48, 2
    b = Batch(codec, "mixed", W, H, n)
    for kw in (dict(shift=8, bins=1), dict(shift=0, bins=257), dict(shift=1, bins=129), dict(bins=0),
               dict(per_frame=False, total=False), dict(rw=65), dict(x=1, rw=64)):
        with pytest.raises((dv.DbdeError, ValueError)):
            codec.histogram(b.buf, b.lead, b.total, b.offs, W, H, n, **kw)
