"""GPU: binned decode -- dbde_hip_decode_binned (Codec.decode_binned).

Expected values are exact integers: tests/binned_ref.py's definition (numpy reduceat over the window) applied to the
images dbde_hip_decode_frames writes for the same frames, to the CPU oracle's and the reference's images of the
device-encoded bytes, and to the numpy decoder's images of crafted frames (tests/crafted.py: wrapping minima, rejected
frames).  Every plane sits at an odd element offset inside a sentinel-filled buffer whose guard elements are checked.
Results rows are compared with what dbde_hip_decode_frames reports.
"""
import numpy as np
import pytest

import binned_ref as br
import crafted as cr
from test_gpu_project import Batch, Crafted

pytestmark = pytest.mark.gpu

MODES = ("noise8", "mixed", "flat", "smooth")
BINS = (2, 4, 8)
ALL = ("sum", "max", "min")
GUARD = 40
SENT = {"sum": 0x5A5A, "max": 0x5A, "min": 0x5A}
SHAPES = [(4096, 3072, 3), (1921, 1081, 3), (200, 123, 7), (1, 1, 5), (8, 8, 9), (9, 9, 9), (4200, 24, 3)]


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


class Planes:
    """A Binned whose planes start GUARD + odd elements into sentinel-filled buffers (odd: 1 for the first plane, 3, 5
    for the next ones, so that a U16 plane is 2-byte but not 4-byte aligned)."""

    def __init__(self, dv, n, rw, rh, b, stats, pix=1):
        import torch
        oh, ow = br.out_shape(rw, rh, b)
        self.n, self.oh, self.ow, self.stats, self.bufs = n, oh, ow, stats, {}
        dtypes = {"sum": torch.int16, "max": torch.uint8, "min": torch.uint8} if pix == 1 else \
                 {"sum": torch.int32, "max": torch.int16, "min": torch.int16}
        self.sent = dict(SENT) if pix == 1 else {"sum": 0x5A5A5A5A, "max": 0x5A5A, "min": 0x5A5A}
        views = {}
        for k, s in enumerate(stats):
            odd = 2 * k + 1
            buf = torch.full((2 * GUARD + odd + n * oh * ow,), self.sent[s], dtype=dtypes[s], device="cuda")
            self.bufs[s] = (buf, GUARD + odd)
            views[s] = buf[GUARD + odd: GUARD + odd + n * oh * ow].view(n, oh, ow)
        self.out = dv.Binned(**views)

    def read(self):
        """{stat: int64 (n, oh, ow)} of the unsigned element values, after checking the guards."""
        got = {}
        for s, (buf, lo) in self.bufs.items():
            h = buf.cpu().numpy()
            h = h.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[h.itemsize]).astype(np.int64)
            hi = lo + self.n * self.oh * self.ow
            assert (h[:lo] == self.sent[s]).all(), f"wrote in front of the {s} plane"
            assert (h[hi:] == self.sent[s]).all(), f"wrote behind the {s} plane"
            got[s] = h[lo:hi].reshape(self.n, self.oh, self.ow)
        return got


def run(dv, codec, buf, lead, total, offs, W, H, n, b, win, stats, call="decode_binned", pix=1):
    x, y, rw, rh = win
    pl = Planes(dv, n, rw, rh, b, stats, pix=pix)
    out, res = getattr(codec, call)(buf, lead, total, offs, W, H, n, b, x, y, rw, rh, out=pl.out)
    codec.sync()
    assert out is pl.out and out.bin == b and tuple(out.pixels.shape) == (pl.oh, pl.ow)
    assert (out.pixels.cpu().numpy() == br.bin_pixels(rw, rh, b)).all()
    return pl.read(), res


def compare(got, want, stats, what, keep=None, sent=SENT):
    for s in stats:
        for f in range(got[s].shape[0]):
            if keep is not None and not keep[f]:
                assert (got[s][f] == sent[s]).all(), f"{what}: rejected frame {f}'s {s} plane was written"
                continue
            if not (got[s][f] == want[s][f]).all():
                i, j = np.argwhere(got[s][f] != want[s][f])[0]
                raise AssertionError(f"{what}: {s} of frame {f} differs at bin ({i}, {j}): "
                                     f"{got[s][f][i, j]} != {want[s][f][i, j]}")
    assert set(got) == set(stats)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W,H,n", SHAPES)
def test_planes_match_binned_decoded_images(dv, codec, mode, W, H, n):
    import torch
    bt = Batch(codec, mode, W, H, n)
    images = bt.images.cpu().numpy()
    for b in BINS:
        wins = br.windows(W, H, b)
        assert len(wins) == 5 or min(W, H) < 12
        for win in wins:
            want = br.binned_reduceat(images, *win, b)
            for stats in (ALL, ("sum",)):
                got, res = run(dv, codec, bt.buf, bt.lead, bt.total, bt.offs, W, H, n, b, win, stats)
                compare(got, want, stats, f"{mode} {W}x{H} bin {b} window {win} {stats}")
                assert torch.equal(res, bt.results)


def packed_frames(bt):
    host = bt.buf.cpu().numpy()
    o, r = bt.offs.cpu().numpy(), bt.results.cpu().numpy()
    return [host[bt.lead + int(o[f]): bt.lead + int(o[f]) + int(r[f][3])] for f in range(bt.n)]


def test_planes_match_binned_oracle_images(dv, codec, oracle):
    W, H, n = 203, 117, 4
    bt = Batch(codec, "mixed", W, H, n)
    assert [int(v) for v in bt.results.cpu().numpy()[:, 3]] == list(np.diff(list(bt.offs.cpu().numpy()) + [bt.total]))
    images = np.stack([oracle.unpack_frame(p, W, H)[2] for p in packed_frames(bt)])
    for b in BINS:
        for win in br.windows(W, H, b):
            got, _ = run(dv, codec, bt.buf, bt.lead, bt.total, bt.offs, W, H, n, b, win, ALL)
            compare(got, br.binned_reduceat(images, *win, b), ALL, f"oracle bin {b} window {win}")


def test_planes_match_binned_reference_images(dv, codec, reference):
    W, H, n = 203, 117, 4
    bt = Batch(codec, "smooth", W, H, n)
    images = np.stack([reference.unpack_frame(p, W, H)[2] for p in packed_frames(bt)])
    for b in BINS:
        for win in br.windows(W, H, b):
            got, _ = run(dv, codec, bt.buf, bt.lead, bt.total, bt.offs, W, H, n, b, win, ALL)
            compare(got, br.binned_reduceat(images, *win, b), ALL, f"reference bin {b} window {win}")


@pytest.mark.parametrize("W,H,n,how", [(64, 48, 40, "concat"), (200, 123, 23, "residues"), (1921, 17, 9, "slots"),
                                       (8, 8, 70, "offsets"), (4200, 9, 7, "concat")])
def test_crafted_and_rejected_frames(dv, codec, W, H, n, how):
    """Every depth, wrapping minima, random payload; rejected frames keep the sentinel, results are decode_frames'."""
    import torch
    rng = np.random.default_rng(W * 7919 + H)
    s = Crafted(rng, W, H, n, how)
    keep = [im is not None for im in s.images]
    assert any(keep) and not all(keep)
    _, want_res = codec.decode_frames(s.buf, s.lead, s.total, s.offs, W, H, n)
    imgs = np.stack([im if im is not None else np.zeros((H, W), np.uint8) for im in s.images])
    for b in BINS:
        for win in br.windows(W, H, b):
            for stats in (ALL, ("sum",)):
                got, res = run(dv, codec, s.buf, s.lead, s.total, s.offs, W, H, n, b, win, stats)
                compare(got, br.binned_reduceat(imgs, *win, b), stats, f"crafted {how} bin {b} {win}", keep=keep)
                assert torch.equal(res, want_res)


def test_wrapping_minima_bin_as_decoded_bytes(dv, codec):
    import torch
    rng = np.random.default_rng(5)
    W, H, n = 43, 27, 6
    frames = [cr.craft(rng, W, H, 8, "max", "max" if f % 2 else "boundary", "ones" if f % 3 else "random",
                       header=(2, f, 0)) for f in range(n)]
    images = [cr.decode_frame(fr, W, H)[2] for fr in frames]
    assert all(im is not None for im in images)
    buf, lead, offs, total = cr.layout(frames, "concat", lead=32)
    bb, o = torch.from_numpy(buf).cuda(), torch.from_numpy(offs).cuda()
    for b in BINS:
        for win in br.windows(W, H, b):
            got, _ = run(dv, codec, bb, lead, total, o, W, H, n, b, win, ALL)
            compare(got, br.binned_reduceat(np.stack(images), *win, b), ALL, f"wrapping minima bin {b} {win}")


@pytest.mark.parametrize("slot,misalign", [(0, 1), (0, 3), (4096 * 3 + 5, 0), (20000, 2)])
def test_layouts(dv, codec, slot, misalign):
    """Concatenated streams at misaligned leads and slot layouts; stream_bytes ends exactly at the last frame."""
    W, H, n = 100, 75, 11
    bt = Batch(codec, "mixed", W, H, n, slot_stride=slot, misalign=misalign)
    images = bt.images.cpu().numpy()
    for b in BINS:
        for win in [(0, 0, W, H), (b, b, 91, 61)]:
            got, _ = run(dv, codec, bt.buf, bt.lead, bt.total, bt.offs, W, H, n, b, win, ALL)
            compare(got, br.binned_reduceat(images, *win, b), ALL, f"slot {slot} misalign {misalign} bin {b} {win}")


def test_zero_frames_and_absent_planes(dv, codec):
    import torch
    W, H, n = 200, 123, 4
    bt = Batch(codec, "mixed", W, H, n)
    pl = Planes(dv, n, 191, 113, 4, ALL)
    codec.decode_binned(bt.buf, bt.lead, bt.total, bt.offs, W, H, 0, 4, 8, 8, 191, 113, out=pl.out)
    codec.sync()
    got = pl.read()
    assert all((got[s] == SENT[s]).all() for s in ALL), "n == 0 wrote a plane"
    out, res = codec.decode_binned(bt.buf, bt.lead, bt.total, bt.offs, W, H, 0, 2)
    assert tuple(out.sum.shape) == (0, 62, 100) and tuple(res.shape) == (0, 4)
    # a plane given as None is neither written nor required
    images = bt.images.cpu().numpy()
    for stats in (("max",), ("min",), ("sum", "min"), ("max", "min")):
        got, _ = run(dv, codec, bt.buf, bt.lead, bt.total, bt.offs, W, H, n, 4, (8, 8, 191, 113), stats)
        compare(got, br.binned_reduceat(images, 8, 8, 191, 113, 4), stats, f"planes {stats}")
    out, _ = codec.decode_binned(bt.buf, bt.lead, bt.total, bt.offs, W, H, n, 8, stats=("max",))
    codec.sync()
    assert out.sum is None and out.min is None and out.max.dtype == torch.uint8
    assert (out.max.cpu().numpy() == br.binned_reduceat(images, 0, 0, W, H, 8)["max"]).all()
    full, _ = codec.decode_binned(bt.buf, bt.lead, bt.total, bt.offs, W, H, n, 8, 8, 8, 191, 113)
    codec.sync()
    want = br.binned_reduceat(images, 8, 8, 191, 113, 8)["sum"] / br.bin_pixels(191, 113, 8)
    assert np.allclose(full.mean().cpu().numpy(), want.astype(np.float32), rtol=1e-6, atol=0)


def test_timing_slots(dv, codec):
    W, H, n = 300, 200, 2
    bt = Batch(codec, "mixed", W, H, n)
    codec.timing(True)
    codec.timing_read(reset=True)
    codec.decode_binned(bt.buf, bt.lead, bt.total, bt.offs, W, H, n, 4)
    t = codec.timing_read(reset=True)
    codec.timing(False)
    assert [t[k][1] for k in ("encode", "decode_index", "decode", "scan")] == [0, 1, 1, 0]


def test_argument_errors(dv, codec):
    import torch
    W, H, n = 64, 48, 2
    bt = Batch(codec, "mixed", W, H, n)
    for kw in (dict(bin=3), dict(bin=16), dict(bin=0), dict(bin=4, x=2), dict(bin=8, y=4), dict(bin=2, rw=65),
               dict(bin=2, x=2, rw=64), dict(bin=2, rh=0), dict(bin=2, stats=())):
        b = kw.pop("bin")
        with pytest.raises((dv.DbdeError, ValueError)):
            codec.decode_binned(bt.buf, bt.lead, bt.total, bt.offs, W, H, n, b, **kw)
    raw = torch.zeros(2 * n * 24 * 32 + 2, dtype=torch.uint8, device="cuda")   # a U16 plane at an odd address
    rc = codec.L.dbde_hip_decode_binned(codec.h, bt.buf.data_ptr() + bt.lead, bt.total, bt.offs.data_ptr(), W, H, n,
                                        0, 0, W, H, 2, raw.data_ptr() + 1, None, None, None)
    assert rc == dv.ERR_ARG
