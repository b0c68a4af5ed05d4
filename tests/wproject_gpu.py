"""What the GPU tests of the weighted projections share (test infrastructure, like crop_gpu.py; not a test module):
weight families, strided device weights with NaN outside the slice, crafted streams with chosen rejected frames, the
bit-for-bit comparison and the one check every case runs -- the call against tests/wproject_ref.py's chain for the
segments the plan reports."""
import numpy as np

import crafted as cr
import wproject_ref as wr

SENT_BITS = 0x7FC5A5A5          # a quiet NaN with a payload no arithmetic produces: the guard bands' sentinel
FAMILIES = ("normal", "e30", "overflow", "subnormal", "ones")


def cus_of(codec):
    import torch
    return torch.cuda.get_device_properties(codec.device).multi_processor_count


def family(rng, name, R, n):
    """(R, n) float32 weights: normal values with negatives, zeros and -0.0; 1e30; values whose products overflow to
    +inf (one sign, so that no inf - inf turns up); 1e-42 subnormals of both signs; all ones."""
    if name == "normal":
        w = rng.standard_normal((R, n)).astype(np.float32)
        w.flat[::5] = 0.0
        w.flat[2::7] = -0.0
        w.flat[3::11] *= -1000.0
        return w
    if name == "e30":
        return (rng.standard_normal((R, n)) * 1e30).astype(np.float32)
    if name == "overflow":
        return (rng.uniform(0.5, 1.0, (R, n)) * 3e38).astype(np.float32)
    if name == "subnormal":
        return (rng.integers(-3, 4, (R, n)) * np.float32(1e-42)).astype(np.float32)
    if name == "ones":
        return np.ones((R, n), np.float32)
    raise ValueError(name)


def strided(w, pad=3):
    """The weights as a column slice of a wider device tensor whose other columns are NaN: only [0, n) may be read."""
    import torch
    w = np.asarray(w, np.float32)
    R, n = w.shape
    wide = np.full((R, n + 2 * pad + 1), np.nan, np.float32)
    wide[:, pad:pad + n] = w
    return torch.from_numpy(wide).cuda()[:, pad:pad + n]


def assert_bits(got, want, what=""):
    """Bit for bit (.view(int32)); where the reference is NaN (inf - inf, NaN weights) the result must be NaN too."""
    g = got.detach().cpu().numpy() if hasattr(got, "detach") else np.asarray(got)
    want = np.asarray(want, np.float32)
    assert g.shape == want.shape, (what, g.shape, want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(g), nan), (what, "NaN positions differ")
    gb, wb = np.where(nan, 0, wr.bits(g)), np.where(nan, 0, wr.bits(want))
    if not np.array_equal(gb, wb):
        bad = tuple(np.argwhere(gb != wb)[0])
        raise AssertionError(f"{what}: differs at {bad}: {g[bad]!r} ({gb[bad] & 0xFFFFFFFF:#x}) != {want[bad]!r} "
                             f"({wb[bad] & 0xFFFFFFFF:#x}); {int((gb != wb).sum())} of {gb.size} elements")


class Stream:
    """Frames in one device buffer: buf, lead, total, offs, W, H, n and the images (None: rejected)."""

    def __init__(self, buf, lead, total, offs, W, H, images):
        self.buf, self.lead, self.total, self.offs, self.W, self.H = buf, lead, total, offs, W, H
        self.images, self.n = list(images), len(images)

    def first(self, n):
        return Stream(self.buf, self.lead, self.total, self.offs, self.W, self.H, self.images[:n])


def crafted_stream(rng, W, H, n, bits, bad=()):
    """Crafted frames (tests/crafted.py: wrapping minima, every depth pattern) with the frames in `bad` broken by one
    rule each, concatenated in one device buffer."""
    import torch
    T = cr.tiles(W, H)
    frames, images = [], []
    for f in range(n):
        fr = cr.craft(rng, W, H, bits, cr.DEPTHS[f % len(cr.DEPTHS)], cr.MINIMA[f % len(cr.MINIMA)],
                      cr.PAYLOADS[f % len(cr.PAYLOADS)])
        if f in bad:
            fr = cr.break_rule(fr, cr.BREAKS[f % len(cr.BREAKS)], bits, tile=int(rng.integers(0, T)))
        img = cr.decode_frame(fr, W, H, bits)[2]
        assert (img is None) == (f in bad), (f, "a crafted frame's verdict")
        frames.append(fr)
        images.append(img)
    buf, lead, offs, total = cr.layout(frames, "concat", lead=32)
    return Stream(torch.from_numpy(buf).cuda(), lead, total, torch.from_numpy(offs).cuda(), W, H, images)


def check(call, plan, cus, s, w, win, one_segment=False, what="", **kw):
    """One call on stream s with weights w (numpy (R, n)) against the reference chain for the plan's segments.
    Returns (WeightedProjection, results, plan)."""
    import torch
    x, y, rw, rh = win
    w = np.asarray(w, np.float32)
    p = plan(s.W, s.H, s.n, x, y, rw, rh, regressors=min(w.shape[0], 8), n_cu=cus, one_segment=one_segment)
    want, count = wr.wproject(s.images, w, x, y, rw, rh, segments=p["segments"], fps=p["frames_per_segment"])
    out, res = call(s.buf, s.lead, s.total, s.offs, s.W, s.H, s.n, strided(w), x, y, rw, rh, one_segment=one_segment, **kw)
    torch.cuda.synchronize()
    what = f"{what} {s.W}x{s.H} n={s.n} R={w.shape[0]} {win} S={p['segments']}"
    assert out.out.dtype == torch.float32 and tuple(out.out.shape) == (w.shape[0], rh, rw), what
    assert_bits(out.out, want, what)
    assert int(out.count.item()) == count, (what, "count")
    return out, res, p
