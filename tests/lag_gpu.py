"""What the tests of the lag projections share (test infrastructure, like pairs_gpu.py; not a test module): the streams
(crafted on the host from a seed, so that the CPU test can judge their content before any GPU run), the cap that keeps
a case from passing with the wrong lag, a pixel paired with itself or nothing counted, and the one check every GPU case
runs -- the call against tests/lag_ref.py, by equality."""
import numpy as np

import crafted as cr
import lag_ref as lr

LAGS = tuple(range(1, 9))
# each statistic alone, all five, and two mixed masks that map to different instances (3 | 8 -> 31, 4 | 16 -> 28)
MASKS = (1, 2, 4, 8, 16, 31, 11, 20)
FRAME = (200, 123)                       # odd width: one piece at 8 bits, two at 16
WIDE = (300, 20)                         # two pieces at 8 bits
WINDOWS = [(0, 0, 200, 123), (3, 5, 41, 27), (8, 16, 189, 104), (97, 67, 1, 1)]
SMALL = WINDOWS[1]
PIX = {8: np.uint8, 16: np.uint16}


def host_frames(kind, seed, W, H, n, bits, bad=()):
    """The frames and images (None = rejected) of a stream, on the host, from rng = default_rng(seed).
    "crafted": wproject_gpu.crafted_stream's (the same draws in the same order): every depth pattern, minimum family and
      payload family of tests/crafted.py in turn, the frames in `bad` broken by one rule each.
    "noise": full-depth tiles with random minima and payloads, so every pixel is uniform over the pixel type and
      independent from frame to frame (a one-pixel window still tells the lags apart); `bad` likewise.
    "alternating": frames of constant 0 and constant 255 / 65,535 in turn (depth 0, the minimum the value)."""
    rng = np.random.default_rng(seed)
    T = cr.tiles(W, H)
    frames, images = [], []
    for f in range(n):
        if kind == "crafted":
            fr = cr.craft(rng, W, H, bits, cr.DEPTHS[f % len(cr.DEPTHS)], cr.MINIMA[f % len(cr.MINIMA)],
                          cr.PAYLOADS[f % len(cr.PAYLOADS)])
        elif kind == "noise":
            fr = cr.craft(rng, W, H, bits, "max", "random", "random")
        else:
            assert kind == "alternating"
            fr = cr.frame(np.zeros(T, np.uint8), np.full(T, ((1 << bits) - 1) * (f & 1)), [], (2, f, 0), bits)
        if f in bad:
            fr = cr.break_rule(fr, cr.BREAKS[f % len(cr.BREAKS)], bits, tile=int(rng.integers(0, T)))
        img = cr.decode_frame(fr, W, H, bits)[2]
        assert (img is None) == (f in bad), (f, "a crafted frame's verdict")
        frames.append(fr)
        images.append(img)
    return frames, images


_HOST, _DEVICE = {}, {}


def host_images(kind, seed, W, H, n, bits, bad=()):
    key = (kind, seed, W, H, n, bits, tuple(bad))
    if key not in _HOST:
        _HOST[key] = host_frames(*key)
    return _HOST[key][1]


def stream(kind, seed, W, H, n, bits, bad=()):
    """The device stream of host_frames(...) (a wproject_gpu.Stream: frames concatenated behind a lead of 32 bytes),
    cached for the session."""
    import torch
    import wproject_gpu as wg
    key = (kind, seed, W, H, n, bits, tuple(bad))
    if key not in _DEVICE:
        images = host_images(*key)
        if kind == "crafted":   # wproject_gpu.crafted_stream itself; the host copy the CPU test judged must be its twin
            s = wg.crafted_stream(np.random.default_rng(seed), W, H, n, bits, bad=tuple(bad))
            assert all((a is None) == (b is None) and (a is None or np.array_equal(a, b)) for a, b in zip(s.images, images))
        else:
            buf, lead, offs, total = cr.layout(_HOST[key][0], "concat", lead=32)
            s = wg.Stream(torch.from_numpy(buf).cuda(), lead, total, torch.from_numpy(offs).cuda(), W, H, images)
        _DEVICE[key] = s
    return _DEVICE[key]


def seed_of(W, H, bits):
    return W * 7 + H + bits


def cap(images, lag, win, lead=0, bits=8):
    """The cap on the expected planes, where at least 3 pairs are counted: product is not all zero and differs from the
    sum of squares over the later frames (a lag of 0); every plane differs from the same plane for lag - 1 and lag + 1
    where those lags are valid (the wrong slot of the ring); absdiff and maxdiff are not all zero."""
    want = lr.lag(images, lag, *win, lead=lead, bits=bits)
    if want["pairs"] < 3:
        return want
    assert want["product"].any(), "product is all zero"
    assert not np.array_equal(want["product"], lr.sumsq_later(images, lag, *win, lead=lead)), "product equals sumsq"
    assert want["absdiff"].any() and want["maxdiff"].any(), "absdiff or maxdiff is all zero"
    for other in (lag - 1, lag + 1):
        if 1 <= other <= 8:
            wrong = lr.lag(images, other, *win, lead=lead, bits=bits)
            for k in lr.STATS:
                assert not np.array_equal(want[k], wrong[k]), f"{k} is the same for lag {lag} and lag {other}"
    return want


def planes(out):
    """LagProjection's requested planes on the host: the U64 bits the int64 tensors hold, maxdiff in the pixel type."""
    got = {}
    for k in out.stats:
        t = getattr(out, k).cpu().numpy()
        got[k] = t.view(np.uint64) if k != "maxdiff" else t.view(np.uint16) if t.dtype == np.int16 else t
    return got


def compare(out, want, names, what):
    import torch
    got = planes(out)
    assert tuple(got) == tuple(names), (what, tuple(got), names)
    for k in names:
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, (what, k, got[k].dtype)
        if not np.array_equal(got[k], want[k]):
            bad = tuple(np.argwhere(got[k] != want[k])[0])
            raise AssertionError(f"{what}: {k} differs at {bad}: {got[k][bad]} != {want[k][bad]}; "
                                 f"{int((got[k] != want[k]).sum())} of {got[k].size} elements")
    assert out.pairs.dtype == torch.int64 and int(out.pairs.item()) == want["pairs"], (what, "pairs")
    assert int(out.count.item()) == want["count"], (what, "count")


def check(codec, s, lag, win, mask=31, lead=0, bits=8, what="", use_cap=True, **kw):
    """One call on stream s (wproject_gpu.Stream) against lag_ref.  Returns (out, results)."""
    import torch
    want = cap(s.images, lag, win, lead, bits) if use_cap else lr.lag(s.images, lag, *win, lead=lead, bits=bits)
    call = codec.project_lag if bits == 8 else codec.project_lag16
    names = lr.names_of(mask)
    out, res = call(s.buf, s.lead, s.total, s.offs, s.W, s.H, s.n, lag, names, lead, *win, **kw)
    torch.cuda.synchronize()
    compare(out, want, names, f"{what} {s.W}x{s.H} n={s.n} lag={lag} lead={lead} mask={mask} {win} {bits}-bit")
    assert out.lag == lag
    return out, res


def split_on_device(codec, s, lag, win, B, mask=31, bits=8):
    """The header's split rule as accumulating calls on slices of the stream's offsets."""
    call = codec.project_lag if bits == 8 else codec.project_lag16
    names = lr.names_of(mask)
    out = None
    for lo, cnt, lead in lr.split_calls(s.n, lag, B):
        out, _ = call(s.buf, s.lead, s.total, s.offs[lo:], s.W, s.H, cnt, lag, names, lead, *win, out=out,
                      accumulate=out is not None)
    codec.sync()
    return out
