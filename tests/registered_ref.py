"""The definition of the registered projections (dbde_hip_project_registered) in numpy over host images, window by
window (test infrastructure, like lag_ref.py; not a test module).  Independent of the call: it clamps each origin as the
header says, cuts the window out of the decoded image and reduces.  images: one (H, W) array per frame, None = rejected.
"""
import numpy as np

STATS = ("max", "min", "sum", "sumsq")
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def names_of(mask):
    return tuple(k for b, k in enumerate(STATS) if mask >> b & 1)


def clamp(origins, W, H, rw, rh):
    """int64 (n, 2): every origin clamped into [0, W - rw] x [0, H - rh]."""
    o = np.asarray(origins, np.int64).reshape(-1, 2)
    return np.stack([np.clip(o[:, 0], 0, W - rw), np.clip(o[:, 1], 0, H - rh)], 1)


def registered(images, origins, rw, rh, bits=8):
    """{"max", "min": (rh, rw) in the pixel type; "sum", "sumsq": (rh, rw) uint64; "count": accepted frames; "used":
    {frame: clamped origin} of the accepted frames}.  No accepted frame: max 0, min all ones, sums 0."""
    pix = np.uint8 if bits == 8 else np.uint16
    shape = next((im.shape for im in images if im is not None), None)
    mx = np.zeros((rh, rw), pix)
    mn = np.full((rh, rw), (1 << bits) - 1, pix)
    s = np.zeros((rh, rw), np.uint64)
    sq = np.zeros((rh, rw), np.uint64)
    used, count = {}, 0
    for f, im in enumerate(images):
        if im is None:
            continue
        H, W = shape
        x, y = (int(v) for v in clamp(origins[f], W, H, rw, rh)[0])
        win = im[y:y + rh, x:x + rw]
        assert win.shape == (rh, rw) and win.dtype == pix
        mx = np.maximum(mx, win)
        mn = np.minimum(mn, win)
        w64 = win.astype(np.uint64)
        s += w64
        sq += w64 * w64
        used[f] = (x, y)
        count += 1
    return {"max": mx, "min": mn, "sum": s, "sumsq": sq, "count": count, "used": used}


def brute(images, origins, rw, rh, W, H, bits=8):
    """The same, pixel by pixel in Python integers (the reference's own check; small cases only)."""
    top = (1 << bits) - 1
    out = {k: [[0] * rw for _ in range(rh)] for k in STATS}
    for Y in range(rh):
        for X in range(rw):
            vals = []
            for f, im in enumerate(images):
                if im is None:
                    continue
                x = min(max(int(origins[f][0]), 0), W - rw)
                y = min(max(int(origins[f][1]), 0), H - rh)
                vals.append(int(im[y + Y][x + X]))
            out["max"][Y][X] = max(vals, default=0)
            out["min"][Y][X] = min(vals, default=top)
            out["sum"][Y][X] = sum(vals)
            out["sumsq"][Y][X] = sum(v * v for v in vals)
    return out
