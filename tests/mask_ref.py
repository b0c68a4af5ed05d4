"""The threshold mask's definition in numpy (dbde_hip_decode_mask): images -> words, counts, boxes.

Test infrastructure only, imported like crafted.py (not a test module).

For the pixel at frame coordinates (X, Y) with decoded value p, L = lo[Y, X] (or the scalar lo) and Hh = hi[Y, X] (or
the scalar hi).  INSIDE sets the bit iff L <= p <= Hh, OUTSIDE iff p < L or p > Hh; L > Hh is an empty band.  The
window of frame f starts at (x, y), or at origins[f] clamped into [0, W - rw] x [0, H - rh]; the maps stay in frame
coordinates.  The mask is uint64 (n, rh, words), words = ceil(rw / 64): bit (c & 63) of word (c >> 6) of row r is
window pixel (r, c), the bits at and beyond rw are 0.  counts (uint32, (n,)) are the set bits of each frame, boxes
(int32, (n, 4)) their x_min, y_min, x_max, y_max in window coordinates, inclusive, (rw, rh, -1, -1) when there is none.
"""
import numpy as np

INSIDE, OUTSIDE = 0, 1


def words_of(rw):
    return (rw + 63) // 64


def clamp_origins(origins, W, H, rw, rh):
    o = np.asarray(origins, np.int64).reshape(-1, 2)
    return np.stack([np.clip(o[:, 0], 0, W - rw), np.clip(o[:, 1], 0, H - rh)], 1)


def verdicts(images, x, y, rw, rh, lo, hi, mode=INSIDE, origins=None):
    """bool (n, rh, rw): the bit of every window pixel.  images: (n, H, W) unsigned; lo / hi: a scalar or (H, W)."""
    images = np.asarray(images)
    n, H, W = images.shape
    org = np.tile([[x, y]], (n, 1)) if origins is None else clamp_origins(origins, W, H, rw, rh)
    out = np.zeros((n, rh, rw), bool)
    for f in range(n):
        ox, oy = int(org[f, 0]), int(org[f, 1])
        p = images[f, oy:oy + rh, ox:ox + rw].astype(np.int64)
        L = np.asarray(lo).astype(np.int64)
        Hh = np.asarray(hi).astype(np.int64)
        L = L[oy:oy + rh, ox:ox + rw] if L.ndim == 2 else L
        Hh = Hh[oy:oy + rh, ox:ox + rw] if Hh.ndim == 2 else Hh
        inside = (p >= L) & (p <= Hh)
        out[f] = ~inside if mode == OUTSIDE else inside
    return out


def pack(bits):
    """bool (n, rh, rw) -> uint64 (n, rh, words)."""
    bits = np.asarray(bits, bool)
    n, rh, rw = bits.shape
    words = words_of(rw)
    c = np.arange(rw)
    out = np.zeros((n, rh, words), np.uint64)
    weight = np.uint64(1) << (c & 63).astype(np.uint64)
    for w in range(words):
        sel = (c >> 6) == w
        out[:, :, w] = (bits[:, :, sel] * weight[sel]).sum(axis=2, dtype=np.uint64)
    return out


def unpack(words, rw):
    """uint64 (n, rh, words) -> bool (n, rh, rw)."""
    words = np.asarray(words, np.uint64)
    n, rh, nw = words.shape
    sh = np.arange(64, dtype=np.uint64)
    return (((words[..., None] >> sh) & np.uint64(1)) != 0).reshape(n, rh, nw * 64)[:, :, :rw]


def counts(bits):
    return np.asarray(bits, bool).sum(axis=(1, 2)).astype(np.uint32)


def boxes(bits):
    bits = np.asarray(bits, bool)
    n, rh, rw = bits.shape
    out = np.empty((n, 4), np.int32)
    for f in range(n):
        ys, xs = np.nonzero(bits[f])
        out[f] = (rw, rh, -1, -1) if len(xs) == 0 else (xs.min(), ys.min(), xs.max(), ys.max())
    return out


def expected(images, x, y, rw, rh, lo, hi, mode=INSIDE, origins=None):
    """-> (words uint64 (n, rh, words), counts uint32 (n,), boxes int32 (n, 4))."""
    b = verdicts(images, x, y, rw, rh, lo, hi, mode, origins)
    return pack(b), counts(b), boxes(b)
