"""Numpy reference of the patch moments (dbde_hip_patch_moments): thresholded image moments of patches cut out of fully
decoded frames.

moments(img, W, H, pw, ph, x, y, mode, lo, hi, weight) -> (eight Python ints, box, used origin) for one patch;
expected(frames, ...) -> (moments (n, K, 8) object array of Python ints, boxes (n, K, 4), used (n, K, 2), live (n, K)).
The patch is patch_ref.patch(..., FILL)'s (in CLAMP mode at the clamped origin) with a mask of the pixels inside the
frame: a pixel outside the frame is part of no sum.  Every sum is a sum of Python ints, so nothing overflows (a single
pixel's term is formed in int64, where it cannot: it is below 2^35).
"""
import numpy as np

import patch_ref as pr

COUNT, VALUE, ABOVE, BELOW = 0, 1, 2, 3
WEIGHTS = ("count", "value", "above", "below")
SLOTS = ("N", "S", "Sx", "Sy", "Sxx", "Sxy", "Syy", "Sww")


def weights_of(p, lo, hi, weight):
    """The weights of the selected pixel values p (int64)."""
    if weight == COUNT:
        return p * 0 + 1
    if weight == VALUE:
        return p
    if weight == ABOVE:
        return p - lo
    assert weight == BELOW
    return hi - p


def moments(img, W, H, pw, ph, x, y, mode, lo, hi, weight):
    """One patch of the H x W image img at origin (x, y) -> ([N, S, Sx, Sy, Sxx, Sxy, Syy, Sww], (j_min, i_min, j_max,
    i_max), (used x, used y))."""
    x, y = int(x), int(y)
    if mode == pr.CLAMP:
        assert pw <= W and ph <= H
        x, y = pr.clamp(x, 0, W - pw), pr.clamp(y, 0, H - ph)
    px, used = pr.patch(img, W, H, pw, ph, x, y, pr.FILL, 0)
    inside, _ = pr.patch(np.ones((H, W), np.uint8), W, H, pw, ph, x, y, pr.FILL, 0)
    sel = (inside == 1) & (px >= lo) & (px <= hi)
    i, j = np.nonzero(sel)
    if len(i) == 0:
        return [0] * 8, (pw, ph, -1, -1), used
    # one product per selected pixel in int64 (at most 65535 * 511 * 511 < 2^35), every SUM on Python ints
    p = px[i, j].astype(np.int64)
    w = weights_of(p, int(lo), int(hi), weight)
    i, j = i.astype(np.int64), j.astype(np.int64)
    out = [len(p)] + [sum(t.tolist()) for t in (w, w * j, w * i, w * j * j, w * i * j, w * i * i, w * w)]
    return out, (int(j.min()), int(i.min()), int(j.max()), int(i.max())), used


def moments_loops(img, W, H, pw, ph, x, y, mode, lo, hi, weight):
    """The same by a plain double loop over the patch, straight from the definition."""
    x, y = int(x), int(y)
    if mode == pr.CLAMP:
        x, y = pr.clamp(x, 0, W - pw), pr.clamp(y, 0, H - ph)
    out = [0] * 8
    box = [pw, ph, -1, -1]
    for i in range(ph):
        for j in range(pw):
            fx, fy = x + j, y + i
            if not (0 <= fx < W and 0 <= fy < H):
                continue
            p = int(img[fy, fx])
            if not lo <= p <= hi:
                continue
            w = (1, p, p - lo, hi - p)[weight]
            for s, v in enumerate((1, w, w * j, w * i, w * j * j, w * i * j, w * i * i, w * w)):
                out[s] += v
            box = [min(box[0], j), min(box[1], i), max(box[2], j), max(box[3], i)]
    return out, tuple(box), (x, y)


UNTOUCHED = -0x1111111111111112   # 0xEEEEEEEEEEEEEEEE as int64: a canvas of 0xEE bytes


def expected(frames, W, H, pw, ph, origins, counts, mode, lo, hi, weight):
    """frames: n images (H x W), None for a frame the decoder rejects.  origins: (n, K, 2) ints (x, y).  Entries the call
    must leave untouched hold the 0xEE canvas (UNTOUCHED, pr.UNTOUCHED_ORIGIN) and are False in live."""
    origins = np.asarray(origins).reshape(len(frames), -1, 2)
    n, K = origins.shape[:2]
    mom = np.full((n, K, 8), UNTOUCHED, dtype=object)
    box = np.full((n, K, 4), pr.UNTOUCHED_ORIGIN, dtype=np.int64)
    used = np.full((n, K, 2), pr.UNTOUCHED_ORIGIN, dtype=np.int64)
    live = np.zeros((n, K), dtype=bool)
    for f in range(n):
        if frames[f] is None:
            continue
        cnt = K if counts is None else min(int(counts[f]), K)
        for k in range(cnt):
            m, b, u = moments(frames[f], W, H, pw, ph, origins[f, k, 0], origins[f, k, 1], mode, lo, hi, weight)
            mom[f, k], box[f, k], used[f, k] = m, b, u
            live[f, k] = True
    return mom, box, used, live
