"""Numpy reference of the patch decode (dbde_hip_decode_patches): patches cut out of fully decoded frames.

expected(frames, W, H, pw, ph, origins, ...) -> (patches (n, K, ph, pw), used (n, K, 2) int32, live (n, K) bool).
Patches and used origins that the call must leave untouched (k >= count, or a frame given as None: rejected) hold
`untouched` / UNTOUCHED_ORIGIN and are False in live.  All arithmetic is on Python ints: any int32 origin is legal.
"""
import numpy as np

CLAMP, FILL = 0, 1
UNTOUCHED_ORIGIN = -286331154   # 0xEEEEEEEE as int32: a canvas of 0xEE bytes


def clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def patch(img, W, H, pw, ph, x, y, mode, fill=0):
    """One pw x ph patch of the H x W image img at origin (x, y) -> (patch, (used x, used y))."""
    x, y = int(x), int(y)
    if mode == CLAMP:
        assert pw <= W and ph <= H
        x, y = clamp(x, 0, W - pw), clamp(y, 0, H - ph)
        return img[y:y + ph, x:x + pw].copy(), (x, y)
    out = np.full((ph, pw), fill, dtype=img.dtype)
    x0, x1 = max(x, 0), min(x + pw, W)   # the part of the patch inside the frame, in frame coordinates
    y0, y1 = max(y, 0), min(y + ph, H)
    if x0 < x1 and y0 < y1:
        out[y0 - y:y1 - y, x0 - x:x1 - x] = img[y0:y1, x0:x1]
    return out, (x, y)


def expected(frames, W, H, pw, ph, origins, counts=None, mode=CLAMP, fill=0, untouched=0xEE, dtype=np.uint8):
    """frames: n images (H x W), None for a frame the decoder rejects.  origins: (n, K, 2) ints (x, y)."""
    origins = np.asarray(origins).reshape(len(frames), -1, 2)
    n, K = origins.shape[:2]
    out = np.full((n, K, ph, pw), untouched, dtype=dtype)
    used = np.full((n, K, 2), UNTOUCHED_ORIGIN, dtype=np.int32)
    live = np.zeros((n, K), dtype=bool)
    for f in range(n):
        if frames[f] is None:
            continue
        cnt = K if counts is None else min(int(counts[f]), K)
        for k in range(cnt):
            out[f, k], used[f, k] = patch(frames[f], W, H, pw, ph, origins[f, k, 0], origins[f, k, 1], mode, fill)
            live[f, k] = True
    return out, used, live
