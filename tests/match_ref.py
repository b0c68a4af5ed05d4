"""Numpy reference of the patch match (dbde_hip_match_patches): the definition, on fully decoded frames.

The search patch P of (tw + 2S) x (th + 2S) pixels is tests/patch_ref.py's patch (the patch decoder's rule, fill pixels
included); for -S <= dy, dx <= S the entry at row dy + S, column dx + S of each surface is, over the template's
footprint 0 <= i < th, 0 <= j < tw:

    prod = sum T[i][j] * P[i + dy + S][j + dx + S],   sum = sum P[...],   sq = sum P[...]^2

surfaces(P, T, S) -> (prod, sum, sq) int64 (D, D).  expected(frames, W, H, templates, S, origins, ...) ->
(prod, sum, sq (n, K, D, D) int64, used (n, K, 2) int32, live (n, K) bool); entries the call must leave untouched
(k >= count, or a frame given as None: rejected) hold UNTOUCHED / patch_ref.UNTOUCHED_ORIGIN.  Everything fits int64: an
entry is at most 128^2 * 65535^2 < 2^46.
"""
import numpy as np

import patch_ref as pr

PROD, SUM, SQ = 1, 2, 4
NAMES = ("prod", "sum", "sq")
UNTOUCHED = -1229782938247303442   # 0xEEEE... as int64: a canvas of 0xEE bytes


def surfaces(P, T, S):
    """The three D x D surfaces of template T (th, tw) over the search patch P (th + 2S, tw + 2S)."""
    th, tw = T.shape
    D = 2 * S + 1
    assert P.shape == (th + 2 * S, tw + 2 * S)
    P64, T64 = P.astype(np.int64), T.astype(np.int64)
    win = np.lib.stride_tricks.sliding_window_view(P64, (th, tw))   # (D, D, th, tw): win[r, c] = P[r:r + th, c:c + tw]
    assert win.shape[:2] == (D, D)
    return (win * T64).sum((2, 3)), win.sum((2, 3)), (win * win).sum((2, 3))


def expected(frames, W, H, templates, S, origins, counts=None, mode=pr.CLAMP, fill=0):
    """frames: n images (H x W), None for a frame the decoder rejects.  templates: (Kt, th, tw), Kt in (1, K).
    origins: (n, K, 2) ints (x, y) of the SEARCH patches."""
    templates = np.asarray(templates)
    Kt, th, tw = templates.shape
    n = len(frames)
    origins = np.asarray(origins).reshape(n, -1, 2)
    K = origins.shape[1]
    assert Kt in (1, K)
    D = 2 * S + 1
    out = [np.full((n, K, D, D), UNTOUCHED, dtype=np.int64) for _ in range(3)]
    used = np.full((n, K, 2), pr.UNTOUCHED_ORIGIN, dtype=np.int32)
    live = np.zeros((n, K), dtype=bool)
    for f in range(n):
        if frames[f] is None:
            continue
        cnt = K if counts is None else min(int(counts[f]), K)
        for k in range(cnt):
            P, used[f, k] = pr.patch(frames[f], W, H, tw + 2 * S, th + 2 * S, origins[f, k, 0], origins[f, k, 1], mode, fill)
            for o, s in zip(out, surfaces(P, templates[k if Kt > 1 else 0], S)):
                o[f, k] = s
            live[f, k] = True
    return out[0], out[1], out[2], used, live


def zncc(prod, sum_, sq, T):
    """float64 zncc surfaces from the exact integers (Python ints, so nothing rounds before the division)."""
    N = T.size
    ts, tq = int(T.astype(np.int64).sum()), int((T.astype(np.int64) ** 2).sum())
    out = np.full(prod.shape, np.nan)
    for idx in np.ndindex(prod.shape):
        p, s, q = int(prod[idx]), int(sum_[idx]), int(sq[idx])
        den = (N * tq - ts * ts) * (N * q - s * s)
        if den > 0:
            out[idx] = (N * p - ts * s) / np.sqrt(float(N * tq - ts * ts) * float(N * q - s * s))
    return out


def best(score, S, maximize=True):
    """The arg-max (arg-min) of one D x D surface, NaN never winning; ties to the smallest |dx| + |dy|, then dy, then dx.
    -> ((dx, dy), value); an all-NaN surface gives ((0, 0), nan)."""
    cands = []
    for r in range(2 * S + 1):
        for c in range(2 * S + 1):
            v = score[r, c]
            if not (isinstance(v, float) and np.isnan(v)) and not np.isnan(float(v)):
                dy, dx = r - S, c - S
                cands.append(((-v if maximize else v), abs(dx) + abs(dy), dy, dx))
    if not cands:
        return (0, 0), float("nan")
    v, _, dy, dx = min(cands)
    return (dx, dy), (-v if maximize else v)
