"""The shared case list of the patch match tests (tests/test_match_ref.py caps every case on the CPU before any GPU run;
tests/test_gpu_match.py and test_gpu_match16.py run them), and the shift-recovery scenes of the registration tests.

A case's content is made here in numpy, so the CPU tests see exactly what the GPU tests encode: noise frames (every
pixel random, so that a kernel which mixes up axes or offsets cannot pass), noise templates, and origins by kind.
Frames run from 72 x 56 up to 200 x 136 and beyond them by a partial last tile row and column.
"""
import numpy as np

import patch_ref as pr

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1

TEMPLATES = [(1, 1), (1, 9), (9, 1), (3, 5), (7, 7), (8, 8), (16, 12), (33, 31)]   # (tw, th)
RADII = [0, 1, 2, 8, 16]


def case(name, W, H, n, tw, th, S, origins, mode=pr.FILL, fill=0, shared=False, counts=None, stats=7, K=None):
    return dict(name=name, W=W, H=H, n=n, tw=tw, th=th, S=S, origins=origins, mode=mode, fill=fill, shared=shared,
                counts=counts, stats=stats, K=K)


def _cases():
    out = []
    # every template size with every radius, dealt over the geometries, both edge modes and the fill values
    geos = [(75, 61, 2), (72, 56, 3), (197, 131, 2), (200, 136, 2), (139, 99, 3)]
    i = 0
    for tw, th in TEMPLATES:
        for S in RADII:
            W, H, n = geos[i % len(geos)]
            mode = pr.CLAMP if i % 2 and tw + 2 * S <= W and th + 2 * S <= H else pr.FILL
            out.append(case(f"t{tw}x{th}_S{S}", W, H, n, tw, th, S, "mixed", mode, fill=(0x5A, 0, 0xFF)[i % 3],
                            shared=i % 3 == 1, K=(3, 1, 5)[i % 3]))
            i += 1
    # the largest legal case: the search patch is 160 x 160, larger than the frame is high
    out.append(case("largest", 197, 131, 2, 128, 128, 16, "mixed", pr.FILL, fill=7, K=3))
    out.append(case("largest_clamp", 200, 163, 2, 128, 128, 16, "clamp_sides", pr.CLAMP, K=None))
    # all 64 residues (x & 7, y & 7) of the origin in one call
    out.append(case("residues", 139, 99, 2, 16, 12, 2, "residues", pr.CLAMP))
    out.append(case("residues_fill", 75, 61, 2, 7, 7, 8, "residues", pr.FILL, fill=0x33))
    # FILL over each edge and corner, wholly outside, int32 extremes; CLAMP clamped on every side
    out.append(case("fill_edges", 75, 61, 3, 8, 8, 2, "fill_edges", pr.FILL, fill=0xC3))
    out.append(case("fill_edges_wide", 197, 131, 2, 33, 31, 8, "fill_edges", pr.FILL, fill=1, shared=True))
    out.append(case("clamp_sides", 139, 99, 2, 16, 12, 8, "clamp_sides", pr.CLAMP))
    # n_templates 1 and K for K = 1, 3 and 70; counts 0, partial and larger than K
    for K in (1, 3, 70):
        for shared in (False, True):
            out.append(case(f"K{K}_{'shared' if shared else 'own'}", 72, 56, 4, 7, 7, 1, "random", pr.FILL, fill=9,
                            shared=shared, counts=[K + 5, 0, (K + 1) // 2, K], K=K))
    # every stats mask
    for m in range(1, 8):
        out.append(case(f"stats{m}", 75, 61, 2, 9, 1 + m, 2, "random", pr.CLAMP, stats=m, K=4))
    return out


CASES = _cases()
IDS = [c["name"] for c in CASES]


def top(bits):
    return 255 if bits == 8 else 65535


def fill_of(c, bits):
    """The case's fill pixel: its byte, twice for 16-bit pixels."""
    return c["fill"] * (1 if bits == 8 else 257)


def origins_of(c, rng):
    """(n, K, 2) int64 origins of the SEARCH patches of case c."""
    W, H, n, S = c["W"], c["H"], c["n"], c["S"]
    pw, ph = c["tw"] + 2 * S, c["th"] + 2 * S
    mx, my = max(W - pw, 0), max(H - ph, 0)
    kind = c["origins"]
    if kind == "residues":
        base = [(8 * int(rng.integers(0, mx // 8)) + rx, 8 * int(rng.integers(0, my // 8)) + ry) for ry in range(8) for rx in range(8)]
    elif kind == "fill_edges":
        base = [(-pw // 2, my // 2), (W - pw // 2, my // 2), (mx // 2, -ph // 2), (mx // 2, H - ph // 2),      # each edge
                (-3, -2), (W - pw + 3, -1), (-1, H - ph + 2), (W - pw // 2, H - ph // 2),                      # each corner
                (-pw, 0), (W, 5), (3, -ph), (4, H), (-pw - 9, -ph - 9), (W + 100, H + 100),                    # wholly outside
                (I32_MIN, I32_MAX), (I32_MAX, I32_MIN), (I32_MIN, 0), (0, I32_MAX), (I32_MAX, I32_MAX), (I32_MIN, I32_MIN),
                (-pw + 1, -ph + 1), (W - 1, H - 1), (mx // 2, my // 2)]
    elif kind == "clamp_sides":
        base = [(-5, my // 2), (W, my // 2), (mx // 2, -7), (mx // 2, H + 3), (-1, -1), (W - pw + 1, H - ph + 1),
                (I32_MIN, I32_MAX), (I32_MAX, I32_MIN), (0, 0), (mx, my), (mx // 2, my // 2), (mx - 1, my - 1)]
    elif kind == "random":
        base = [(int(rng.integers(-pw, W + 1)), int(rng.integers(-ph, H + 1))) for _ in range(c["K"])]
        if c["mode"] == pr.CLAMP:
            base = [(int(rng.integers(0, mx + 1)), int(rng.integers(0, my + 1))) for _ in range(c["K"])]
    else:   # "mixed": inside, over an edge, at a tile boundary
        base = [(mx // 2, my // 2), (mx, my), (0, 0), (-3, my // 3), (mx // 3, H - ph + 2), (8, 8), (7, 9)][:c["K"]]
        base += [(int(rng.integers(-2, mx + 3)), int(rng.integers(-2, my + 3))) for _ in range(c["K"] - len(base))]
    base = np.array(base, np.int64)
    return np.stack([base[rng.permutation(len(base))] if kind != "residues" else base for _ in range(n)])


def content(c, bits):
    """-> (frames (n, H, W), templates (Kt, th, tw), origins (n, K, 2) int64, counts or None) of case c: noise over the
    whole range of the pixel type (8 bits: half the frames in a narrow range, so that shallow tiles occur)."""
    rng = np.random.default_rng(sum(map(ord, c["name"])) * 7919 + bits)
    dt = np.uint8 if bits == 8 else np.uint16
    frames = rng.integers(0, top(bits) + 1, size=(c["n"], c["H"], c["W"])).astype(dt)
    frames[1::2] = (frames[1::2] >> (bits - 5)) + dt(top(bits) // 3)   # 5-bit noise on a level
    org = origins_of(c, rng)
    K = org.shape[1]
    templates = rng.integers(0, top(bits) + 1, size=(1 if c["shared"] else K, c["th"], c["tw"])).astype(dt)
    counts = c["counts"]
    return frames, templates, org, (None if counts is None else list(counts[:c["n"]]))


# ---- the shift-recovery scenes --------------------------------------------------------------------------------------
SCENE = dict(W=200, H=136, n=9, tw=32, th=32, S=8, margin=8,
             shifts=[(0, 0), (6, -6), (-6, 6), (1, 0), (0, -1), (-3, 5), (4, 4), (-5, -2), (2, 3)],
             positions=[(30, 24), (140, 20), (84, 52), (24, 90), (150, 88)])


def scene_frames(sc=SCENE, seed=5):
    """-> (reference (H, W) uint8, frames (n, H, W) uint8): a smooth scene (blurred blobs on a gradient, with a grain of
    +-2 levels that moves with the scene), frame f moved by shifts[f]: frame[y][x] = reference'[y - dy][x - dx], all cut
    out of one larger image, so that registered[Y][X] = frame[Y + dy][X + dx] is the reference."""
    W, H, m = sc["W"], sc["H"], sc["margin"]
    rng = np.random.default_rng(seed)
    BH, BW = H + 2 * m, W + 2 * m
    yy, xx = np.mgrid[0:BH, 0:BW].astype(np.float64)
    big = 60.0 + 0.15 * xx + 0.1 * yy
    for _ in range(60):
        cx, cy, r, a = rng.uniform(0, BW), rng.uniform(0, BH), rng.uniform(3, 9), rng.uniform(20, 90)
        big += a * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * r * r))
    big = np.clip(np.round(big + rng.integers(-2, 3, size=big.shape)), 0, 255).astype(np.uint8)
    frames = np.stack([big[m - dy:m - dy + H, m - dx:m - dx + W] for dx, dy in sc["shifts"]])
    return big[m:m + H, m:m + W].copy(), frames
