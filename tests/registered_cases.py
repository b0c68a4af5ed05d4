"""The cases of the registered projections' tests (test infrastructure; not a test module): streams by their seed
(lag_gpu.host_frames' kinds), window sizes and per-frame origins.  tests/test_registered_ref.py holds the cap on every
one of them before any GPU run; tests/test_gpu_registered.py runs them.

A case is (name, spec, rw, rh, origins, mask): spec = lag_gpu.stream's arguments, origins an int64 (n, 2) array.
"""
import numpy as np

import registered_ref as rr

FRAME = (77, 45)                 # partial edge tiles both ways
WINDOW = (41, 27)
BIG = (200, 123)
WIDE = (300, 20)
LONG = (4107, 17)                # 514 tiles across: a tile row of two index chunks
MASKS = (1, 2, 4, 8, 15, 5, 10)  # each statistic alone, all four, two mixed masks (both run instance 15)
I32_MIN, I32_MAX = rr.I32_MIN, rr.I32_MAX
N_ALL = 67
BAD = (0, 22, 23, 33, 45, 46, 66)   # first, middle, last, and both sides of the borders of 3 segments of 23 frames


def seed_of(W, H, bits, salt=0):
    return W * 11 + H * 3 + bits + 1000 * salt


def noise(W, H, n, bits, salt=0):
    return ("noise", seed_of(W, H, bits, salt), W, H, n, bits, ())


def crafted(W, H, n, bits, bad=()):
    return ("crafted", seed_of(W, H, bits, 7), W, H, n, bits, tuple(bad))


def residue_origin(a, b, k=0):
    """An origin with residues (a, b) inside [0, 36] x [0, 18], the k-th of three that differ by whole tiles."""
    return (a + 8 * (0, 1, 3)[k], b + 8 * (0, 1, 0)[k])


def residues_each(bits):
    """Each residue (x & 7, y & 7) alone: three frames whose origins share it and differ by whole tiles."""
    spec = noise(*FRAME, 3, bits)
    return [(f"residue {a},{b}", spec, *WINDOW, np.array([residue_origin(a, b, k) for k in range(3)], np.int64), 15)
            for b in range(8) for a in range(8)]


def all_origins():
    """67 origins for FRAME / WINDOW: every residue once, then three corners."""
    o = [(i % 8 + 8 * ((i * 3) % 4), i // 8 + 8 * ((i * 5) % 2)) for i in range(64)] + [(36, 18), (0, 0), (36, 0)]
    return np.array(o, np.int64)


def residues_all(bits):
    return [("all residues", noise(*FRAME, N_ALL, bits, 1), *WINDOW, all_origins(), 15)]


def windows(bits):
    W, H = FRAME
    junk = np.array([(I32_MAX, -5), (3, 4), (-1, I32_MIN), (60, 60), (0, 0)], np.int64)
    spread = np.array([(0, 0), (76, 44), (13, 7), (40, 44), (76, 3)], np.int64)
    edge = np.array([(40, 24), (0, 0), (40, 0), (3, 24), (17, 11)], np.int64)      # (W - rw, H - rh) and others
    edge48 = np.array([(40, 27), (0, 0), (40, 5), (3, 27), (17, 11)], np.int64)
    return [("full frame", noise(W, H, 5, bits, 2), W, H, junk, 15),
            ("1x1", noise(W, H, 5, bits, 2), 1, 1, spread, 15),
            ("37x21 at the far corner", noise(W, H, 5, bits, 2), 37, 21, edge, 15),
            ("37x21, H a multiple of 8", noise(W, 48, 5, bits, 2), 37, 21, edge48, 15)]


def wide(bits):
    """rw = 290: two pieces of 248 columns at 8 bits, three of 120 at 16; the x shifts move columns between the
    pieces' source tiles."""
    W, H = WIDE
    o = np.array([(0, 0), (3, 1), (8, 3), (10, 2), (5, 0), (7, 3), (1, 1)], np.int64)
    return [("wide", noise(W, H, 7, bits, 3), 290, 17, o, 15)]


def long_row(bits):
    """A tile row of more than 512 tiles.  The last piece starts at output column 3968 (8 bits: 16 * 248) or 3960
    (16 bits: 33 * 120); the x origins put its first source tile at 508 / 512 (8 bits) or 507 / 512 (16 bits), and the
    y origins 3, 5 and 1 make the band span two tile rows."""
    W, H = LONG
    rw, xs = (3975, (100, 132)) if bits == 8 else (3965, (100, 140))
    o = np.array([(xs[f % 2], (3, 5, 8, 1, 0)[f % 5]) for f in range(9)], np.int64)
    return [("long row", noise(W, H, 9, bits, 4), rw, 9, o, 15)]


def segment_origins(n, W, H, rw, rh, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, W - rw + 1, n), rng.integers(0, H - rh + 1, n)], 1).astype(np.int64)


def segments(bits):
    W, H = BIG
    return [("segments", noise(W, H, 70, bits, 5), 150, 100, segment_origins(70, W, H, 150, 100, 5), 15)]


def rejected(bits):
    """Crafted streams with broken frames whose origin rows hold int32 extremes; the last case rejects every frame."""
    W, H = FRAME
    o = all_origins()
    for f in BAD:
        o[f] = (I32_MIN, I32_MAX) if f % 2 else (I32_MAX, I32_MIN)
    gone = np.array([(I32_MIN, I32_MAX)] * 13, np.int64)
    return [("rejected", crafted(W, H, N_ALL, bits, BAD), *WINDOW, o, 15),
            ("all rejected", crafted(W, H, 13, bits, tuple(range(13))), *WINDOW, gone, 15)]


def clamping(bits):
    W, H = FRAME
    o = np.array([(I32_MIN, 5), (I32_MAX, 5), (5, I32_MIN), (5, I32_MAX), (I32_MIN, I32_MIN), (I32_MAX, I32_MAX),
                  (-1, -1), (37, 19), (10, 10)], np.int64)
    return [("clamping", noise(W, H, 9, bits, 6), *WINDOW, o, 15)]


def masks(bits):
    return [(f"mask {m}", noise(*FRAME, N_ALL, bits, 1), *WINDOW, all_origins(), m) for m in MASKS]


def every(bits):
    return (residues_each(bits) + residues_all(bits) + windows(bits) + wide(bits) + long_row(bits) + segments(bits) +
            rejected(bits) + clamping(bits) + masks(bits))
