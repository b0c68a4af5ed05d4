"""The geometry matrix: four small frames that land in each regime of roi_index_geometry's hard spot, with the windows,
origins and patches every stream-reading family is run at (test infrastructure, imported like crafted.py; not a test
module).  tests/test_geometry_cases.py judges all of it on the CPU before any GPU run; tests/test_gpu_geometry.py runs
every family x pixel size x geometry.

Every kernel that reads a window of a compressed frame has its own copy of the same front half: the index chunk of its
first tile (dec_chunk_of / dec_chunk_begin on roi_index_geometry) and the sum of the npre = pos0 - chunk_begin < 512
depth bytes in front of it.  roi_index_geometry has three regimes -- A: at most 512 tiles across, one chunk per tile row;
B: wider, 512-tile pieces of a row; C: plain 512-tile chunks that do not start at tile rows -- and the geometries are
the smallest frames that reach each regime where a copy can go wrong:

  row512   4096 x 17      512 x 3 tiles      A at its widest: npre up to 511, the last tile row 1 px high
  row513   4104 x 17      513 x 3 tiles      B at its smallest: the second piece of every row holds one tile
  row1025  8200 x 33      1025 x 5 tiles     B with three pieces; 15 chunks per frame, so few frames take the split index
  plain    24 x 262147    3 x 32769 tiles    C; 512 mod 3 != 0, so 128 of the 192 chunk boundaries fall inside a tile row
                                             (the first: tile 512 = row 170, column 2); the last tile row 3 px high

Streams: N frames per (geometry, pixel size), each crafted with random depths, boundary minima and random payloads (so
every tile differs from its neighbours), frame BAD broken by one rule (the depth of the frame's last tile one above the
maximum), placed with crafted.layout's "residues".  pool() gives them as a sequences.Pool with the rows and images of
crafted.decode_frame, built once per process.
"""
import numpy as np

import crafted as cr

N = 5
BAD = 2
RULE = "depth"
GEOMETRIES = {"row512": (4096, 17), "row513": (4104, 17), "row1025": (8200, 33), "plain": (24, 262147)}
NAMES = tuple(GEOMETRIES)
BITS = (8, 16)
REGIME = {"row512": "A", "row513": "B", "row1025": "B", "plain": "C"}
# what every family's plan function reports of the index at n = 3 (index_split: None = whatever index_split_for gives,
# which the CPU test restates)
PLAN = {"row512": dict(chunks_per_frame=3, chunk_tiles=512, chunk_pieces=1),
        "row513": dict(chunks_per_frame=6, chunk_tiles=512, chunk_pieces=2),
        "row1025": dict(chunks_per_frame=15, chunk_tiles=512, chunk_pieces=3),
        "plain": dict(chunks_per_frame=193, chunk_tiles=512, chunk_pieces=0, index_split=49)}

DEEP = 17066                     # a tile row of `plain` that chunk boundary 100 cuts (tile 51200 = row 17066, column 2)
WINDOWS = {
    "row512": ((4035, 0, 61, 17),            # tile_x 504: a prefix of at least 504 depth bytes
               (2051, 5, 300, 9),
               (0, 0, 4096, 17)),
    "row513": ((4097, 3, 7, 14),             # wholly in the last piece
               (4080, 3, 24, 14),            # across the seam
               (0, 0, 4104, 17)),
    "row1025": ((4097, 3, 7, 14),            # wholly in the second piece
                (8193, 3, 7, 14),            # wholly in the last piece
                (6001, 2, 300, 20),          # starts 238 tiles inside the second piece: a prefix behind a seam
                (4080, 3, 24, 14),           # across the first seam
                (4090, 1, 4110, 30),         # across both seams
                (0, 0, 8200, 33)),
    "plain": ((0, 1355, 24, 21),             # tile rows 169..171, around the first straddled row
              (3, DEEP * 8 - 3, 19, 14),     # around a deep straddled row
              (17, 262144, 7, 3),            # the cut bottom-right tile, tile row 32768
              (0, 262136, 24, 11)),
}

# per-frame origins (x, y) of a window RW x RH that moves across the seam / the straddled row from frame to frame
# (families with per-frame origins: decode_roi, decode_scaled, decode_mask, crop_frames, registered projections)
MOVING = {
    "row512": ((61, 9), ((4035, 0), (3000, 8), (4030, 3), (2051, 5), (4027, 8))),
    "row513": ((7, 12), ((4089, 0), (4092, 2), (4097, 5), (4090, 3), (4096, 1))),
    "row1025": ((20, 14), ((4080, 0), (8180, 19), (4070, 10), (4096, 3), (8176, 7))),
    "plain": ((19, 14), ((3, 1357), (0, 1360), (5, DEEP * 8 - 3), (2, DEEP * 8), (5, 262133))),
}

# origins of the patch families' patches (sequences.PATCH = 24 x 16, six per frame), the same in every frame: over the
# right edge, over the seams, on the straddled rows, and the last over the bottom edge (inside the frame in clamp mode
# after the clamp, hanging over it in fill mode)
PATCHES = {
    "row512": ((4080, 0), (4085, 1), (4030, -3), (2040, 1), (-5, 0), (4060, 9)),
    "row513": ((4090, 0), (4085, 1), (4080, -3), (4097, 1), (-5, 0), (4088, 9)),
    "row1025": ((4085, 3), (8180, 9), (8190, 17), (4096, 0), (-5, 20), (8183, 25)),
    "plain": ((0, 1355), (3, 1361), (-2, DEEP * 8 - 5), (0, DEEP * 8), (5, 0), (4, 262139)),
}
# the search patches of match_patches, by (tw, th, S): origins of the SEARCH patch (tw + 2S x th + 2S), four per frame,
# at the same places; the larger search patch (49 x 47) is higher than three of the frames and wider than the fourth, so
# it runs in fill mode
MATCH = ((16, 12, 2), (33, 31, 8))
SEARCH = {
    "row512": {2: ((4076, 0), (4030, 1), (2047, 0), (4070, 5)), 8: ((4060, -8), (4025, -20), (2047, -15), (-9, 3))},
    "row513": {2: ((4084, 0), (4090, 1), (4078, 0), (4080, 5)), 8: ((4070, -8), (4090, -20), (4050, -15), (4096, 3))},
    "row1025": {2: ((4084, 3), (8180, 13), (8176, 0), (4090, 20)), 8: ((4070, -8), (8170, -3), (8160, 0), (4096, 10))},
    "plain": {2: ((0, 1355), (4, 1359), (2, DEEP * 8 - 5), (3, 262135)),
              8: ((-12, 1340), (-3, DEEP * 8 - 20), (-20, 262120), (5, 1352))},
}


def seed_of(name, bits):
    return NAMES.index(name) * 100 + bits + 20250


# ---- roi_index_geometry, restated (csrc/dbde_roi_kernels.h; dec_chunk_of / dec_chunk_begin of dbde_kernels.h) -----------

def index_geometry(W, H):
    """-> dict(w, h, T, ct, pieces, cpf, regime)."""
    w, h = (W + 7) // 8, (H + 7) // 8
    pieces = (w + 511) // 512
    if h * pieces <= 32768:
        return dict(w=w, h=h, T=w * h, ct=w if pieces == 1 else 512, pieces=pieces, cpf=h * pieces,
                    regime="A" if pieces == 1 else "B")
    return dict(w=w, h=h, T=w * h, ct=512, pieces=1, cpf=(w * h + 511) // 512, regime="C")


def chunk_of(g, pos):
    if g["pieces"] == 1:
        return pos // g["ct"]
    ty, tx = divmod(pos, g["w"])
    return ty * g["pieces"] + tx // 512


def chunk_begin(g, c):
    if g["pieces"] == 1:
        return min(c * g["ct"], g["T"])
    ty, pc = divmod(c, g["pieces"])
    return ty * g["w"] + pc * 512


def window_rows(W, H, win):
    """What the front half of a window kernel meets at each of the window's tile rows: [(tile row, first tile pos0, its
    chunk, npre = pos0 - chunk_begin, the piece of the row the chunk is, the chunks of the row's window tiles)]."""
    g = index_geometry(W, H)
    x, y, rw, rh = win
    tx0, tx1 = x // 8, (x + rw - 1) // 8
    out = []
    for ty in range(y // 8, (y + rh - 1) // 8 + 1):
        pos0 = ty * g["w"] + tx0
        c = chunk_of(g, pos0)
        piece = c % g["pieces"] if g["regime"] == "B" else 0
        out.append((ty, pos0, c, pos0 - chunk_begin(g, c), piece,
                    sorted({chunk_of(g, ty * g["w"] + tx) for tx in range(tx0, tx1 + 1)})))
    return out


# ---- the streams ------------------------------------------------------------------------------------------------------

_HOST, _POOLS = {}, {}


def host_frames(name, bits):
    """(frames, rows, images) of a geometry's stream: rows as the decoders report them, images None where rejected."""
    key = (name, bits)
    if key not in _HOST:
        W, H = GEOMETRIES[name]
        rng = np.random.default_rng(seed_of(name, bits))
        frames, rows, images = [], [], []
        for f in range(N):
            fr = cr.craft(rng, W, H, bits, "random", "boundary", "random")
            if f == BAD:
                fr = cr.break_rule(fr, RULE, bits)
            adv, head, img = cr.decode_frame(fr, W, H, bits)
            frames.append(fr)
            rows.append((head[0], head[1], head[2], adv))
            images.append(img)
        _HOST[key] = (frames, rows, images)
    return _HOST[key]


def pool(name, bits):
    """The stream as a sequences.Pool (host arrays; dev() uploads them once), one per (geometry, pixel size) and process."""
    import sequences as sq
    key = (name, bits)
    if key not in _POOLS:
        W, H = GEOMETRIES[name]
        frames, rows, images = host_frames(name, bits)
        _POOLS[key] = sq.Pool.of_frames(f"{name}_{bits}", bits, W, H, frames, rows, images, "residues")
    return _POOLS[key]


def stream(name, bits):
    """The same device stream as a wproject_gpu.Stream (what counts_gpu, pairs_gpu and lag_gpu check on)."""
    import wproject_gpu as wg
    p = pool(name, bits)
    buf, offs = p.dev()
    return wg.Stream(buf, p.lead, p.total, offs, p.W, p.H, p.images)


# ---- what the families that need more than a window are given ---------------------------------------------------------

def aligned(win):
    """The window with its origin rounded down to a multiple of 8 (crop_frames and decode_binned require one): the same
    tiles, so the same prefix and the same chunks."""
    x, y, rw, rh = win
    return x & ~7, y & ~7, rw + (x & 7), rh + (y & 7)


def patch_origins(name):
    """(N, 6, 2): PATCHES in every frame, rotated by the frame number so that every patch slot meets every place."""
    base = list(PATCHES[name])
    return tuple(tuple(base[(k + f) % len(base)] for k in range(len(base))) for f in range(N))


def search_origins(name, S):
    base = list(SEARCH[name][S])
    return np.array([[base[(k + f) % len(base)] for k in range(len(base))] for f in range(N)], np.int64)


def templates(name, bits, tw, th):
    """One random template per search patch."""
    rng = np.random.default_rng(seed_of(name, bits) + tw)
    return rng.integers(0, 1 << bits, (4, th, tw)).astype(np.uint8 if bits == 8 else np.uint16)


def match_mode(name, tw, th, S):
    """patch_ref.CLAMP where the search patch fits the frame, else patch_ref.FILL."""
    import patch_ref as pr
    W, H = GEOMETRIES[name]
    return pr.CLAMP if tw + 2 * S <= W and th + 2 * S <= H else pr.FILL


def displaced(name, win):
    """The window 8 px left, right, up and down, where that stays inside the frame."""
    W, H = GEOMETRIES[name]
    x, y, rw, rh = win
    return [(x + dx, y + dy, rw, rh) for dx, dy in ((-8, 0), (8, 0), (0, -8), (0, 8))
            if 0 <= x + dx and x + dx + rw <= W and 0 <= y + dy and y + dy + rh <= H]
