"""Crafted images for the encoders: families of frames whose depth and minimum arrays are known by construction.

Test infrastructure only, imported like crafted.py (not a test module).  NumPy only, deterministic, no GPU, no oracle.

The synthetic contents of oracle/synth.c put a tile's extremes at fixed pixels, realise only the top of each depth's
range and never look at what lies behind a partial tile.  The families here put them everywhere else:

  lone_extreme(high)  one valid pixel per tile differs from a flat background by delta; its position walks through
                      the tile's valid positions, delta through both ends of every depth
  range_ladder        tile minimum m, maximum m + r, r through every range; extremes at two walking positions
  padding_trap        partial tiles whose valid part is nearly flat while everything an unclamped load could fetch
                      instead (the next image row, the next frame, the guard bytes) is far away
  depth_runs(run)     depth patterns for prefix sums and per-chunk accounting (empty chunks beside full ones)
  bit_patterns(d)     all ones but one zero, checkerboards, a walking one bit, at depth d over a walking minimum

A family is a function (W, H, frame, bits) -> (image (H, W) uint8 / uint16, depth[T] uint8, minimum[T] int64); depth
and minimum are what the construction realises, tile by tile, row-major -- computed from the parameters the image was
built from, never from the image.  bits is 8 or 16; top = 2^bits - 1.

pack_numpy(image, bits) is an encoder written from the format description alone (the module docstring of crafted.py,
whose decode_image is its inverse): tiles row-major, clamp-to-edge padding, depth = bit_length(max - min), values
packed least significant bit first.
"""
import struct

import numpy as np

GUARD = 60                      # the byte around a padding_trap batch (60 -> 0x3C3C = 15420 as a 16-bit pixel)
TRAP_LEVELS = (10, 120, 230)    # x 256 for 16-bit pixels
P_TILE, P_DELTA = 29, 7         # strides of the walks over the tile number (29 is coprime to every count of valid pixels)


def top_of(bits):
    return (1 << bits) - 1


def dtype_of(bits):
    return np.uint8 if bits == 8 else np.uint16


def bit_length(x):
    """Element-wise bit length of a non-negative integer array (0 for 0)."""
    x = np.asarray(x, np.int64)
    n = np.zeros(x.shape, np.int64)
    for k in range(17):
        n += (x >> k) > 0
    return n


class Grid:
    """The tiles of a W x H frame: w x h of them, row-major; vc / vr: valid columns / rows of each (8, or the margin)."""

    def __init__(self, W, H):
        self.W, self.H = W, H
        self.w, self.h = (W + 7) // 8, (H + 7) // 8
        self.T = self.w * self.h
        t = np.arange(self.T)
        self.t, self.ty, self.tx = t, t // self.w, t % self.w
        self.vc = np.minimum(8, W - 8 * self.tx)
        self.vr = np.minimum(8, H - 8 * self.ty)
        self.nvalid = self.vc * self.vr
        self.rm, self.dm = W - 8 * (self.w - 1), H - 8 * (self.h - 1)      # 1..8
        # tile classes: 0 interior, 1 right edge, 2 bottom edge, 3 corner (edge = a partial tile's side)
        right = (self.tx == self.w - 1) & (self.rm < 8)
        bottom = (self.ty == self.h - 1) & (self.dm < 8)
        self.cls = right.astype(np.int64) + 2 * bottom.astype(np.int64)

    def spread(self, per_tile):
        """A per-tile array as an (H, W) image (every pixel holds its tile's value)."""
        a = np.asarray(per_tile).reshape(self.h, self.w)
        return np.repeat(np.repeat(a, 8, 0), 8, 1)[:self.H, :self.W]

    def pixel(self, pos):
        """(y, x) in the image of each tile's valid position number pos[t] (row-major over its vr x vc valid pixels)."""
        return 8 * self.ty + pos // self.vc, 8 * self.tx + pos % self.vc

    def in_tile(self):
        """(r, c): each pixel's row and column inside its tile, as (H, W) arrays."""
        y, x = np.mgrid[0:self.H, 0:self.W]
        return y & 7, x & 7


def per_tile_kind(g, kind, fn):
    """fn(valid rows, valid columns, kind) -> (lo, hi), evaluated once per distinct triple, as two per-tile arrays."""
    key = (g.vr * 16 + g.vc) * 256 + np.asarray(kind, np.int64)
    lo, hi = np.zeros(g.T, np.int64), np.zeros(g.T, np.int64)
    for k in np.unique(key):
        lo[key == k], hi[key == k] = fn(int(k) >> 12, (int(k) >> 8) & 15, int(k) & 255)
    return lo, hi


CLASSES = ("interior", "right edge", "bottom edge", "corner")


def deltas(bits):
    """1, 2, 3, 4, 7, 8, ..., 2^(bits-1) - 1, 2^(bits-1), top: the smallest and the largest range of every depth."""
    out = [1]
    for d in range(2, bits + 1):
        out += [1 << (d - 1), (1 << d) - 1]
    return out


def ladder_ranges(bits):
    """Every range 0..255; 16-bit: 0..300, then 2^k - 1, 2^k, 2^k + 1 up to 65535."""
    if bits == 8:
        return list(range(256))
    out = set(range(301))
    for k in range(8, 17):
        out.update(v for v in ((1 << k) - 1, 1 << k, (1 << k) + 1) if v <= 65535)
    return sorted(out)


def walk_minimum(u, r, bits):
    """A minimum for range r that cycles through 0, top - r and a value in between with the counter u."""
    hi = top_of(bits) - np.asarray(r, np.int64)
    u = np.asarray(u, np.int64)
    mid = (hi * ((u * 37) % 101 + 1)) // 103
    return np.where(u % 3 == 0, 0, np.where(u % 3 == 1, hi, mid))


# ---- lone_extreme ------------------------------------------------------------------------------------------------

def lone_position(g, f):
    """Valid position number of each tile's lone pixel in frame f."""
    return (P_TILE * g.t + f) % g.nvalid


def lone_delta_index(g, f, bits):
    return (P_DELTA * g.t + f) % len(deltas(bits))


def lone_extreme(high):
    """Every tile one background value and exactly one valid pixel delta above it (high) or below it.  A tile with a
    single valid pixel is that pixel: depth 0."""
    def family(W, H, f, bits):
        g, top = Grid(W, H), top_of(bits)
        delta = np.array(deltas(bits), np.int64)[lone_delta_index(g, f, bits)]
        u = g.t + 3 * f
        low = walk_minimum(u, delta, bits)              # the smaller of the tile's two values
        bg, px = (low, low + delta) if high else (low + delta, low)
        img = g.spread(bg).copy()
        y, x = g.pixel(lone_position(g, f))
        img[y, x] = px
        single = g.nvalid == 1
        depth = np.where(single, 0, bit_length(delta))
        minimum = np.where(single, px, low)
        assert img.max() <= top and img.min() >= 0
        return img.astype(dtype_of(bits)), depth.astype(np.uint8), minimum
    family.__name__ = "lone_high" if high else "lone_low"
    return family


# ---- tiles of a given range (range_ladder, depth_runs) ---------------------------------------------------------------

def extreme_positions(g, f):
    """Valid position numbers of each tile's minimum and maximum in frame f: distinct wherever a tile has two pixels."""
    pmin = (P_TILE * g.t + f) % g.nvalid
    step = 1 + (g.t + 5 * f) % np.maximum(g.nvalid - 1, 1)
    return pmin, (pmin + step) % g.nvalid


def ranged_image(g, f, bits, r, m, seed):
    """Tile t: minimum m[t] and maximum m[t] + r[t] at the walking positions, seeded random values between them
    elsewhere.  Tiles with one valid pixel hold m[t] (range 0).  -> (image, depth, minimum)."""
    r = np.where(g.nvalid == 1, 0, np.asarray(r, np.int64))
    m = np.asarray(m, np.int64)
    rng = np.random.default_rng([seed, g.W, g.H, f, bits])
    img = g.spread(m) + rng.integers(0, g.spread(r) + 1)
    pmin, pmax = extreme_positions(g, f)
    y, x = g.pixel(pmax)
    img[y, x] = m + r
    y, x = g.pixel(pmin)
    img[y, x] = np.where(g.nvalid == 1, m + r, m)
    return img.astype(dtype_of(bits)), bit_length(r).astype(np.uint8), m


def range_ladder(W, H, f, bits):
    """The k-th tile of frame f that has two valid pixels or more has range ranges[(f K + k) mod len(ranges)], K such
    tiles per frame (a single-pixel tile can only be flat and takes no turn)."""
    g = Grid(W, H)
    ranges = np.array(ladder_ranges(bits), np.int64)
    many = g.nvalid > 1
    u = f * int(many.sum()) + np.cumsum(many) - 1
    r = np.where(many, ranges[u % len(ranges)], 0)
    return ranged_image(g, f, bits, r, walk_minimum(u // len(ranges) + u, r, bits), 0x1ADDE2)


def ladder_frames(W, H, bits):
    """Frames of range_ladder after which every range has had its turn."""
    return -(-len(ladder_ranges(bits)) // max(int((Grid(W, H).nvalid > 1).sum()), 1))


RUN_KINDS = ("last", "first", "runs", "stairs", "ones", "odd")


def run_pattern(kind, T, run, bits):
    """The depth pattern of depth_runs: all 0 but the last tile / but the first; runs of `run` tiles of depth 0
    alternating with runs of the largest depth; t mod (bits + 1); all 1; all odd depths."""
    t = np.arange(T)
    if kind == "last":
        return np.where(t == T - 1, bits, 0)
    if kind == "first":
        return np.where(t == 0, bits, 0)
    if kind == "runs":
        return np.where((t // run) % 2 == 1, bits, 0)
    if kind == "stairs":
        return t % (bits + 1)
    if kind == "ones":
        return np.ones(T, np.int64)
    if kind == "odd":
        return 1 + 2 * (t % (bits // 2))
    raise ValueError(kind)


def depth_runs(run, kind=None):
    """Frames whose depth array is run_pattern(kind) (kind None: RUN_KINDS[frame mod 6]), content random at exactly
    that depth, both extremes present.  `runs` starts with an empty and with a full run in turn: its odd frames
    (kind None: every other of its turns) hold the complement.  A tile with a single valid pixel has depth 0 whatever
    the pattern."""
    def family(W, H, f, bits):
        g = Grid(W, H)
        k = kind or RUN_KINDS[f % len(RUN_KINDS)]
        d = run_pattern(k, g.T, run, bits)
        if k == "runs" and (f // (len(RUN_KINDS) if kind is None else 1)) % 2 == 1:
            d = bits - d
        rng = np.random.default_rng([0xDE97, W, H, f, bits, run])
        lo = np.where(d > 0, 1 << np.maximum(d - 1, 0), 0)
        hi = (1 << d) - 1
        r = np.where(rng.integers(0, 3, g.T) == 0, hi, rng.integers(lo, hi + 1))       # a third of the tiles: the top
        r = np.where(g.nvalid == 1, 0, r)
        return ranged_image(g, f, bits, r, walk_minimum(g.t + f, r, bits), 0xDE98)
    family.__name__ = f"depth_runs({run}{', ' + kind if kind else ''})"
    return family


# ---- bit_patterns ----------------------------------------------------------------------------------------------------

BIT_KINDS = ("one_zero", "checker0", "checker1", "walking_bit")


def bit_patterns(d=None):
    """Depth d (None: tile t of frame f takes depth 1 + (t // 4 + f) mod bits).  Tile t of frame f takes
    BIT_KINDS[(t + f) mod 4] as its min-subtracted values: all 2^d - 1 but one 0 at a walking position; the two
    checkerboards of 0 and 2^d - 1; pixel i of the tile (row-major in the 8 x 8) holds 1 << (i mod d).  The base walks
    through 0 and top - (2^d - 1)."""
    def family(W, H, f, bits):
        g = Grid(W, H)
        dd = np.full(g.T, d, np.int64) if d else 1 + (g.t // 4 + f) % bits
        full = (np.int64(1) << dd) - 1
        kind = (g.t + f) % 4
        base = walk_minimum(g.t // 4 + f, full, bits)
        r_in, c_in = g.in_tile()
        K, F, D = g.spread(kind), g.spread(full), g.spread(dd)
        checker = ((r_in + c_in) & 1) * F
        walking = np.int64(1) << ((8 * r_in + c_in) % D)
        v = np.where(K == 1, checker, np.where(K == 2, F - checker, np.where(K == 3, walking, F)))
        y, x = g.pixel(lone_position(g, f))
        zero_at = np.zeros((H, W), bool)
        zero_at[y, x] = True
        v = np.where((K == 0) & zero_at, 0, v)
        img = g.spread(base) + v

        # what each tile realises, from its kind, its depth and its count of valid rows and columns alone
        def realised(vr, vc, k):
            k, depth = k & 3, k >> 2
            top_v = (1 << depth) - 1
            if k == 0:
                return (0, top_v) if vr * vc > 1 else (0, 0)
            if k in (1, 2):
                first = 0 if k == 1 else top_v
                return (0, top_v) if vr * vc > 1 else (first, first)
            e = {(8 * r + c) % depth for r in range(vr) for c in range(vc)}
            return 1 << min(e), 1 << max(e)
        lo, hi = per_tile_kind(g, kind + 4 * dd, realised)
        return img.astype(dtype_of(bits)), bit_length(hi - lo).astype(np.uint8), base + lo
    family.__name__ = f"bit_patterns({d or ''})"
    return family


# ---- padding_trap ----------------------------------------------------------------------------------------------------

def trap_levels(bits):
    return tuple(v * (1 if bits == 8 else 256) for v in TRAP_LEVELS)


def padding_trap(W, H, f, bits):
    """pixel = level + ((x + 2 y + f) & 3).  Frames wider than one tile: partial tiles' column and row of tiles at the
    low level in even frames and the high one in odd frames, all other tiles at the middle level.  Frames one tile
    wide: level[(f h + ty) mod 3] per tile row (an unclamped row runs on into the tile's own next rows there, so only
    the next tile row can differ).  Meant to lie in one allocation with GUARD bytes in front and behind
    (trap_batch)."""
    g = Grid(W, H)
    L = trap_levels(bits)
    if g.w > 1:
        edge = ((g.tx == g.w - 1) & (g.rm < 8)) | ((g.ty == g.h - 1) & (g.dm < 8))
        level = np.where(edge, L[0] if f % 2 == 0 else L[2], L[1])
    else:
        level = np.array(L, np.int64)[(f * g.h + g.ty) % 3]
    y, x = np.mgrid[0:H, 0:W]
    img = g.spread(level) + ((x + 2 * y + f) & 3)
    # a tile starts at multiples of 8: (x + 2 y) & 3 inside it is (c + 2 r) & 3 of the tile's own row r and column c
    def realised(vr, vc, k):
        e = {(c + 2 * r + f) & 3 for r in range(vr) for c in range(vc)}
        return min(e), max(e)
    lo, hi = per_tile_kind(g, np.zeros(g.T, np.int64), realised)
    return img.astype(dtype_of(bits)), bit_length(hi - lo).astype(np.uint8), level + lo


def trap_batch(W, H, n, bits, first=0, lead=4096, tail=None):
    """n padding_trap frames as the GPU test lays them out: one buffer of GUARD bytes, the frames back to back from
    byte `lead`, at least 8 image rows + 8 pixels of GUARD bytes behind them.
    -> (buffer uint8, lead, [(image, depth, minimum)] per frame)."""
    px = bits // 8
    tail = (8 * W + 16) * px + 64 if tail is None else tail
    frames = [padding_trap(W, H, first + k, bits) for k in range(n)]
    buf = np.full(lead + n * W * H * px + tail, GUARD, np.uint8)
    body = np.stack([fr[0] for fr in frames])
    buf[lead: lead + body.nbytes] = body.reshape(-1).view(np.uint8)
    return buf, lead, frames


# ---- the families of a case ------------------------------------------------------------------------------------------

def families(runs=(64,)):
    """The families a batch is drawn from (padding_trap aside: its batches keep their own layout): the run pattern at
    every given run length, every other depth pattern once."""
    return ([lone_extreme(True), lone_extreme(False), range_ladder, bit_patterns()]
            + [depth_runs(r, "runs") for r in runs] + [depth_runs(runs[0], k) for k in RUN_KINDS if k != "runs"])


def draw(k, fams, first=0):
    """The k-th frame of a mixed batch: families in turn, so that neighbouring frames in memory differ, each with its
    own frame counter.  -> (family, frame number)."""
    return fams[k % len(fams)], first + k // len(fams)


def mixed_batch(W, H, n, bits, runs=(64,), first=0, skip=0):
    """Frames skip .. skip + n - 1 of the mixed sequence -> (images (n, H, W), [(family name, frame number, depth,
    minimum)])."""
    fams = families(runs)
    imgs, info = [], []
    for k in range(skip, skip + n):
        fam, f = draw(k, fams, first)
        img, d, m = fam(W, H, f, bits)
        imgs.append(img)
        info.append((fam.__name__, f, d, m))
    return np.stack(imgs), info


# ---- the encoder, from the format alone --------------------------------------------------------------------------------

def tile_pixels(image, bits=8):
    """(T, 64) int64: every tile of the image as a dense 8 x 8, clamp-to-edge padded (each row's last valid pixel
    repeated to the right, then the last row repeated downwards)."""
    H, W = image.shape
    w, h = (W + 7) // 8, (H + 7) // 8
    ys = np.minimum(np.arange(8 * h), H - 1)
    xs = np.minimum(np.arange(8 * w), W - 1)
    full = np.asarray(image, np.int64)[np.ix_(ys, xs)]
    return full.reshape(h, 8, w, 8).transpose(0, 2, 1, 3).reshape(w * h, 64)


def pack_tiles(px, bits=8):
    """(depth[T], minimum[T], payload bytes) of dense tiles px (T, 64)."""
    lo, hi = px.min(1), px.max(1)
    depth = bit_length(hi - lo)
    v = px - lo[:, None]
    # tiles in order; a tile of depth d is 64 values of d bits each, least significant bit first: 8 d bytes
    order = np.argsort(depth, kind="stable")
    out = [None] * len(px)
    for d in range(1, bits + 1):
        sel = order[depth[order] == d]
        if len(sel) == 0:
            continue
        b = ((v[sel][:, :, None] >> np.arange(d)) & 1).astype(np.uint8).reshape(len(sel), 64 * d)
        packed = np.packbits(b, axis=1, bitorder="little")
        for k, t in enumerate(sel):
            out[t] = packed[k]
    parts = [p for p in out if p is not None]
    payload = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
    return depth.astype(np.uint8), lo, payload


def pack_numpy(image, bits=8):
    """frame_data of the image: I32 T | U8 depth[T] | I32 nm | min[T] (U8, or U16 LE with nm = 2 T) | I32 n64 |
    payload.  Without the 20-byte frame header (frame_numpy adds it)."""
    depth, lo, payload = pack_tiles(tile_pixels(image, bits), bits)
    T = len(depth)
    mins = lo.astype(np.uint8) if bits == 8 else lo.astype("<u2").view(np.uint8)
    i32 = lambda v: np.frombuffer(struct.pack("<I", v), np.uint8)   # noqa: E731
    return np.concatenate([i32(T), depth, i32(len(mins)), mins, i32(int(depth.astype(np.int64).sum())), payload])


def frame_numpy(index, image, bits=8):
    """The frame an encoder writes: header {u64s 2, index, elapsed 0.0} and frame_data."""
    return np.concatenate([np.frombuffer(struct.pack("<IQQ", 2, index, 0), np.uint8), pack_numpy(image, bits)])


def frame_arrays(frame, W, H, bits=8):
    """(depth[T], minimum[T] int64, payload offset of every tile, payload bytes) of a frame with its 20-byte header."""
    T = ((W + 7) // 8) * ((H + 7) // 8)
    mb = bits // 8
    fr = np.asarray(frame, np.uint8)
    depth = fr[24:24 + T]
    mins = fr[28 + T: 28 + T + mb * T]
    mins = mins.astype(np.int64) if mb == 1 else np.ascontiguousarray(mins).view("<u2").astype(np.int64)
    offs = 8 * np.concatenate([[0], np.cumsum(depth.astype(np.int64))[:-1]])
    return depth, mins, offs, fr[32 + T + mb * T:]


def first_difference(got, want, W, H, bits=8):
    """Where two frames of a W x H image first differ, for a test's message: the first tile whose depth, minimum or
    payload differs, its valid columns and rows, and which of the three it is; or the header field."""
    got, want = np.asarray(got, np.uint8), np.asarray(want, np.uint8)
    if got[:20].tobytes() != want[:20].tobytes():
        return "frame header differs"
    g = Grid(W, H)
    dg, mg, og, pg = frame_arrays(got, W, H, bits)
    dw, mw, ow, pw = frame_arrays(want, W, H, bits)
    for what, a, b in (("depth", dg, dw), ("minimum", mg, mw)):
        if len(a) == len(b) and not np.array_equal(a, b):
            t = int(np.nonzero(a != b)[0][0])
            return (f"first differing tile {t} (tile row {t // g.w}, column {t % g.w}; rm {int(g.vc[t])}, dm "
                    f"{int(g.vr[t])}): {what} {int(a[t])} != {int(b[t])}")
    for t in range(g.T):
        a, b = pg[og[t]: og[t] + 8 * int(dg[t])], pw[ow[t]: ow[t] + 8 * int(dw[t])]
        if a.tobytes() != b.tobytes():
            return (f"first differing tile {t} (tile row {t // g.w}, column {t % g.w}; rm {int(g.vc[t])}, dm "
                    f"{int(g.vr[t])}): payload differs (depth {int(dw[t])}, minimum {int(mw[t])})")
    if len(got) != len(want):
        return f"sizes differ: {len(got)} != {len(want)}"
    return "the I32 fields differ" if got.tobytes() != want.tobytes() else "equal"
