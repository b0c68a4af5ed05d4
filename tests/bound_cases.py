"""The cases that fill the segment projections' per-lane U32 accumulators to their 65,536-frame bound, and their
counting references (test infrastructure, like geometry_cases.py; not a test module; no GPU, no torch).

A segment workgroup of project, project_registered, project_pairs and project_lag, and a group of project_groups, sums
at most N_SEG = 65,536 frames in U32 registers: 65,536 * 255^2 and 65,536 * 65,535 lie just below 2^32.  To put 65,536
frames into one workgroup two things are needed:

  * a stream that holds only a PALETTE of four encoded frames, and an offsets array of 65,536 or 131,072 entries that
    points into it in a chosen ORDER (the kernels take any d_frame_offsets[f]); no batch of n images exists anywhere;
  * a frame one tile across and 4 * n_cu tile rows high (shape_for), whose full-frame window alone gives the plan its
    4 workgroups per compute unit, so that it cuts no segment below the bound (grouped projections take
    group_frames = 65,536 directly and need no such frame: theirs is 16 x 64, two tiles across).

The palette.  Slots 0..3 hold the frames A, F, B, F.  A and B carry payload in every tile; F is flat (depth 0) at full
scale.  Tile number q (row-major over the frame; the tile row where the frame is one tile across) of A and B holds, in
an 8 x 8 layout rolled by (3q, 5q) so that the classes sit elsewhere in every tile row:
  FF  20 pixels full scale in A and in B (and in F: full scale in every palette frame, in payload tiles and flat ones);
  HH  20 pixels high in both (>= 182 / >= 32,768: 65,536 of them total at least 2^31), different in A and B;
  F0   8 pixels full scale in A and 0 in B;   0F   8 pixels 0 in A and full scale in B;
  LL   8 pixels low in both (the lowest quarter of the pixel type at most: totals below 2^31).
The depths differ from tile to tile and between A and B: A's is 1 + q mod bits, B's 1 + (q + 3 or 7) mod bits, so at 16
bits exactly one of the two is odd (the nibble path of the half row) in every tile.  A tile of depth d < bits holds
full scale and 0 at once only because its minimum wraps: minimum = full + 1 - 2^(d-1), so the tile's values are the
2^(d-1) highest and the 2^(d-1) lowest of the pixel type (frames no encoder writes, tests/crafted.py).  Depth = bits
tiles are canonical (minimum 0).  Registered projections embed the same contents, one origin per slot, in a frame 16
pixels larger both ways whose background is noise of another depth per tile (canonical tiles); F stays full scale.

The orders (slots per frame): "const" A A A ...; "alternate" A B A B ...; "mixed" a period of 16 with seven A, seven B
and both F slots (F in one frame of eight: with more, its full-scale tiles alone would lift every pixel's total past
2^31); "halves" 65,536 times A, then mixed.  Lag 1 over "alternate" pairs (A, B) and (B, A): |b - a| is full scale at F0
and 0F in every pair.  Lag 2 over "mixed" pairs every two of A, B and F: equal full-scale partners at FF in every pair.

The counting references never touch n frames: a segment's partial is the sum over the classes of frames (slot [,
origin]) or of pairs (slot a, slot b) in it of count * that class's term, the counts from np.unique over the order.
Every value stays far below 2^63 (131,072 * 65,535^2 * 2 < 2^51), so the planes are numpy int64.
"""
import numpy as np

import crafted as cr

N_SEG = 65536                       # kProjMaxFramesPerSegment = kGProjMaxGroupFrames
FULL = {8: 255, 16: 65535}
HIGH = {8: 182, 16: 32768}          # N_SEG * 182^2 >= 2^31 > N_SEG * 181^2;  N_SEG * 32,768 = 2^31
FAMILIES = ("project", "registered", "pairs", "lag", "groups")
BITS = (8, 16)
SLOT_NAMES = ("A", "F", "B", "F")
ORIGINS = ((3, 5), (16, 16), (8, 11), (0, 0))      # the registered window's origin in slot k's frame
MARGIN = 16                                        # the registered frame is this much larger than the window
GROUPS_SHAPE = (16, 64)                            # the grouped projections' frame: 16 tiles, every depth of A and B
PAIR_OFFSETS = ((1, 0), (0, 1), (1, 1), (-1, 1))   # plane order of mask 15
LAG_SUMS = ("product", "pairsum", "absdiff", "sqdiff")
SUMS = {"project": ("sum", "sumsq"), "registered": ("sum", "sumsq"), "groups": ("sum", "sumsq"),
        "pairs": ("product",), "lag": LAG_SUMS}
EXTREMES = {"project": ("max", "min"), "registered": ("max", "min"), "groups": ("max", "min"), "pairs": (),
            "lag": ("maxdiff",)}
FOLD = {"max": np.maximum, "min": np.minimum, "maxdiff": np.maximum}

# what each kernel keeps per lane (the header comments of dbde_project_kernels.hip, dbde_pairs_kernels.hip and
# dbde_lag_kernels.hip; the grouped and registered kernels follow project's)
_SINGLE = {8: (("sum", "sumsq"), ()), 16: (("sum",), ("sumsq",))}
U32 = {(f, b): _SINGLE[b][0] for f in ("project", "registered", "groups") for b in BITS}
U64 = {(f, b): _SINGLE[b][1] for f in ("project", "registered", "groups") for b in BITS}
U32.update({("pairs", 8): ("product",), ("pairs", 16): (), ("lag", 8): LAG_SUMS, ("lag", 16): ("absdiff",)})
U64.update({("pairs", 8): (), ("pairs", 16): ("product",), ("lag", 8): (),
            ("lag", 16): ("product", "pairsum", "sqdiff")})


def bound(bits, stat):
    """The largest total N_SEG frames (pairs) can give a pixel of `stat`: the header comments' arithmetic."""
    full = FULL[bits]
    per = {"sum": full, "absdiff": full, "pairsum": 2 * full, "sumsq": full * full, "product": full * full,
           "sqdiff": full * full}[stat]
    return N_SEG * per


def near(family, bits):
    """The U32-accumulated statistics whose bound reaches 2^31 (the others, such as the 8-bit sum's 16,711,680, cannot
    tell a signed accumulator from an unsigned one at any frame count the plan allows)."""
    return tuple(s for s in U32[(family, bits)] if bound(bits, s) >= 2 ** 31)


def shape_for(n_cu):
    """The smallest frame whose full window stops the plan's cutting: one tile across, 4 * n_cu tile rows."""
    return 8, 32 * n_cu


# ---- the palette ------------------------------------------------------------------------------------------------

def depths_of(bits, q):
    """(A's, B's) depth of tile q."""
    return 1 + q % bits, 1 + (q + (3 if bits == 8 else 7)) % bits


def tile_pair(bits, q):
    """[(8 x 8 int64 values, depth, minimum)] of tile q for A and B."""
    full = FULL[bits]
    rng = np.random.default_rng([bits, q])
    out = []
    for which, d in enumerate(depths_of(bits, q)):
        half = 1 << (d - 1)
        m = 0 if d == bits else full + 1 - half
        lo, hi = max(full + 1 - half, HIGH[bits]), full - 1          # HH: high, but not full scale (none at depth 1)
        t = np.zeros((8, 8), np.int64)
        t[0:5, 0:4] = full
        t[0:5, 4:8] = rng.integers(lo, hi + 1, (5, 4)) if hi >= lo else full
        t[5, :] = full if which == 0 else 0
        t[6, :] = 0 if which == 0 else full
        t[7, :] = rng.integers(0, min(half, 1 << (bits - 2)), 8)
        out.append((np.roll(t, ((3 * q) % 8, (5 * q) % 8), (0, 1)), d, m))
    return out


def classes_of(q):
    """8 x 8 array of class names of tile q ("FF", "HH", "F0", "0F", "LL"), rolled as tile_pair rolls."""
    c = np.empty((8, 8), object)
    c[0:5, 0:4], c[0:5, 4:8], c[5, :], c[6, :], c[7, :] = "FF", "HH", "F0", "0F", "LL"
    return np.roll(c, ((3 * q) % 8, (5 * q) % 8), (0, 1))


def contents(bits, W, H):
    """{"A" | "B" | "F": (image int64 (H, W), depths (T,), minima (T,))} of a W x H frame (multiples of 8)."""
    assert W % 8 == 0 and H % 8 == 0
    ntx, nty = W // 8, H // 8
    img = {k: np.zeros((H, W), np.int64) for k in "AB"}
    dep = {k: np.zeros(ntx * nty, np.uint8) for k in "AB"}
    mins = {k: np.zeros(ntx * nty, np.int64) for k in "AB"}
    for q in range(ntx * nty):
        ty, tx = divmod(q, ntx)
        for k, (t, d, m) in zip("AB", tile_pair(bits, q)):
            img[k][8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8] = t
            dep[k][q], mins[k][q] = d, m
    T = ntx * nty
    out = {k: (img[k], dep[k], mins[k]) for k in "AB"}
    out["F"] = (np.full((H, W), FULL[bits], np.int64), np.zeros(T, np.uint8), np.full(T, FULL[bits], np.int64))
    return out


def background(bits, W, H, seed):
    """Noise of another depth per tile: tile q holds base + [0, 2^d), d = q mod (bits + 1)."""
    rng = np.random.default_rng([bits, W, H, seed])
    img = np.zeros((H, W), np.int64)
    ntx = W // 8
    for q in range(ntx * (H // 8)):
        ty, tx = divmod(q, ntx)
        d = q % (bits + 1)
        base = int(rng.integers(0, FULL[bits] + 2 - (1 << d)))
        img[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8] = base + rng.integers(0, 1 << d, (8, 8))
    return img


def encode_image(img, bits, depths=None, minima=None, index=0):
    """One frame (tests/crafted.py's layout) of an image whose sides are multiples of 8.  depths / minima (per tile,
    row-major) default to the canonical ones: the tile's minimum and the bits of its range.  Given ones may wrap:
    every pixel must be minimum + [0, 2^depth) modulo 2^bits."""
    H, W = img.shape
    assert W % 8 == 0 and H % 8 == 0
    tl = np.asarray(img, np.int64).reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3).reshape(-1, 64)
    if depths is None:
        minima = tl.min(1)
        depths = np.array([int(v).bit_length() for v in tl.max(1) - minima], np.uint8)
    rel = (tl - np.asarray(minima, np.int64)[:, None]) & FULL[bits]
    assert (rel < (1 << np.asarray(depths, np.int64))[:, None]).all(), "a pixel outside its tile's depth"
    payload = []
    for r, d in zip(rel, depths):
        if d:
            b = (r[:, None] >> np.arange(int(d))) & 1
            payload.append(np.packbits(b.astype(np.uint8).reshape(-1), bitorder="little"))
    payload = np.concatenate(payload) if payload else np.zeros(0, np.uint8)
    return cr.frame(depths, minima, payload, (2, index, 0), bits)


# ---- the orders -------------------------------------------------------------------------------------------------

ORDERS = ("const", "alternate", "mixed", "halves")
MIXED = (0, 1, 2, 0, 2, 0, 2, 0, 2, 3, 0, 2, 0, 2, 0, 2)       # A F B A B A B A  B F A B A B A B


def order(name, n, half=N_SEG):
    """The slot (0..3: A, F, B, F) of each of n frames (half: where "halves" changes, for cut-down copies)."""
    f = np.arange(n)
    if name == "const":
        return np.zeros(n, np.int64)
    if name == "alternate":
        return np.array([0, 2])[f & 1]
    if name == "mixed":
        return np.asarray(MIXED)[f % len(MIXED)]
    if name == "halves":
        return np.concatenate([np.zeros(min(n, half), np.int64), order("mixed", max(n - half, 0))])
    raise ValueError(name)


def origins_of(slots):
    """int32 (n, 2): each frame's registered origin, the one its slot's frame was built for."""
    return np.asarray(ORIGINS, np.int32)[np.asarray(slots)]


# ---- a family at one bit depth and frame shape --------------------------------------------------------------------

class Setup:
    """The palette of one family: W, H (the frame), rw, rh (the window: the full frame, but for registered), images
    (per slot, in the pixel type), frames (per slot, encoded; header index = slot), contents (per slot, int64 (rh, rw):
    what the window shows)."""

    def __init__(self, family, bits, n_cu=1, shape=None):
        assert family in FAMILIES and bits in BITS
        self.family, self.bits = family, bits
        self.rw, self.rh = shape if shape is not None else GROUPS_SHAPE if family == "groups" else shape_for(n_cu)
        pix = np.uint8 if bits == 8 else np.uint16
        con = contents(bits, self.rw, self.rh)
        self.contents = [con[k][0] for k in SLOT_NAMES]
        if family == "registered":
            self.W, self.H = self.rw + MARGIN, self.rh + MARGIN
            self.images, self.frames = [], []
            for k, (name, (ox, oy)) in enumerate(zip(SLOT_NAMES, ORIGINS)):
                im = (np.full((self.H, self.W), FULL[bits], np.int64) if name == "F" else
                      background(bits, self.W, self.H, k))
                im[oy:oy + self.rh, ox:ox + self.rw] = con[name][0]
                self.images.append(im.astype(pix))
                self.frames.append(encode_image(im, bits, index=k))
        else:
            self.W, self.H = self.rw, self.rh
            self.images = [con[k][0].astype(pix) for k in SLOT_NAMES]
            self.frames = [encode_image(con[name][0], bits, con[name][1], con[name][2], index=k)
                           for k, name in enumerate(SLOT_NAMES)]
        self._terms = {}

    def stream(self):
        """(buffer uint8, lead, per-slot offsets int64, stream bytes): the four frames back to back."""
        return cr.layout(self.frames, "concat", lead=32)

    def result_rows(self, slots):
        """int64 (n, 4): the result row of every frame (u64s 2, the slot as index, elapsed 0, the frame's bytes)."""
        rows = np.array([[2, k, 0, len(fr)] for k, fr in enumerate(self.frames)], np.int64)
        return rows[np.asarray(slots)]

    def window(self, slot, origin=None):
        """int64 (rh, rw): what the window shows of slot's frame (registered: at the origin, clamped into the frame)."""
        im = self.images[slot].astype(np.int64)
        if self.family != "registered":
            return im
        ox = min(max(int(origin[0]), 0), self.W - self.rw)
        oy = min(max(int(origin[1]), 0), self.H - self.rh)
        return im[oy:oy + self.rh, ox:ox + self.rw]

    def term(self, key):
        """One class's contribution per statistic: key = (slot,), (slot, ox, oy) or, for lag, (slot a, slot b)."""
        key = tuple(int(v) for v in key)
        if key not in self._terms:
            if self.family == "lag":
                a, b = self.window(key[0]), self.window(key[1])
                d = np.abs(b - a)
                t = dict(product=a * b, pairsum=a + b, absdiff=d, sqdiff=d * d, maxdiff=d)
            elif self.family == "pairs":
                t = dict(product=pair_products(self.window(key[0])))
            else:
                w = self.window(key[0], key[1:] or None)
                t = dict(max=w, min=w, sum=w, sumsq=w * w)
            self._terms[key] = t
        return self._terms[key]

    def keys(self, slots, lo, hi, lag=0, origins=None):
        """int64 (m, k): the class key of every frame of [lo, hi) (lag: of every pair whose later frame lies there)."""
        slots = np.asarray(slots, np.int64)
        if self.family == "lag":
            f = np.arange(max(lo, lag), max(hi, max(lo, lag)))
            return np.stack([slots[f - lag], slots[f]], 1)
        if self.family == "registered":
            org = np.asarray(origins_of(slots) if origins is None else origins, np.int64)
            return np.concatenate([slots[lo:hi, None], org[lo:hi]], 1)
        return slots[lo:hi, None]

    def empty(self):
        """The empty projection: sums 0, max 0, min all ones."""
        z = np.zeros(((4,) if self.family == "pairs" else ()) + (self.rh, self.rw), np.int64)
        out = {s: z.copy() for s in SUMS[self.family]}
        out.update({s: z + (FULL[self.bits] if s == "min" else 0) for s in EXTREMES[self.family]})
        return out

    def partial(self, keys):
        """What the frames (pairs) with these keys give: each sum as sum over classes of count * term, each extreme
        folded over the classes present; "frames": how many.  The empty projection for none."""
        out = self.empty()
        out["frames"] = len(keys)
        if len(keys):
            u, c = np.unique(keys, axis=0, return_counts=True)
            for key, cnt in zip(u, c):
                t = self.term(key)
                for s in SUMS[self.family]:
                    out[s] = out[s] + int(cnt) * t[s]
                for s in EXTREMES[self.family]:
                    out[s] = FOLD[s](out[s], t[s])
        return out

    def parts(self, slots, ranges, lag=0, origins=None):
        """The partial of every frame range (the plan's segments, or the groups)."""
        return [self.partial(self.keys(slots, lo, hi, lag, origins)) for lo, hi in ranges]

    def last_terms(self, slots, ranges, lag=0, origins=None):
        """Per range the term of its last frame (pair), None for an empty one: what mutants (c) and (d) lose or double."""
        out = []
        for lo, hi in ranges:
            k = self.keys(slots, lo, hi, lag, origins)
            out.append(self.term(k[-1]) if len(k) else None)
        return out


def pair_products(w):
    """int64 (4, rh, rw): w[y][x] * w[y + dy][x + dx] per offset of PAIR_OFFSETS, 0 where the partner is outside."""
    rh, rw = w.shape
    pad = np.zeros((rh + 1, rw + 2), np.int64)
    pad[:rh, 1:rw + 1] = w
    return np.stack([w * pad[dy:dy + rh, 1 + dx:1 + dx + rw] for dx, dy in PAIR_OFFSETS])


def segments(n, fps=N_SEG):
    """The frame ranges of the plan's segments where it cuts by the bound alone."""
    return [(lo, min(lo + fps, n)) for lo in range(0, n, fps)]


def fold(setup, parts, times=1):
    """The call's outputs from its segments' partials: sums added (times: the same call accumulated that often), extremes
    folded, "frames" added."""
    out = setup.empty()
    out["frames"] = 0
    for p in parts:
        for s in SUMS[setup.family]:
            out[s] = out[s] + times * p[s]
        for s in EXTREMES[setup.family]:
            out[s] = FOLD[s](out[s], p[s])
        out["frames"] += times * p["frames"]
    return out


def expected(setup, slots, n, lag=0, times=1, fps=N_SEG, origins=None):
    """The outputs of one call over frames [0, n) (of `times` accumulated calls): fold's dict, "count" = the accepted
    frames; for lag "pairs" too."""
    out = fold(setup, setup.parts(slots, segments(n, fps), lag, origins), times)
    frames = out.pop("frames")
    out["count"] = times * n
    if setup.family == "lag":
        out["pairs"] = frames
        assert frames == times * max(n - lag, 0)
    else:
        assert frames == times * n
    return out


def expected_groups(setup, slots, ranges, times=1):
    """Grouped planes: per statistic (n_groups, rh, rw) int64 and "counts" (n_groups,); accumulated calls add modulo the
    planes' widths (the U32 sum and counts; the U64 sumsq cannot wrap here)."""
    parts = setup.parts(slots, ranges)
    out = {s: np.stack([p[s] for p in parts]) for s in ("max", "min")}
    out["sum"] = np.stack([times * p["sum"] for p in parts]) % 2 ** 32
    out["sumsq"] = np.stack([times * p["sumsq"] for p in parts])
    out["counts"] = np.array([times * p["frames"] for p in parts], np.int64) % 2 ** 32
    return out


# ---- the cases --------------------------------------------------------------------------------------------------

def cases(family):
    """[(name, n, order, lag)]: what the GPU module runs per bit depth (each also once more with accumulate)."""
    if family == "lag":
        return [("one-lag1", N_SEG, "alternate", 1), ("one-lag2", N_SEG, "mixed", 2),
                ("two-lag1", 2 * N_SEG, "alternate", 1), ("two-lag2", 2 * N_SEG, "mixed", 2)]
    if family == "groups":
        return [("uniform", 2 * N_SEG, "halves", 0), ("ragged", N_SEG, "mixed", 0)]
    return [("one", N_SEG, "mixed", 0), ("two", 2 * N_SEG, "halves", 0)]


def ranges_of(family, case):
    """The frame ranges one workgroup accumulates in the case: the plan's segments, or the groups."""
    return segments(case[1])


def designated(family, case):
    """The sums the case is built to stress: all of a single-frame family's; for lag the differences at lag 1 over the
    alternation (full-scale differences in every pair) and product and pairsum at lag 2 over mixed (equal full-scale
    partners)."""
    if family == "lag":
        return ("absdiff", "sqdiff") if case[3] == 1 else ("product", "pairsum")
    return SUMS[family]


def fills(family, case):
    """Whether a workgroup of the case counts N_SEG frames (pairs), so that its designated U32 statistics reach bound()
    exactly.  Lag's first segment holds lag pairs less; its second segment, in the two-segment cases, holds 65,536."""
    return family != "lag" or case[1] > N_SEG


# ---- the mutants ------------------------------------------------------------------------------------------------

MUTANTS = ("a", "b", "c", "d", "e", "f")


def mutant(setup, which, parts, lasts):
    """{statistic: the call's plane under one wrong kernel}, for the statistics that mutant touches:
    (a) U32 partials sign-extended from int32;  (b) U32 partials modulo 2^31;  (c) every segment without its last frame;
    (d) every segment with its last frame twice;  (e) the U32 partials of two segments added modulo 2^32;
    (f) the U64-accumulated statistics' partials truncated to 32 bits."""
    fam, bits = setup.family, setup.bits
    out = {}
    if which in ("a", "b", "e"):
        for s in near(fam, bits):
            if which == "a":
                out[s] = sum(np.where(p[s] >= 2 ** 31, p[s] - 2 ** 32, p[s]) for p in parts)
            elif which == "b":
                out[s] = sum(p[s] % 2 ** 31 for p in parts)
            elif len(parts) > 1:
                out[s] = sum(p[s] for p in parts) % 2 ** 32
    elif which in ("c", "d"):
        sign = -1 if which == "c" else 1
        for s in SUMS[fam]:
            out[s] = sum(p[s] + (sign * t[s] if t is not None else 0) for p, t in zip(parts, lasts))
    elif which == "f":
        for s in U64[(fam, bits)]:
            out[s] = sum(p[s] % 2 ** 32 for p in parts)
    else:
        raise ValueError(which)
    return out


def tile_rows(mask):
    """bool (..., rh / 8): whether any pixel of each tile row (8 window rows) is set, per leading plane."""
    m = np.asarray(mask)
    return m.reshape(m.shape[:-2] + (m.shape[-2] // 8, 8 * m.shape[-1])).any(-1)


def tile_row_counts(mask):
    m = np.asarray(mask)
    return m.reshape(m.shape[:-2] + (m.shape[-2] // 8, 8 * m.shape[-1])).sum(-1)
