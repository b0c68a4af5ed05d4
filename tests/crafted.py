"""Crafted DBDE and DBDE16 streams: frames that follow the format's structure but that no encoder writes.

A decoder must accept whatever the reference accepts.  The reference checks four things in a frame: the tile count
T, the minima count (T, or 2T for DBDE16), every depth <= 8 (<= 16) and n64 == sum(depth).  Everything else is free:
each tile's minimum, every payload bit, and the 20-byte frame header (u64s, index and an F64 elapsed).  Encoders only
write canonical frames (min + value never wraps, elapsed is a whole number of nanoseconds); the generators here write
the rest.

Test infrastructure only, imported like oracle_ffi (not a test module).  Written from the format description alone:
  frame          := I32 u64s | U64 index | F64 elapsed | frame_data
  frame_data     := I32 T | U8 depth[T] | I32 nm | min[T] | I32 n64 | U64 payload[n64]
  8-bit:  nm = T,  U8 minima,        depth 0..8
  DBDE16: nm = 2T, U16 LE minima,    depth 0..16
Tiles are 8x8, row-major over the frame (ceil(W/8) across); edge tiles are cut at the frame's right and bottom edges.
Pixel i (row-major inside the tile, 0..63) of a depth-d tile is bits [i*d, (i+1)*d) of the tile's 8*d payload bytes,
least significant bit first, plus the tile's minimum modulo 2^8 (2^16).  Depth 0 gives the minimum.
"""
import math
import struct

import numpy as np

U64S = (0, 1, 2, 3, 0xFFFFFFFF)
MASK64 = (1 << 64) - 1


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


# elapsed fields (F64 bit patterns) no encoder writes: NaNs, infinities, negatives, fractions, subnormals, and the
# edges of the unsigned 64-bit range (2^63, 2^64 and their neighbours)
SPECIAL_ELAPSED = [
    _bits(0.0), _bits(-0.0), _bits(0.5), _bits(1.0), _bits(1.5), _bits(-0.5), _bits(-1.0), _bits(-1.5),
    0x0000000000000001, 0x800000000000000F, _bits(2.0 ** 53 + 2), _bits(2.0 ** 63 - 1024), _bits(2.0 ** 63),
    _bits(2.0 ** 63 + 2048), _bits(2.0 ** 64 - 2048), _bits(2.0 ** 64), _bits(2.0 ** 64 + 4096), _bits(1e19),
    _bits(1e300), _bits(-(2.0 ** 63)), _bits(-(2.0 ** 63) - 2048), _bits(-1e300),
    0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001,
    0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0x7FEFFFFFFFFFFFFF,
]


def f64_to_u64_x86(bits):
    """What `(uint64_t)double` gives on x86-64 as g++ compiles it (the reference's frame-header read): a truncating
    signed conversion below 2^63, else the same of v - 2^63 with bit 63 flipped; out of range and NaN give the
    'integer indefinite' 2^63 (so 2^64 and above, and +inf, give 0)."""
    v = struct.unpack("<d", struct.pack("<Q", bits & MASK64))[0]

    def cvtt(a):
        if math.isnan(a) or a >= 2.0 ** 63 or a < -(2.0 ** 63):
            return 1 << 63
        return int(a) & MASK64

    if v >= 2.0 ** 63:          # False for NaN
        return cvtt(v - 2.0 ** 63) ^ (1 << 63)
    return cvtt(v)


def tiles(W, H):
    return ((W + 7) // 8) * ((H + 7) // 8)


# ---- generators ------------------------------------------------------------------------------------------------

DEPTHS = ("random", "zero", "max", "runs256", "runs512", "odd")
MINIMA = ("random", "max", "boundary")
PAYLOADS = ("random", "ones", "zeros")


def depth_pattern(rng, kind, T, bits=8):
    """Depth bytes of T tiles: uniform in 0..max; all 0; all max (8 or 16); one depth per aligned run of 256 or 512
    tiles (the decoders' chunks); or all max except one tile of another depth per 256-tile run (its last tile)."""
    dmax = bits
    if kind == "random":
        return rng.integers(0, dmax + 1, T).astype(np.uint8)
    if kind == "zero":
        return np.zeros(T, np.uint8)
    if kind == "max":
        return np.full(T, dmax, np.uint8)
    if kind in ("runs256", "runs512"):
        run = 256 if kind == "runs256" else 512
        per = rng.integers(0, dmax + 1, (T + run - 1) // run)
        per[0::3] = dmax                   # every third run is all max: the all-max wave paths
        return np.repeat(per, run)[:T].astype(np.uint8)
    if kind == "odd":
        d = np.full(T, dmax, np.uint8)
        d[255::256] = rng.integers(0, dmax, len(d[255::256]))
        d[-1] = rng.integers(0, dmax)
        return d
    raise ValueError(kind)


def boundary_minima(bits=8):
    """Minima at the edges of the wrap: around every power of two, and max - (2^d - 1) + {-1, 0, 1} for every depth d
    (the largest minimum a depth-d tile can have without wrapping, and its neighbours)."""
    top = (1 << bits) - 1
    v = {0, 1, top - 1, top}
    for k in range(bits):
        v.update(((1 << k) - 1, 1 << k, (1 << k) + 1))
    for d in range(bits + 1):
        b = top - ((1 << d) - 1)
        v.update((b - 1, b, b + 1))
    return np.array(sorted(x for x in v if 0 <= x <= top), np.int64)


def minima_pattern(rng, kind, depths, bits=8):
    T, top = len(depths), (1 << bits) - 1
    if kind == "random":
        return rng.integers(0, top + 1, T)
    if kind == "max":
        return np.full(T, top, np.int64)
    if kind == "boundary":
        # per tile: one of its own depth's wrap edges, or one of the shared boundary values
        own = top - ((1 << depths.astype(np.int64)) - 1) + rng.integers(-1, 2, T)
        shared = rng.choice(boundary_minima(bits), T)
        return np.clip(np.where(rng.integers(0, 2, T) == 1, own, shared), 0, top)
    raise ValueError(kind)


def payload_bytes(rng, kind, n):
    if kind == "random":
        return rng.integers(0, 256, n, dtype=np.uint8)
    if kind == "ones":
        return np.full(n, 0xFF, np.uint8)
    if kind == "zeros":
        return np.zeros(n, np.uint8)
    raise ValueError(kind)


def frame_header(u64s, index, elapsed_bits):
    return np.frombuffer(struct.pack("<IQQ", u64s & 0xFFFFFFFF, index & MASK64, elapsed_bits & MASK64), np.uint8)


def random_header(rng, u64s=None):
    """A header with an arbitrary index, u64s from U64S (or as given) and an elapsed from SPECIAL_ELAPSED or random
    bits."""
    if u64s is None:
        u64s = U64S[int(rng.integers(0, len(U64S)))]
    index = int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))
    if rng.integers(0, 2):
        el = SPECIAL_ELAPSED[int(rng.integers(0, len(SPECIAL_ELAPSED)))]
    else:
        el = int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))
    return u64s, index, el


def frame(depths, minima, payload, header=(2, 0, 0), bits=8, T=None, nm=None, n64=None):
    """One frame from its parts.  T, nm and n64 default to what a valid frame holds; pass others to break one rule."""
    depths = np.asarray(depths, np.uint8)
    nt = len(depths)
    mb = 1 if bits == 8 else 2
    T = nt if T is None else T
    nm = nt * mb if nm is None else nm
    n64 = int(depths.astype(np.int64).sum()) if n64 is None else n64
    mins = np.asarray(minima, np.int64)
    mins = mins.astype(np.uint8) if mb == 1 else mins.astype("<u2").view(np.uint8)
    i32 = lambda v: np.frombuffer(struct.pack("<I", v & 0xFFFFFFFF), np.uint8)   # noqa: E731
    return np.concatenate([frame_header(*header), i32(T), depths, i32(nm), mins, i32(n64),
                           np.asarray(payload, np.uint8)])


def craft(rng, W, H, bits=8, depth="random", minima="random", payload="random", header=None):
    """A valid-structure frame of a W x H image with the chosen patterns; header random unless given."""
    T = tiles(W, H)
    d = depth_pattern(rng, depth, T, bits)
    m = minima_pattern(rng, minima, d, bits)
    p = payload_bytes(rng, payload, 8 * int(d.astype(np.int64).sum()))
    return frame(d, m, p, random_header(rng) if header is None else header, bits)


def all_pairs_frame(rng, payload, perm=None, T=None, header=(2, 0, 0), bits=8):
    """A frame whose tiles hold every (depth, minimum) pair.  8-bit: depth 0..8 x minimum 0..255, exactly once in 2304
    tiles (384 x 384); DBDE16: depth 0..16 x boundary_minima(16).  In `perm` order ("random": a random one), cycled to
    fill T tiles."""
    mins = np.arange(256) if bits == 8 else boundary_minima(16)
    d = np.repeat(np.arange(bits + 1), len(mins))
    m = np.tile(mins, bits + 1)
    if perm is not None:
        perm = rng.permutation(len(d)) if isinstance(perm, str) else perm
        d, m = d[perm], m[perm]
    if T is not None:
        d, m = np.resize(d, T), np.resize(m, T)
    return frame(d.astype(np.uint8), m, payload_bytes(rng, payload, 8 * int(d.sum())), header, bits)


# ---- breaking one rule ------------------------------------------------------------------------------------------

BREAKS = ("depth", "nm+1", "nm-1", "n64+1", "n64-1", "T+1", "T-1")


def break_rule(fr, how, bits=8, tile=None):
    """A copy of frame `fr` with exactly one validity rule broken, at its edge: a depth one above the maximum (at
    `tile`, default the last; n64 and the payload grow with it, so that n64 == sum(depth) still holds and only the
    depth check can reject the frame), the minima count or n64 one off, or the first tile count one off."""
    g = fr.copy()
    T = int(g[20:24].view("<u4")[0])
    mb = 1 if bits == 8 else 2
    at_nm, at_n64 = 24 + T, 28 + T + mb * T

    def add(at, k):
        g[at:at + 4] = np.frombuffer(struct.pack("<I", (int(g[at:at + 4].view("<u4")[0]) + k) & 0xFFFFFFFF), np.uint8)

    if how == "depth":
        at = 24 + (T - 1 if tile is None else tile)
        grow = bits + 1 - int(g[at])
        g[at] = bits + 1
        add(at_n64, grow)
        g = np.concatenate([g, np.full(8 * grow, 0xA5, np.uint8)])
    elif how in ("nm+1", "nm-1"):
        add(at_nm, 1 if how == "nm+1" else -1)
    elif how in ("n64+1", "n64-1"):
        add(at_n64, 1 if how == "n64+1" else -1)
    elif how in ("T+1", "T-1"):
        add(20, 1 if how == "T+1" else -1)
    else:
        raise ValueError(how)
    return g


# ---- numpy decoder ----------------------------------------------------------------------------------------------

def parse_header(fr):
    """(u64s, index, elapsed_ns) as the reference reads them: u64s is 0xFFFFFFFF unless 2."""
    u64s, index, el = struct.unpack("<IQQ", np.asarray(fr[:20], np.uint8).tobytes())
    return (2 if u64s == 2 else 0xFFFFFFFF), index, f64_to_u64_x86(el)


def broken_rules(data, W, H, bits=8):
    """The validity rules frame_data breaks for a W x H frame: a subset of {"T", "nm", "depth", "n64"}."""
    data = np.asarray(data, np.uint8)
    T, mb = tiles(W, H), (1 if bits == 8 else 2)
    u32 = lambda at: int(data[at:at + 4].view("<u4")[0]) if at + 4 <= len(data) else None   # noqa: E731
    depths = data[4:4 + T].astype(np.int64)
    out = set()
    if u32(0) != T:
        out.add("T")
    if u32(4 + T) != mb * T:
        out.add("nm")
    if (depths > bits).any():
        out.add("depth")
    if u32(8 + T + mb * T) != int(depths.sum()):
        out.add("n64")
    return out


def decode_image(data, W, H, bits=8):
    """frame_data -> (bytes consumed, (H, W) image) or (0, None) when it does not validate."""
    data = np.asarray(data, np.uint8)
    T, mb = tiles(W, H), (1 if bits == 8 else 2)
    if broken_rules(data, W, H, bits):
        return 0, None
    depths = data[4:4 + T].astype(np.int64)
    mins = data[8 + T: 8 + T + mb * T]
    mins = (mins.astype(np.int64) if mb == 1 else mins.view("<u2").astype(np.int64))
    start = 12 + T + mb * T
    end = start + 8 * int(depths.sum())
    if end > len(data):
        return 0, None
    pay = data[start:end]
    offs = 8 * np.concatenate([[0], np.cumsum(depths)[:-1]])
    px = np.zeros((T, 64), np.int64)
    for d in range(1, bits + 1):
        sel = np.nonzero(depths == d)[0]
        if len(sel) == 0:
            continue
        raw = pay[offs[sel][:, None] + np.arange(8 * d)]                          # (k, 8d) bytes
        b = np.unpackbits(raw, axis=1, bitorder="little").reshape(len(sel), 64, d).astype(np.int64)
        px[sel] = b @ (np.int64(1) << np.arange(d, dtype=np.int64))
    px = (px + mins[:, None]) & ((1 << bits) - 1)
    w, h = (W + 7) // 8, (H + 7) // 8
    img = px.reshape(h, w, 8, 8).transpose(0, 2, 1, 3).reshape(8 * h, 8 * w)[:H, :W]
    return end, np.ascontiguousarray(img.astype(np.uint8 if bits == 8 else np.uint16))


def decode_frame(fr, W, H, bits=8):
    """-> (bytes advanced, header as the reference reads it, image or None): a frame that does not validate advances
    20 bytes and reports u64s 0xFFFFFFFF."""
    u64s, index, el = parse_header(fr)
    n, img = decode_image(np.asarray(fr)[20:], W, H, bits)
    if n == 0:
        return 20, (0xFFFFFFFF, index, el), None
    return 20 + n, (u64s, index, el), img


# ---- placing frames in a stream ---------------------------------------------------------------------------------

def payload_start(fr):
    T = int(fr[20:24].view("<u4")[0])
    nm = int(fr[24 + T:28 + T].view("<u4")[0])
    return 32 + T + nm


def layout(frames, how="concat", lead=32, slot=0, junk=0xA5):
    """Places frames in one stream buffer.  how = "concat": back to back; "slots": frame k at k * slot; "residues":
    frame k at the first position after frame k-1 where its payload starts at residue k mod 16 (of the buffer's
    address, which torch allocates 256-byte aligned); "offsets": frame k starts at residue k mod 16.
    -> (buffer uint8, lead, offsets int64 relative to lead, stream bytes from lead to the end of the last frame).
    Junk lies between frames and for 64 bytes behind the last."""
    offs, at = [], 0
    for k, fr in enumerate(frames):
        if how == "slots":
            at = k * slot
            assert len(fr) <= slot
        elif how in ("residues", "offsets"):
            want = (k % 16 - (payload_start(fr) if how == "residues" else 0)) % 16
            at += (want - (lead + at)) % 16
        offs.append(at)
        at += len(fr)
    total = at
    buf = np.full(lead + total + 64, junk, np.uint8)
    for o, fr in zip(offs, frames):
        buf[lead + o: lead + o + len(fr)] = fr
    return buf, lead, np.array(offs, np.int64), total
