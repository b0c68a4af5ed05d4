"""The compressed-domain crop as a splice of packed tiles, in numpy (test infrastructure, like binned_ref.py).

crop_frame(frame, W, H, x, y, rw, rh, bits) is the model of dbde_hip_crop_frames for one frame: a window tile whose
valid margins equal its source tile's is COPIED (depth byte, minimum, payload bytes as stored); any other tile is
decoded (wrapping add), its valid pixels are clamp-to-edge padded (dbde_pack_8x8_partial's padding) and packed again.
Both halves come from the format alone: crafted.decode_image's tile decode and crafted_images.pack_tiles (the numpy
encoder that test_encode_crafted pins to the oracle).  tests/test_crop_ref.py pins this file to the oracles.
crop_batch adds the rejected-frame and per-frame-origin rules and both output layouts.
"""
import struct

import numpy as np

import crafted
import crafted_images as ci


def tiles_of(n):
    return (n + 7) // 8


def margins(n, t0, nt, extent):
    """Valid pixels of each of nt window tiles from tile t0 on (window extent `extent`), and of their source tiles
    (image extent n)."""
    i = np.arange(nt)
    return np.minimum(8, extent - 8 * i), np.minimum(8, n - 8 * (t0 + i))


def clamp_origin(W, H, rw, rh, x, y):
    """Per-frame origin rule: clamped into [0, W-rw] x [0, H-rh], then rounded down to a multiple of 8."""
    x = min(max(int(x), 0), W - rw)
    y = min(max(int(y), 0), H - rh)
    return x & ~7, y & ~7


def decode_tiles(depth, mins, offs, pay, sel, bits):
    """(len(sel), 64) int64 pixels of the selected tiles (the wrapping add included)."""
    px = np.zeros((len(sel), 64), np.int64)
    for k, t in enumerate(sel):
        d = int(depth[t])
        if d:
            raw = pay[offs[t]: offs[t] + 8 * d]
            b = np.unpackbits(raw, bitorder="little").reshape(64, d).astype(np.int64)
            px[k] = b @ (np.int64(1) << np.arange(d, dtype=np.int64))
    return (px + np.asarray(mins)[sel][:, None]) & ((1 << bits) - 1)


def pad_tile(px, rm, dm):
    """64 pixels with columns from rm on repeating column rm-1 and rows from dm on repeating row dm-1."""
    t = px.reshape(8, 8)
    return t[np.ix_(np.minimum(np.arange(8), dm - 1), np.minimum(np.arange(8), rm - 1))].reshape(64)


def crop_frame(frame, W, H, x, y, rw, rh, bits=8, stats=None):
    """The cropped frame (20-byte header kept) of a VALID frame; x, y multiples of 8.  stats: optional dict that
    receives the counts of tiles copied and re-packed."""
    assert x % 8 == 0 and y % 8 == 0 and 0 <= x <= W - rw and 0 <= y <= H - rh and rw >= 1 and rh >= 1
    fr = np.asarray(frame, np.uint8)
    w = tiles_of(W)
    tx, ty, ntx, nty = x // 8, y // 8, tiles_of(rw), tiles_of(rh)
    depth, mins, offs, pay = ci.frame_arrays(fr, W, H, bits)
    rm, srm = margins(W, tx, ntx, rw)
    dm, sdm = margins(H, ty, nty, rh)
    out_d, out_m, out_p = [], [], []
    copied = recoded = 0
    for j in range(nty):
        for i in range(ntx):
            t = (ty + j) * w + tx + i
            if rm[i] == srm[i] and dm[j] == sdm[j]:
                out_d.append(int(depth[t]))
                out_m.append(int(mins[t]))
                out_p.append(pay[offs[t]: offs[t] + 8 * int(depth[t])])
                copied += 1
            else:
                px = pad_tile(decode_tiles(depth, mins, offs, pay, [t], bits)[0], int(rm[i]), int(dm[j]))
                d, lo, p = ci.pack_tiles(px[None, :], bits)
                out_d.append(int(d[0]))
                out_m.append(int(lo[0]))
                out_p.append(p)
                recoded += 1
    if stats is not None:
        stats["copied"] = stats.get("copied", 0) + copied
        stats["recoded"] = stats.get("recoded", 0) + recoded
    payload = np.concatenate(out_p) if out_p else np.zeros(0, np.uint8)
    T2 = ntx * nty
    mb = bits // 8
    m = np.array(out_m, np.int64)
    m = m.astype(np.uint8) if mb == 1 else m.astype("<u2").view(np.uint8)
    i32 = lambda v: np.frombuffer(struct.pack("<I", v), np.uint8)   # noqa: E731
    return np.concatenate([fr[:20], i32(T2), np.array(out_d, np.uint8), i32(mb * T2), m, i32(sum(out_d)), payload])


def frame_valid(frame, W, H, bits=8):
    fr = np.asarray(frame, np.uint8)
    T, mb = crafted.tiles(W, H), bits // 8
    if len(fr) < 32 + T + mb * T or crafted.broken_rules(fr[20:], W, H, bits):
        return False
    n64 = int(fr[28 + T + mb * T: 32 + T + mb * T].view("<u4")[0])
    return len(fr) >= 32 + T + mb * T + 8 * n64


def frame_length(frame, W, H, bits=8):
    fr = np.asarray(frame, np.uint8)
    T, mb = crafted.tiles(W, H), bits // 8
    return 32 + T + mb * T + 8 * int(fr[24:24 + T].astype(np.int64).sum())


def max_frame_bytes(W, H, bits=8):
    return 32 + (66 if bits == 8 else 131) * crafted.tiles(W, H)


def crop_batch(frames, W, H, x, y, rw, rh, bits=8, origins=None, slot_stride=0):
    """-> (cropped frames, None for a rejected one; offsets; bytes; origins used) as dbde_hip_crop_frames reports them:
    a rejected frame has 0 bytes and, concatenated, the offset the next accepted frame takes."""
    outs, offs, nbytes, used = [], [], [], []
    at = 0
    for f, fr in enumerate(frames):
        ox, oy = (x, y) if origins is None else clamp_origin(W, H, rw, rh, *origins[f])
        used.append((ox, oy))
        out = crop_frame(fr[:frame_length(fr, W, H, bits)], W, H, ox, oy, rw, rh, bits) if frame_valid(fr, W, H, bits) else None
        outs.append(out)
        offs.append(f * slot_stride if slot_stride else at)
        nbytes.append(0 if out is None else len(out))
        at += nbytes[-1]
    return outs, np.array(offs, np.int64), np.array(nbytes, np.int64), np.array(used, np.int32).reshape(-1, 2)


def windows(W, H):
    """Windows of a W x H frame that end on a tile boundary, inside a tile and on the frame's own (partial) edge, from
    the frame's corner and from inside it; the whole frame among them."""
    out = [(0, 0, W, H)]
    for x, y in ((0, 0), (8 * (W // 24), 8 * (H // 24))):
        for rw in {min(8, W - x), 8 * ((W - x) // 16), (W - x) // 2 + 1, W - x - 1, W - x}:
            for rh in {8 * ((H - y) // 16), (H - y + 2) // 3, H - y}:
                if rw >= 1 and rh >= 1:
                    out.append((x, y, rw, rh))
    return sorted(set(out))
