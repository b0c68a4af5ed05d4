"""Frames and images at byte offsets past 2^31 and 2^32, laid out so that an offset bug gives wrong values, not a fault.

Test infrastructure only, imported like crafted.py (not a test module).

The layout invariant
--------------------
Every device buffer a far test hands to a kernel is one allocation:

    | lead: L sentinel bytes | the region the kernel is given (pointer P) ... last byte in use | tail: >= 2^26 |

with L a multiple of 256, L >= 2^31 + 2^26 for byte-addressed buffers (streams, U8 images) and L >= 2^33 for U16
image batches, and every offset in use below 2^33.

Take an offset X in [0, 2^33) that a kernel wrongly narrows to 32 bits.  Its unsigned alias X mod 2^32 lies in
[0, 2^32): at or behind P and before P + X, inside the region.  Its signed alias (the same bits sign-extended) lies in
[-2^31, 2^31): at least P - 2^31, which the lead covers with 2^26 bytes to spare for whatever the kernel then reads
from there (a frame of 4096 x 3072 is 13 MB).  A U16 element index E that goes negative lands 2 * 2^31 = 2^32 bytes in
front of P, inside a lead of 2^33.  An unsigned element index wraps to an element in front of E.  The tail covers a
read or write that runs on past the last byte in use.  So a truncation or sign extension anywhere in a kernel moves
its accesses inside the test's own allocation, and the test sees wrong values or a written lead instead of a fault.

Decoys
------
A stream read that loses the high half of a far frame's offset would mostly land on sentinel bytes and reject the
frame.  That fails the test, but a truncated read should fail it loudly and for the right reason.  So every frame
with bytes at or past 2^31 gets a decoy at X - 2^32, where each of those bytes lands under both aliases (the frames
here stay below 2^32 + 2^31, where the two aliases agree): a different valid frame of the same geometry, with other
pixels and another index.  A kernel that truncates decodes that frame and reports its numbers.  Decoys of frames in
[2^31, 2^32) lie in the lead, the others in the near part of the region, which holds no real frame.

Placements (placements())
-------------------------
one frame ending just below 2^31; one whose header is below 2^31 and whose depth bytes are above it; one at an odd
offset past 2^31; one across 2^32 (its depth array, minima array or payload holds byte 2^32, one kind per stream, as
frames cannot overlap); one at an odd offset past 2^32; and the last, ending at stream_bytes.  Consumers take any
offsets, so the same placements repeat to make n as large as a kernel form needs.
"""
import numpy as np

G31, G32, G33 = 1 << 31, 1 << 32, 1 << 33
MARGIN = 1 << 26
LEAD8 = G31 + MARGIN            # byte-addressed buffers: streams, U8 images
LEAD16 = G33                    # U16 image batches
SENTINEL = 0xA5
STRADDLES = ("depth", "minima", "payload")
SLOTS = ("below_2^31", "header_2^31", "odd_past_2^31", "across_2^32", "odd_past_2^32", "last")


def aliases(x):
    """The addresses offset x turns into when it loses its high half: unsigned and signed 32-bit views, other than x."""
    u = x & 0xFFFFFFFF
    s = u - G32 if u >= G31 else u
    return sorted({u, s} - {x})


def parts(fr):
    """Byte ranges of a frame's fields: dict name -> (start, end), relative to the frame."""
    fr = np.asarray(fr, np.uint8)
    u32 = lambda at: int(fr[at:at + 4].view("<u4")[0]) if at + 4 <= len(fr) else 0   # noqa: E731
    T = u32(20)
    nm = u32(24 + T)
    n64 = u32(28 + T + nm)
    out = dict(header=(0, 20), T=(20, 24), depth=(24, 24 + T), nm=(24 + T, 28 + T), minima=(28 + T, 28 + T + nm),
               n64=(28 + T + nm, 32 + T + nm), payload=(32 + T + nm, 32 + T + nm + 8 * n64))
    return {k: (min(a, len(fr)), min(b, len(fr))) for k, (a, b) in out.items()}


def _round(x, m):
    return (x + m - 1) // m * m


def placements(frames, straddle, step=None):
    """Offsets of the six SLOTS for frames[0..5] (packed frames, numpy uint8).  frames[3] crosses 2^32 with the field
    `straddle` ("depth", "minima" or "payload"; the byte at 2^32 is the field's middle one).  step: the distance kept
    between frames past 2^31 (and so between their decoys), at least the largest frame or decoy."""
    assert len(frames) == len(SLOTS) and straddle in STRADDLES
    sizes = [len(f) for f in frames]
    step = step or _round(max(sizes) + 4096, 1 << 20)
    a, b = parts(frames[3])[straddle]
    assert b > a, f"frame 3 has no {straddle} bytes"
    x1 = G31 - 23                                   # header [2^31 - 23, 2^31 - 3), depth from 2^31 + 1
    x0 = x1 - 40 - sizes[0]                         # ends 40 bytes below frame 1, just below 2^31
    x2 = _round(x1 + sizes[1], 1 << 20) + step + 0x1235   # odd, past 2^31
    x3 = G32 - a - (b - a) // 2
    x4 = _round(x3 + sizes[3], 1 << 20) + step + 0x2469 + 2   # odd, past 2^32
    x5 = _round(x4 + sizes[4], 1 << 20) + step + 0x10 + 3
    return [x0, x1, x2, x3, x4, x5]


class Layout:
    """Where frames and decoys go in a far stream: host arithmetic only (tests/test_far_layout.py pins it).
    offsets[k], frames[k]: the real frames; decoys: list of (offset, decoy frame, k) for frames with bytes >= 2^31;
    stream_bytes: the end of the last frame; size: the allocation, lead + stream_bytes + the tail."""

    def __init__(self, frames, offsets, decoys, lead=LEAD8):
        assert lead % 256 == 0 and lead >= LEAD8
        self.frames, self.offsets, self.lead = list(frames), [int(x) for x in offsets], lead
        self.decoys = []
        d = 0
        for k, (x, fr) in enumerate(zip(self.offsets, self.frames)):
            if x + len(fr) > G31:
                self.decoys.append((x - G32, decoys[d % len(decoys)], k))
                d += 1
        self.stream_bytes = max(x + len(f) for x, f in zip(self.offsets, self.frames))
        self.size = _round(lead + self.stream_bytes + MARGIN, 256)

    def spans(self):
        """(start, end, what) of every frame and decoy, relative to P."""
        out = [(x, x + len(f), f"frame {k}") for k, (x, f) in enumerate(zip(self.offsets, self.frames))]
        return out + [(x, x + len(f), f"decoy of {k}") for x, f, k in self.decoys]

    def check(self):
        """The invariant of the module docstring, for this layout; raises AssertionError."""
        assert self.offsets[-1] + len(self.frames[-1]) == self.stream_bytes, "the last frame ends the stream"
        sp = sorted(self.spans())
        for (a0, a1, wa), (b0, b1, wb) in zip(sp, sp[1:]):
            assert a1 <= b0, f"{wa} [{a0}, {a1}) overlaps {wb} [{b0}, {b1})"
        for s0, s1, w in sp:
            assert -self.lead <= s0 and s1 + MARGIN <= self.size - self.lead, f"{w} leaves the allocation or its tail"
        real = set(self.offsets)
        decoy_at = {x: k for x, _, k in self.decoys}
        for k, (x, fr) in enumerate(zip(self.offsets, self.frames)):
            assert 0 <= x and x + len(fr) < G33
            assert (x + len(fr) > G31) == (x - G32 in decoy_at), f"frame {k}: decoy where bytes pass 2^31"
            for alias in aliases(x):
                assert -self.lead + MARGIN <= alias and alias + len(fr) + MARGIN <= self.size - self.lead, \
                    f"frame {k}: alias {alias} leaves the allocation"
                assert alias not in real, f"frame {k}: alias {alias} is a real frame"
                assert decoy_at.get(alias) == k, f"frame {k}: alias {alias} is not its decoy"
        for x, dec, k in self.decoys:
            assert not np.array_equal(dec, self.frames[k]), f"decoy of frame {k} is the frame"
            assert bytes(dec[4:20]) != bytes(self.frames[k][4:20]), f"decoy of frame {k} has its index"


def straddles(lay):
    """{k: [fields of frame k that hold byte 2^31 or 2^32, as 'field@2^31' / 'field@2^32']}."""
    out = {}
    for k, (x, fr) in enumerate(zip(lay.offsets, lay.frames)):
        for name, (a, b) in parts(fr).items():
            for g, tag in ((G31, "2^31"), (G32, "2^32")):
                if x + a <= g < x + b:
                    out.setdefault(k, []).append(f"{name}@{tag}")
    return out


# ---- the frames the far tests place ------------------------------------------------------------------------------

SYNTH_SEED = 0xFA2_2016


def frame_set(W, H, bits=8, oracle=None, pack16=None):
    """(good, bad, decoys) for a W x H geometry, the same on every call: good, valid frames (8-bit: the oracle's frames
    of synthetic mixed and noise8 images; DBDE16: pack16 of mixed and full-range images; then crafted frames: every
    (depth, minimum) pair with an all-ones payload, whose minima wrap, and depth / minima / payload patterns); bad,
    each rule of crafted.BREAKS broken once; decoys, valid random frames that none of the others equals."""
    import crafted as cr
    rng = np.random.default_rng(W * 7919 + H * 104729 + bits)
    T = cr.tiles(W, H)
    good = []
    if bits == 8:
        for k, mode in enumerate((1, 0)):                  # mixed, noise8
            img = oracle.synth_frame(mode, SYNTH_SEED, k, W, H)
            good.append(oracle.pack_frame(int(rng.integers(1 << 40, 1 << 62)), img, W, H))
    else:
        full = rng.integers(0, 65536, (H, W)).astype(np.uint16)
        mixed = (rng.integers(0, 65536, (H, W)) >> rng.integers(0, 17, (H, W))).astype(np.uint16)
        good += [pack16(mixed, int(rng.integers(1 << 40, 1 << 62))), pack16(full, int(rng.integers(1 << 40, 1 << 62)))]
    perm = None if (bits == 8 and T == 2304) else "random"
    good.append(cr.all_pairs_frame(rng, "ones", perm, T, header=cr.random_header(rng, 2), bits=bits))
    for d, m, p in (("max", "boundary", "ones"), ("runs256", "boundary", "random"), ("odd", "max", "random")):
        good.append(cr.craft(rng, W, H, bits, d, m, p, header=cr.random_header(rng, 2)))
    bad = [cr.break_rule(good[2 + k % 4], how, bits, tile=min(T, 256) - 1) for k, how in enumerate(cr.BREAKS)]
    for fr in bad:
        fr[:20] = cr.frame_header(*cr.random_header(rng))
    decoys = [cr.craft(rng, W, H, bits, d, "random", "random", header=cr.random_header(rng, 2))
              for d in ("random", "max")]
    return good, bad, decoys


def slot_frames(good, bad, straddle):
    """The six frames of the SLOTS for one straddle kind: valid frames at the 2^31 and 2^32 straddles and at the end,
    frames that break one rule at the odd offsets past 2^31 and past 2^32."""
    v = STRADDLES.index(straddle)
    return [good[v % len(good)], good[(v + 1) % len(good)], bad[2 * v], good[(v + 2) % len(good)],
            bad[2 * v + 1], good[(v + 3) % len(good)]]


def far_layout(good, bad, decoys, straddle, lead=LEAD8):
    frames = slot_frames(good, bad, straddle)
    step = _round(max(len(f) for f in frames + list(decoys)) + 4096, 1 << 20)
    return Layout(frames, placements(frames, straddle, step), decoys, lead)


def far_stream(layout, entries=None, device="cuda"):
    """The layout on the device (FarStream); entries: the slot each of the n offsets reads (repeats allowed)."""
    return FarStream(layout, entries, device)


def entries(n):
    """n offsets that cycle through the six slots."""
    return np.resize(np.arange(len(SLOTS)), n)


# ---- device side -------------------------------------------------------------------------------------------------

class FarStream:
    """A Layout on the device.  buf: the allocation; lead: the stream_offset the API takes (P = buf + lead);
    offs: int64 device offsets of the n entries; slot[f]: which frame entry f reads."""

    def __init__(self, lay, entries=None, device="cuda"):
        import torch
        self.lay, self.lead, self.stream_bytes = lay, lay.lead, lay.stream_bytes
        self.slot = np.arange(len(lay.frames)) if entries is None else np.asarray(entries)
        self.buf = torch.full((lay.size,), SENTINEL, dtype=torch.uint8, device=device)
        for x, fr in [(x, f) for x, f in zip(lay.offsets, lay.frames)] + [(x, f) for x, f, _ in lay.decoys]:
            self.buf[lay.lead + x: lay.lead + x + len(fr)] = torch.from_numpy(np.ascontiguousarray(fr)).to(device)
        self.offs = torch.tensor([lay.offsets[k] for k in self.slot], dtype=torch.int64, device=device)
        self.n = len(self.slot)


class NearStream:
    """The same frames in the same order at small offsets with the same residues mod 256: the control that a far
    call must equal element for element."""

    def __init__(self, lay, entries=None, device="cuda"):
        import torch
        at, offs = 64, []
        for x, fr in zip(lay.offsets, lay.frames):
            at += (x - at) % 256
            offs.append(at)
            at += len(fr)
        self.lead, self.stream_bytes = 256, at
        self.slot = np.arange(len(lay.frames)) if entries is None else np.asarray(entries)
        host = np.full(256 + at + 256, SENTINEL, np.uint8)
        for o, fr in zip(offs, lay.frames):
            host[256 + o: 256 + o + len(fr)] = fr
        self.buf = torch.from_numpy(host).to(device)
        self.offs = torch.tensor([offs[k] for k in self.slot], dtype=torch.int64, device=device)
        self.n = len(self.slot)


class Guarded:
    """A tensor of `shape` and `dtype` at byte `lead` of a sentinel-filled allocation with a tail of MARGIN bytes.
    .t: the tensor (all sentinel bytes at first); .check(): the lead and the tail are still all sentinel."""

    def __init__(self, shape, dtype, lead=None, device="cuda", fill=SENTINEL):
        import torch
        item = torch.empty((), dtype=dtype).element_size()
        lead = (LEAD8 if item == 1 else LEAD16) if lead is None else lead
        assert lead % 256 == 0 and lead >= (LEAD8 if item == 1 else LEAD16)
        self.nbytes = int(np.prod(shape)) * item
        assert self.nbytes < G33
        self.lead, self.fill = lead, fill
        self.buf = torch.full((_round(lead + self.nbytes + MARGIN, 256),), fill, dtype=torch.uint8, device=device)
        self.t = self.buf[lead: lead + self.nbytes].view(dtype).view(shape)

    def check(self, what=""):
        b = self.buf
        assert all_equal(b[:self.lead], self.fill), f"{what}: wrote into the lead in front of the output"
        assert all_equal(b[self.lead + self.nbytes:], self.fill), f"{what}: wrote into the tail behind the output"


def all_equal(t, value, chunk=1 << 30):
    """Every element of the 1-d device tensor t equals value; compared a GiB at a time (a lead of 2^33 bytes would
    otherwise take a comparison mask of the same size)."""
    return all(bool((t[i:i + chunk] == value).all()) for i in range(0, t.numel(), chunk))


def guarded(shape, dtype, lead=None, device="cuda"):
    return Guarded(shape, dtype, lead, device)


def free():
    import gc
    import torch
    gc.collect()
    torch.cuda.empty_cache()


# the geometries the GPU far tests place (tests/test_far_layout.py checks the layout of each)
GEOMETRIES8 = [(8, 8), (72, 72), (150, 150), (180, 180), (200, 123), (384, 384), (1024, 768), (720, 1280),
               (1080, 1920), (1366, 768), (2200, 1000), (4096, 3072)]
GEOMETRIES16 = [(200, 123), (1024, 768), (4096, 3072)]
