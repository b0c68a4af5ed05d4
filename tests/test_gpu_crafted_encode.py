"""GPU: every encoder form of tests/test_encode_forms.ENCODE_CASES on the crafted images of tests/crafted_images.py.

The other encoder tests feed the kernels four synthetic contents whose tile extremes sit at fixed pixels and whose
edge tiles have nothing behind them that could be told from the padding.  Here every row of the coverage table -- each
(kernel, input mode, right margin) the planner offers, each bottom margin per kernel -- encodes two batches:

  * frames drawn in turn from lone_extreme (both polarities), range_ladder, bit_patterns and depth_runs (runs of the
    case's own chunk size, one tile less and one more), so that neighbouring frames in memory differ;
  * padding_trap frames in their own layout: guard bytes around the batch, and behind every partial tile pixels that
    change its depth if a load is not clamped.

Images and output each lie in a sentinel-filled allocation.  Checked: the form with the real device addresses; offsets
and sizes; the whole output allocation byte for byte against the oracle's frames laid out on the host (frames, gaps,
lead and tail at once); every frame's depth and minimum arrays against the arrays known BY CONSTRUCTION (the check that
does not pass through the oracle); the images untouched; decode_frames of the GPU's bytes returns the images.
Integer work: no tolerance anywhere.  A mismatch names the case, the family, the frame, the first differing tile, its
margins and whether depth, minimum or payload differs.
"""
import struct

import numpy as np
import pytest

import crafted_images as ci
from test_encode_forms import ENCODE_CASES, FORM_KEYS, case_id, slot_stride

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
APRON = 1 << 17          # sentinel bytes in front of and behind a buffer: more than 8 image rows of the widest case
DISTINCT = 24            # distinct frames of a batch (two of every family); larger batches repeat them in order
DEVICE = "cuda"          # (a host rehearsal of the checks, with the oracle standing in for the encoder, sets "cpu")
TRAP_PERIOD = 12         # padding_trap repeats after 12 frames (parity 2, level 3, pattern 4)
FIRST_INDEX = (1 << 32) - 3


@pytest.fixture(scope="module")
def dv():
    import dbde_video_cpp_amd as m
    m.build()
    return m


@pytest.fixture(scope="module")
def codec(dv):
    c = dv.Codec(0)
    assert c.arch.startswith("gfx950")
    yield c
    c.close()


class Guarded:
    """nbytes at byte APRON + residue of an allocation filled with `fill`, APRON bytes or more behind them."""

    def __init__(self, nbytes, residue=0, fill=SENTINEL):
        import torch
        self.lead, self.nbytes, self.fill = APRON + residue, nbytes, fill
        self.buf = torch.full(((self.lead + nbytes + APRON + 255) // 256 * 256,), fill, dtype=torch.uint8, device=DEVICE)
        assert DEVICE != "cuda" or self.buf.data_ptr() % 256 == 0

    def host(self):
        return np.full(self.buf.numel(), self.fill, np.uint8)


def runs_of(plan, T):
    """depth_runs' run lengths for a case: the chunk size, one tile less and one more; the whole-frame kernels
    (chunk_tiles 0): a wave of tiles and the frame."""
    ct = plan["chunk_tiles"]
    return (ct, ct - 1, ct + 1) if ct else (64, T)


def mixed_frames(W, H, n, bits, runs):
    """The mixed batches of a case, each (distinct frames, their (family, frame, depth, minimum), the distinct frame
    each of the n batch entries holds).  One batch, or as many as it takes to give every family a frame when n is
    smaller than the number of families."""
    distinct = max(DISTINCT, min(10 * DISTINCT, (1 << 21) // (W * H)))       # small frames: up to twenty of every family
    fams = len(ci.families(runs))
    out = []
    for first in range(0, fams if n < fams else 1, n):
        imgs, info = ci.mixed_batch(W, H, min(n, distinct), bits, runs, skip=first)
        out.append((imgs, info, np.arange(n) % len(imgs)))
    return out


def trap_frames(W, H, n, bits):
    k = min(n, TRAP_PERIOD)
    frames = [ci.padding_trap(W, H, f, bits) for f in range(k)]
    return [(np.stack([f[0] for f in frames]), [("padding_trap", f, fr[1], fr[2]) for f, fr in enumerate(frames)], np.arange(n) % k)]


def expected_stream(bodies, which, first_index, stride, host, lead):
    """Lays the frames out in `host` from byte `lead` as the encoder must: entry k holds header {2, first_index + k,
    0.0} and bodies[which[k]], at k * stride or back to back.  -> (offsets, sizes)."""
    n = len(which)
    sizes = np.array([20 + len(bodies[w]) for w in which], np.int64)
    offs = np.arange(n, dtype=np.int64) * stride if stride else np.concatenate([[0], np.cumsum(sizes)[:-1]])
    if stride:
        view = host[lead: lead + n * stride].reshape(n, stride) if lead + n * stride <= len(host) else None
    else:
        view = None
    idx = (first_index + np.arange(n, dtype=np.uint64)).astype("<u8")
    if view is not None:
        for d, body in enumerate(bodies):
            rows = np.nonzero(which == d)[0]
            view[rows, 20:20 + len(body)] = body
        view[:, 0:4] = np.frombuffer(struct.pack("<I", 2), np.uint8)
        view[:, 4:12] = idx.view(np.uint8).reshape(n, 8)
        view[:, 12:20] = 0
    else:
        for k in range(n):
            at = lead + int(offs[k])
            host[at: at + 4] = (2, 0, 0, 0)
            host[at + 4: at + 12] = idx[k: k + 1].view(np.uint8)
            host[at + 12: at + 20] = 0
            host[at + 20: at + int(sizes[k])] = bodies[which[k]]
    return offs, sizes


def explain(got, want, lead, offs, sizes, info, which, W, H, bits, what):
    """The message of a byte mismatch: which frame, family and tile -- or which bytes outside the frames."""
    for k in range(len(which)):
        a = lead + int(offs[k])
        g, w = got[a: a + int(sizes[k])], want[a: a + int(sizes[k])]
        if g.tobytes() != w.tobytes():
            name, f, _, _ = info[which[k]]
            return (f"{what}: entry {k} ({name}, frame {f}) differs from the oracle: "
                    + ci.first_difference(g, w, W, H, bits))
    at = int(np.nonzero(got != want)[0][0])
    return f"{what}: byte {at - lead} relative to the output (outside every frame) was written: {got[at]:#x}"


def run_batch(codec, what, W, H, bits, imgs, info, which, residue, out_residue, stride, pack_body, guard_fill,
              encode, decode):
    """One encode of the batch and every check of the module docstring.  encode(images tensor, out buffer, out lead,
    capacity) -> (offsets, sizes); decode(out buffer, out lead, total, offsets) -> images tensor."""
    import torch
    n, px = len(which), bits // 8
    T = ((W + 7) // 8) * ((H + 7) // 8)
    maxf = 32 + (66 if bits == 8 else 131) * T
    cap = (n - 1) * stride + maxf if stride else n * maxf
    # the images, inside their guard
    gi = Guarded(n * W * H * px, residue, guard_fill)
    host_i = gi.host()
    host_i[gi.lead: gi.lead + gi.nbytes] = imgs[which].reshape(-1).view(np.uint8)
    gi.buf.copy_(torch.from_numpy(host_i))
    t = gi.buf[gi.lead: gi.lead + gi.nbytes]
    images = t.view(torch.int16).view(n, H, W) if bits == 16 else t.view(n, H, W)
    before = gi.buf.clone()
    go = Guarded(cap, out_residue)
    offs, sizes = encode(images, go.buf, go.lead, cap)
    codec.sync()
    # what the oracle says the whole allocation holds
    bodies = [pack_body(img) for img in imgs]
    want = go.host()
    want_offs, want_sizes = expected_stream(bodies, which, FIRST_INDEX, stride, want, go.lead)
    o, s = offs.cpu().numpy(), sizes.cpu().numpy()
    got = go.buf.cpu().numpy()
    if got.tobytes() != want.tobytes():   # (first, so that a frame of another size is named with its tile)
        raise AssertionError(explain(got, want, go.lead, want_offs, want_sizes, info, which, W, H, bits, what))
    assert np.array_equal(o, want_offs), f"{what}: offsets {o[:8]}.. are not the oracle's {want_offs[:8]}.."
    assert np.array_equal(s, want_sizes), f"{what}: sizes {s[:8]}.. are not the oracle's {want_sizes[:8]}.."
    # by construction, not through the oracle: the depth and minimum arrays of every distinct frame
    for d, (name, f, depth, minimum) in enumerate(info):
        k = int(np.nonzero(which == d)[0][-1])
        a = go.lead + int(o[k])
        gd, gm, _, _ = ci.frame_arrays(got[a: a + int(s[k])], W, H, bits)
        for field, g, w in (("depth", gd, depth), ("minimum", gm, minimum)):
            if not np.array_equal(g, w):
                tile = int(np.nonzero(g != w)[0][0])
                grid = ci.Grid(W, H)
                raise AssertionError(f"{what}: entry {k} ({name}, frame {f}) tile {tile} (rm {int(grid.vc[tile])}, dm "
                                     f"{int(grid.vr[tile])}): {field} {int(g[tile])} is not the {int(w[tile])} the "
                                     f"construction gives")
    assert torch.equal(gi.buf, before), f"{what}: the encoder wrote into the images or their guard"
    total = int(want_offs[-1] + want_sizes[-1])
    back = decode(go.buf, go.lead, total, offs)
    codec.sync()
    if not torch.equal(back, images):
        k = int((back != images).reshape(n, -1).any(1).nonzero()[0][0])
        raise AssertionError(f"{what}: decoding the GPU's bytes: entry {k} ({info[which[k]][0]}) is not the image")


@pytest.mark.parametrize("batch", ["mixed", "padding_trap"])
@pytest.mark.parametrize("case", ENCODE_CASES, ids=case_id)
def test_encoder_forms_on_crafted_images(dv, codec, oracle, case, batch):
    W, H, n, layout, residue, form = case
    stride = slot_stride(layout, W, H)
    T = ((W + 7) // 8) * ((H + 7) // 8)

    def encode(images, out, lead, cap):
        plan = dv.encode_plan(W, H, n, images.data_ptr(), out.data_ptr() + lead, stride)
        got = tuple(plan[k] for k in FORM_KEYS)
        assert got == form, f"{case_id(case)}: encode_plan at the device addresses {plan} is not {form}"
        return codec.encode_frames(images, W, H, n, out, lead, cap, first_index=FIRST_INDEX, slot_stride=stride)

    def decode(out, lead, total, offs):
        return codec.decode_frames(out, lead, total, offs, W, H, n)[0]

    if batch == "mixed":
        batches, fill = mixed_frames(W, H, n, 8, runs_of(dv.encode_plan(W, H, n, residue, 0, stride), T)), SENTINEL
    else:
        batches, fill = trap_frames(W, H, n, 8), ci.GUARD
    for imgs, info, which in batches:
        what = f"{case_id(case)} (rm {W % 8 or 8}, dm {H % 8 or 8}) {batch} batch"
        run_batch(codec, what, W, H, 8, imgs, info, which, residue, 0, stride, lambda img: oracle.pack_image(img, W, H),
                  fill, encode, decode)
