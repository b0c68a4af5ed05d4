"""Shared by the GPU tests of the compressed-domain crop (test infrastructure, not a test module).

run_crop() calls Codec.crop_frames / crop_frames16 into a canvas that holds a position-dependent canary pattern in
front of, between and behind the frames; check_host() compares the call's frames, offsets, bytes, origins and results
with tests/crop_ref.py and every other byte of the canvas with the canary.  Stream / Stream16 are device-made source
batches for the device-scale comparisons with encode_frames(decode_roi(...)).
"""
import numpy as np

import crafted
import crop_ref

GUARD = 96


def canary(n, device="cuda"):
    import torch
    return ((torch.arange(n, dtype=torch.int64, device=device) * 37 + 11) & 0xFF).to(torch.uint8)


def max_frame(rw, rh, bits):
    return crop_ref.max_frame_bytes(rw, rh, bits)


def capacity(n, rw, rh, bits, slot_stride):
    return (n - 1) * slot_stride + max_frame(rw, rh, bits) if slot_stride else n * max_frame(rw, rh, bits)


class Crop:
    """What one crop call left: canvas (device), base (byte of d_out in it), cap, offsets / nbytes / used (numpy),
    results (device tensor)."""

    def frame(self, f):
        a = self.base + int(self.offsets[f])
        return self.canvas[a: a + int(self.nbytes[f])]

    def untouched_outside_frames(self):
        """Every byte of the canvas outside the accepted frames still holds the canary."""
        want = canary(self.canvas.numel())
        at = 0
        spans = sorted((self.base + int(o), self.base + int(o) + int(b)) for o, b in zip(self.offsets, self.nbytes) if b)
        for s0, s1 in spans + [(self.canvas.numel(), self.canvas.numel())]:
            assert s0 >= at, "frames overlap"
            if not bool((self.canvas[at:s0] == want[at:s0]).all()):
                bad = int((self.canvas[at:s0] != want[at:s0]).nonzero()[0]) + at
                raise AssertionError(f"byte {bad - self.base} (relative to d_out) outside every frame was written")
            at = s1


def run_crop(codec, bits, buf, lead, total, offs, W, H, n, x, y, rw, rh, origins=None, slot_stride=0, out_misalign=0):
    import torch
    cap = capacity(n, rw, rh, bits, slot_stride) if n else 0
    c = Crop()
    c.base, c.cap = GUARD + out_misalign, cap
    c.canvas = canary(c.base + cap + GUARD)
    org = None
    if origins is not None:
        org = torch.tensor(np.asarray(origins, np.int32).reshape(n, 2), dtype=torch.int32, device="cuda")
    used = torch.full((max(n, 1), 2), -7, dtype=torch.int32, device="cuda")
    fn = codec.crop_frames if bits == 8 else codec.crop_frames16
    o, b, c.results = fn(buf, lead, total, offs, W, H, n, x, y, rw, rh, c.canvas, c.base, cap, origins=org,
                         slot_stride=slot_stride, origins_used=used)
    codec.sync()
    c.offsets, c.nbytes, c.used = o.cpu().numpy(), b.cpu().numpy(), used.cpu().numpy()[:n]
    return c


def check_host(c, frames, W, H, x, y, rw, rh, bits=8, origins=None, slot_stride=0, what=""):
    """The call's outputs against crop_ref.crop_batch of the host frames (None / broken ones are rejected)."""
    outs, offs, nbytes, used = crop_ref.crop_batch(frames, W, H, x, y, rw, rh, bits, origins, slot_stride)
    assert c.offsets.tolist() == offs.tolist(), (what, c.offsets.tolist(), offs.tolist())
    assert c.nbytes.tolist() == nbytes.tolist(), (what, c.nbytes.tolist(), nbytes.tolist())
    assert c.used.tolist() == used.tolist(), (what, c.used.tolist(), used.tolist())
    for f, want in enumerate(outs):
        if want is not None:
            got = c.frame(f).cpu().numpy()
            if got.tobytes() != want.tobytes():
                import crafted_images as ci
                raise AssertionError(f"{what} frame {f}: {ci.first_difference(got, want, rw, rh, bits)}")
    c.untouched_outside_frames()
    return outs


def upload(frames, how="concat", lead=32, slot=0, misalign=0):
    """Host frames in a device stream buffer (crafted.layout) -> (buf, lead, offs tensor, total)."""
    import torch
    host, lead, offs, total = crafted.layout(frames, how, lead, slot)
    if misalign:
        host = np.concatenate([np.full(misalign, 0x5A, np.uint8), host])
        lead += misalign
    return torch.from_numpy(host).cuda(), lead, torch.from_numpy(offs).cuda(), total


class Stream:
    """n synthetic frames encoded on the device (8-bit), concatenated or in slots, at a chosen residue of the base."""
    bits = 8

    def __init__(self, codec, dv, mode, W, H, n, first=0, slot_extra=None, misalign=0, seed=0xC20B2016):
        self.W, self.H, self.n, self.first = W, H, n, first
        self.images = codec.synth_frames(mode, seed, first, n, W, H)
        self.slot = dv.max_frame_bytes(W, H) + slot_extra if slot_extra is not None else 0
        self.buf, self.lead, cap = codec.alloc_stream(W, H, n, slot_stride=self.slot, lead=48)
        self.lead += misalign
        self.buf.fill_(0xA5)
        self.offs, self.sizes = codec.encode_frames(self.images, W, H, n, self.buf, self.lead, cap,
                                                    first_index=first, slot_stride=self.slot)
        codec.sync()
        self.total = int((self.offs[-1] + self.sizes[-1]).item())

    def moved(self, misalign):
        """A copy of the stream at another residue of the base."""
        import copy
        import torch
        s = copy.copy(self)
        s.buf = torch.full((self.buf.numel() + 16,), 0xA5, dtype=torch.uint8, device="cuda")
        s.lead = 48 + misalign
        s.buf[s.lead: s.lead + self.total] = self.buf[self.lead: self.lead + self.total]
        return s

    def roi_encode(self, codec, x, y, rw, rh, canvas, base, cap, slot_stride, origins=None):
        """The path the crop replaces: decode_roi, then encode_frames of the windows, into `canvas`."""
        win, _ = codec.decode_roi(self.buf, self.lead, self.total, self.offs, self.W, self.H, self.n, x, y, rw, rh,
                                  origins=origins)
        return codec.encode_frames(win, rw, rh, self.n, canvas, base, cap, first_index=self.first,
                                   slot_stride=slot_stride)


class Stream16(Stream):
    """The same for DBDE16: full-range pixels shifted down per 8 x 8 tile, so that every depth 0..16 occurs."""
    bits = 16

    def __init__(self, codec, dv, W, H, n, first=0, slot_extra=None, misalign=0, seed=16):
        import torch
        self.W, self.H, self.n, self.first = W, H, n, first
        g = torch.Generator(device="cuda").manual_seed(seed)
        w, h = (W + 7) // 8, (H + 7) // 8
        px = torch.randint(0, 65536, (n, 8 * h, 8 * w), dtype=torch.int32, device="cuda", generator=g)
        sh = torch.randint(0, 18, (n, h, 1, w, 1), dtype=torch.int32, device="cuda", generator=g)
        px = (px.view(n, h, 8, w, 8) >> sh).view(n, 8 * h, 8 * w)[:, :H, :W]
        base = torch.randint(0, 65536, (n, 1, 1), dtype=torch.int32, device="cuda", generator=g)
        self.images = ((px + base) & 0xFFFF).to(torch.int16).contiguous()
        maxf = int(codec.L.dbde16_hip_max_frame_bytes(W, H))
        self.slot = maxf + slot_extra if slot_extra is not None else 0
        cap = (n - 1) * self.slot + maxf if self.slot else n * maxf
        self.lead = 48 + misalign
        self.buf = torch.full((self.lead + cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
        self.offs, self.sizes = codec.encode_frames16(self.images, W, H, n, self.buf, self.lead, cap, first_index=first,
                                                      slot_stride=self.slot)
        codec.sync()
        self.total = int((self.offs[-1] + self.sizes[-1]).item())

    def roi_encode(self, codec, x, y, rw, rh, canvas, base, cap, slot_stride, origins=None):
        win, _ = codec.decode_roi16(self.buf, self.lead, self.total, self.offs, self.W, self.H, self.n, x, y, rw, rh,
                                    origins=origins)
        return codec.encode_frames16(win, rw, rh, self.n, canvas, base, cap, first_index=self.first,
                                     slot_stride=slot_stride)


def check_device(codec, s, x, y, rw, rh, slot_extra=None, out_misalign=0, origins=None, what=""):
    """crop_frames of the device stream s against encode_frames(decode_roi(...)) of the same windows, on the device:
    offsets, bytes, every frame's bytes, and the canary outside them."""
    import torch
    slot = max_frame(rw, rh, s.bits) + slot_extra if slot_extra is not None else 0
    used = None
    c = run_crop(codec, s.bits, s.buf, s.lead, s.total, s.offs, s.W, s.H, s.n, x, y, rw, rh, origins=origins,
                 slot_stride=slot, out_misalign=out_misalign)
    if origins is not None:
        used = torch.from_numpy(c.used.copy()).cuda()   # decode_roi takes the rounded origins as they are
    ref = canary(c.canvas.numel())
    o, b = s.roi_encode(codec, x, y, rw, rh, ref, c.base, c.cap, slot, origins=used)
    codec.sync()
    assert c.offsets.tolist() == o.cpu().tolist(), (what, c.offsets.tolist(), o.cpu().tolist())
    assert c.nbytes.tolist() == b.cpu().tolist(), (what, c.nbytes.tolist(), b.cpu().tolist())
    for f in range(s.n):
        a = c.base + int(c.offsets[f])
        if not torch.equal(c.frame(f), ref[a: a + int(c.nbytes[f])]):
            import crafted_images as ci
            got, want = c.frame(f).cpu().numpy(), ref[a: a + int(c.nbytes[f])].cpu().numpy()
            raise AssertionError(f"{what} frame {f}: {ci.first_difference(got, want, rw, rh, s.bits)}")
    c.untouched_outside_frames()
    rows = codec.parse_results(c.results)
    assert rows == [(2, s.first + f, 0, int(s.sizes[f])) for f in range(s.n)], (what, rows)
    return c
