"""The window encoder's model and the helpers its tests share (test infrastructure, not a test module).

Model (NumPy + the oracle, no GPU): a pitched byte buffer -> the clamped origin of each frame -> the rw x rh window ->
the oracle's frame of that window (Oracle.pack_frame for DBDE, dbde16_oracle_pack_frame for DBDE16).  Expected bytes
never come from the library's own encoder.

Source layout, as include/dbde_hip.h states it: pixel (x, y) of image f is at byte base + f * frame_stride + y * pitch +
x * PIX of the buffer, PIX = bits / 8; pitch and frame_stride in bytes.

GPU side: Source puts such a buffer on the device, run() calls dbde_hip_encode_window / dbde16_hip_encode_window (the
C-ABI itself, so that image_bytes, pitch and base are exactly the test's) into a sentinel-filled canvas, and check()
compares frames, offsets and sizes with the model and every other byte of the canvas with the sentinel.
"""
import ctypes as C
import struct

import numpy as np

SENTINEL = 0xC3
GUARD = 64


def pix_of(bits):
    return bits // 8


def max_frame_bytes(rw, rh, bits=8):
    T = ((rw + 7) // 8) * ((rh + 7) // 8)
    return 32 + (66 if bits == 8 else 131) * T


def clamp_origin(x, y, W, H, rw, rh):
    """dbde_hip_decode_roi's documented rule: a per-frame origin is clamped into [0, W-rw] x [0, H-rh]."""
    return min(max(int(x), 0), W - rw), min(max(int(y), 0), H - rh)


def compact(W, H, bits=8, pitch=0, frame_stride=0):
    """(pitch, frame_stride) with 0 replaced by the compact values."""
    pitch = pitch or W * pix_of(bits)
    return pitch, frame_stride or H * pitch


def min_image_bytes(W, H, n, bits=8, pitch=0, frame_stride=0):
    pitch, frame_stride = compact(W, H, bits, pitch, frame_stride)
    return (n - 1) * frame_stride + (H - 1) * pitch + W * pix_of(bits) if n else 0


def window(buf, base, pitch, frame_stride, f, x, y, rw, rh, bits=8):
    """The rw x rh window at (x, y) of image f, read byte by byte from the buffer: (rh, rw) uint8 / uint16."""
    px = pix_of(bits)
    rows = [buf[base + f * frame_stride + (y + r) * pitch + x * px: base + f * frame_stride + (y + r) * pitch + (x + rw) * px]
            for r in range(rh)]
    a = np.ascontiguousarray(np.stack(rows))
    return a if bits == 8 else a.view("<u2")


def packer(oracle, bits=8):
    """pack(index, image) -> the oracle's frame of an (H, W) image."""
    if bits == 8:
        return lambda index, img: oracle.pack_frame(int(index), np.ascontiguousarray(img, np.uint8), img.shape[1], img.shape[0])
    from oracle_ffi import ORACLE_SO
    L = C.CDLL(ORACLE_SO)
    u8p, u16p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint16)
    L.dbde16_oracle_pack_frame.restype = C.c_size_t
    L.dbde16_oracle_pack_frame.argtypes = [C.c_uint64, u16p, C.c_int, C.c_int, u8p]

    def pack(index, img):
        H, W = img.shape
        img = np.ascontiguousarray(img, np.uint16)
        out = np.full(max_frame_bytes(W, H, 16) + 16, 0xEE, np.uint8)
        n = L.dbde16_oracle_pack_frame(int(index), img.ctypes.data_as(u16p), W, H, out.ctypes.data_as(u8p))
        assert (out[n:] == 0xEE).all()
        return out[:n].copy()
    return pack


def encode_window(pack, buf, base, W, H, pitch, frame_stride, n, x, y, rw, rh, bits=8, origins=None, first_index=0,
                  indices=None, elapsed_ns=None, slot_stride=0):
    """The model of one call: ([frame bytes], offsets, sizes) with the encoders' layouts (slot_stride 0: concatenated).
    elapsed_ns travels as an F64 in bytes 12..20 of the frame header (the oracle's pack_frame writes 0 there)."""
    pitch, frame_stride = compact(W, H, bits, pitch, frame_stride)
    frames, offs, sizes, at = [], [], [], 0
    for f in range(n):
        ox, oy = (x, y) if origins is None else clamp_origin(origins[f][0], origins[f][1], W, H, rw, rh)
        idx = first_index + f if indices is None else int(indices[f])
        fr = pack(idx, window(buf, base, pitch, frame_stride, f, ox, oy, rw, rh, bits))
        if elapsed_ns is not None:
            fr[12:20] = np.frombuffer(struct.pack("<d", float(int(elapsed_ns[f]))), np.uint8)
        frames.append(fr)
        offs.append(f * slot_stride if slot_stride else at)
        sizes.append(len(fr))
        at += len(fr)
    return frames, offs, sizes


def embed(images, W, H, x, y, bits=8, pitch=0, frame_stride=0, base=0, fill=0, exact=False, tail=GUARD):
    """A source buffer of len(images) W x H images at `base`, filled with `fill` (a pixel value), with images[f] (rh, rw)
    at (x, y) of image f.  exact: the buffer ends with the last image's last window pixel.  -> uint8 buffer."""
    px = pix_of(bits)
    n = len(images)
    rh, rw = images[0].shape
    pitch, frame_stride = compact(W, H, bits, pitch, frame_stride)
    size = base + (n - 1) * frame_stride + ((y + rh - 1) * pitch + (x + rw) * px if exact
                                            else (H - 1) * pitch + W * px + tail)
    assert bits == 8 or base % 2 == 0
    buf = (np.full(size, fill, np.uint8) if bits == 8
           else np.full((size + 1) // 2, fill, "<u2").view(np.uint8)[:size].copy())
    for f, img in enumerate(images):
        b = np.ascontiguousarray(img, np.uint8 if bits == 8 else "<u2").view(np.uint8).reshape(rh, rw * px)
        for r in range(rh):
            at = base + f * frame_stride + (y + r) * pitch + x * px
            buf[at: at + rw * px] = b[r]
    return buf


# ---- GPU side ------------------------------------------------------------------------------------------------------

class Source:
    """A host source buffer on the device.  image_bytes: the extent the call is given (default: to the buffer's end)."""

    def __init__(self, buf, base, W, H, n, bits=8, pitch=0, frame_stride=0, image_bytes=None):
        import torch
        self.host, self.base, self.W, self.H, self.n, self.bits = buf, base, W, H, n, bits
        self.pitch, self.frame_stride = pitch, frame_stride
        self.dev = torch.from_numpy(buf).cuda()
        self.image_bytes = len(buf) - base if image_bytes is None else image_bytes

    def view(self):
        """The source as a strided torch view (n, H, W) of the device buffer."""
        import torch
        px = pix_of(self.bits)
        pitch, stride = compact(self.W, self.H, self.bits, self.pitch, self.frame_stride)
        t = self.dev if px == 1 else self.dev[self.base % 2:][: (len(self.dev) - self.base % 2) // 2 * 2].view(torch.int16)
        return torch.as_strided(t, (self.n, self.H, self.W), (stride // px, pitch // px, 1), self.base // px)


class Result:
    pass


def run(codec, src, x, y, rw, rh, origins=None, first_index=0, indices=None, elapsed_ns=None, slot_stride=0,
        out_misalign=0, cap=None, sentinel=SENTINEL):
    """One C-ABI call into a sentinel canvas -> Result(rc, canvas (numpy), base, cap, offsets, sizes)."""
    import torch
    n, bits = src.n, src.bits
    maxf = max_frame_bytes(rw, rh, bits)
    need = ((n - 1) * slot_stride + maxf if slot_stride else n * maxf) if n else 0
    r = Result()
    r.cap = need if cap is None else cap
    r.base = GUARD + out_misalign
    canvas = torch.full((r.base + max(need, r.cap) + GUARD,), sentinel, dtype=torch.uint8, device="cuda")
    offs = torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda")
    sizes = torch.full((max(n, 1),), -1, dtype=torch.int64, device="cuda")
    org = None if origins is None else torch.tensor(np.asarray(origins, np.int32).reshape(n, 2), dtype=torch.int32, device="cuda")
    ind = None if indices is None else torch.tensor(np.asarray(indices, np.uint64).view(np.int64), dtype=torch.int64, device="cuda")
    ela = None if elapsed_ns is None else torch.tensor(np.asarray(elapsed_ns, np.uint64).view(np.int64), dtype=torch.int64, device="cuda")
    p = lambda t: None if t is None else t.data_ptr()   # noqa: E731
    common = (codec.h, src.dev.data_ptr() + src.base, src.image_bytes, src.W, src.H, src.pitch, src.frame_stride, n, x, y, rw,
              rh, p(org), first_index)
    tail = (canvas.data_ptr() + r.base, r.cap, slot_stride, offs.data_ptr(), sizes.data_ptr())
    if bits == 8:
        r.rc = codec.L.dbde_hip_encode_window(*common, p(ind), p(ela), *tail)
    else:
        r.rc = codec.L.dbde16_hip_encode_window(*common, *tail)
    r.error = codec.L.dbde_hip_last_error(codec.h).decode()
    if r.rc == 0:
        codec.sync()
    else:
        torch.cuda.synchronize()
    r.canvas = canvas.cpu().numpy()
    r.offsets, r.sizes = offs.cpu().numpy()[:n], sizes.cpu().numpy()[:n]
    r.sentinel = sentinel
    return r


def frame_of(r, f):
    a = r.base + int(r.offsets[f])
    return r.canvas[a: a + int(r.sizes[f])]


def untouched(r, spans=None):
    """Every byte of the canvas outside the reported frames (or the given spans) is still the sentinel."""
    keep = np.ones(len(r.canvas), bool)
    for o, s in (zip(r.offsets, r.sizes) if spans is None else spans):
        keep[r.base + int(o): r.base + int(o) + int(s)] = False
    bad = np.nonzero(keep & (r.canvas != r.sentinel))[0]
    assert len(bad) == 0, f"byte {int(bad[0]) - r.base} (relative to d_out) outside every frame was written"


def check(r, frames, offs, sizes, rw, rh, bits=8, what=""):
    """The call's outputs against the model's."""
    import crafted_images as ci
    assert r.rc == 0, (what, r.rc, r.error)
    assert r.offsets.tolist() == list(offs), (what, r.offsets.tolist(), list(offs))
    assert r.sizes.tolist() == list(sizes), (what, r.sizes.tolist(), list(sizes))
    for f, want in enumerate(frames):
        got = frame_of(r, f)
        if got.tobytes() != want.tobytes():
            raise AssertionError(f"{what} frame {f}: {ci.first_difference(got, want, rw, rh, bits)}")
    untouched(r)


def run_and_check(codec, pack, src, x, y, rw, rh, what="", **kw):
    r = run(codec, src, x, y, rw, rh, **kw)
    model_kw = {k: v for k, v in kw.items() if k in ("origins", "first_index", "indices", "elapsed_ns", "slot_stride")}
    frames, offs, sizes = encode_window(pack, src.host, src.base, src.W, src.H, src.pitch, src.frame_stride, src.n, x, y,
                                        rw, rh, src.bits, **model_kw)
    check(r, frames, offs, sizes, rw, rh, src.bits, what)
    return r, frames
