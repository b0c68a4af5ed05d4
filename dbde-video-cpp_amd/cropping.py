"""Cutting a sub-video out of a .dbde file in the compressed domain (Codec.crop_frames).

crop_file() reads the source in pieces, finds the frames of each piece with the device scanner, crops them
concatenated and appends the bytes to the destination behind a video header of the window's size.  No pixel is
written anywhere: tiles are copied as they are stored, only those the window's right / bottom edge cuts are re-packed.
8-bit files only (DBDE16 has no file form).
"""
import numpy as np
import torch

from . import pack_video_header, tiles, unpack_video_header


def crop_file(codec, src_path, dst_path, x, y, rw, rh, batch_bytes=256 << 20):
    """Crops the rw x rh window at (x, y; multiples of 8) out of every frame of the .dbde file src_path into dst_path
    (same frame_hz, frame headers kept).  batch_bytes: bytes of the source read per piece; a frame that a piece cuts is
    carried into the next piece, and a piece grows until it holds a whole frame.  Frames that fail validation are left
    out.  Returns (frames written, frames rejected, bytes of dst_path)."""
    written = rejected = 0
    with open(src_path, "rb") as src, open(dst_path, "wb") as dst:
        used, (u64s, H, W, hz) = unpack_video_header(np.frombuffer(src.read(28), np.uint8))
        W, H = int(W), int(H)
        T = tiles(W, H)
        dst.write(pack_video_header(u64s, rh, rw, hz).tobytes())
        carry = b""
        while True:
            fresh = src.read(max(int(batch_bytes), 1))
            data = carry + fresh
            if not data or (not fresh and len(data) < 32 + 2 * T):
                break   # the end, or a cut frame behind the last whole one
            buf = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(codec.device)
            offs, n = codec.index_stream(buf, 0, len(data), W, H, len(data) // (32 + 2 * T) + 1)
            if n == 0:
                if not fresh:
                    break
                carry = data   # not one whole frame yet: read on
                continue
            out, lead, cap = codec.alloc_stream(rw, rh, n)
            o, b, _ = codec.crop_frames(buf, 0, len(data), offs, W, H, n, x, y, rw, rh, out, lead, cap)
            codec.sync()
            last = int(offs[n - 1].item())
            n64 = int.from_bytes(data[last + 28 + 2 * T: last + 32 + 2 * T], "little")
            end = last + 32 + 2 * T + 8 * n64
            dst.write(out[lead: lead + int((o[n - 1] + b[n - 1]).item())].cpu().numpy().tobytes())
            ok = int((b > 0).sum().item())
            written += ok
            rejected += n - ok
            carry = data[end:]
            if not fresh:
                break
        size = dst.tell()
    return written, rejected, size
