"""Temporal binning of a .dbde file: every run of group_frames frames becomes one frame (Codec.project_groups;
DESIGN.md 4.14).

bin_file() reads the source in pieces, finds the frames of each piece with the device scanner, reduces whole groups
straight from the compressed bytes (no source image is written), forms the binned images in torch and appends them,
encoded, to the destination behind a video header whose frame rate is divided by group_frames.  8-bit files only
(DBDE16 has no file form).
"""
import numpy as np
import torch

from . import pack_video_header, tiles, unpack_video_header

STATS = ("mean", "max", "min")
REJECTED = 0xFFFFFFFF   # header.u64s of a frame that failed validation (d_results)


def bin_file(codec, src_path, dst_path, group_frames, stat="mean", batch_bytes=256 << 20):
    """Bins the frames of the .dbde file src_path group_frames by group_frames into dst_path: each output frame is the
    per-pixel mean (rounded to nearest: (2 * sum + count) // (2 * count)), max or min of its group's accepted frames and
    carries the index and elapsed_ns of the group's first accepted frame; the video header carries frame_hz /
    group_frames.  batch_bytes: bytes of the source read per piece; pieces are cut at multiples of group_frames frames,
    the remainder is carried into the next piece, and a piece grows until it holds a whole group.  A group without an
    accepted frame is left out; the last, shorter group is written.  Returns (groups written, frames rejected, bytes of
    dst_path)."""
    g = int(group_frames)
    if g < 1 or g > 65536:
        raise ValueError(f"group_frames must be 1..65536, not {group_frames!r}")
    if stat not in STATS:
        raise ValueError(f"stat must be one of {STATS}, not {stat!r}")
    written = rejected = 0
    with open(src_path, "rb") as src, open(dst_path, "wb") as dst:
        used, (u64s, H, W, hz) = unpack_video_header(np.frombuffer(src.read(28), np.uint8))
        W, H = int(W), int(H)
        T = tiles(W, H)
        dst.write(pack_video_header(u64s, H, W, hz / g).tobytes())
        carry = b""
        while True:
            fresh = src.read(max(int(batch_bytes), 1))
            data = carry + fresh
            if not data or (not fresh and len(data) < 32 + 2 * T):
                break   # the end, or a cut frame behind the last whole one
            buf = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(codec.device)
            offs, n = codec.index_stream(buf, 0, len(data), W, H, len(data) // (32 + 2 * T) + 1)
            m = n // g * g if fresh else n   # whole groups; at the end of the file the last, shorter one too
            if m == 0:
                if not fresh:
                    break
                carry = data   # not one whole group yet: read on
                continue
            gp, res = codec.project_groups(buf, 0, len(data), offs, W, H, m, group_frames=g,
                                           stats=("sum",) if stat == "mean" else (stat,))
            ng = gp.counts.numel()
            count = gp.counts.to(torch.int64)
            if stat == "mean":
                c = count.clamp(min=1).view(-1, 1, 1)
                images = ((2 * gp.sums() + c) // (2 * c)).to(torch.uint8)
            else:
                images = getattr(gp, stat)
            # the first accepted frame of every group: its index and elapsed_ns go into the binned frame's header
            ok = (res[:, 0] & 0xFFFFFFFF) != REJECTED
            frame = torch.arange(m, device=res.device)
            first = torch.full((ng * g,), m, dtype=torch.int64, device=res.device)
            first[:m] = torch.where(ok, frame, torch.full_like(frame, m))
            first = first.view(ng, g).amin(1)
            keep = count > 0
            k = int(keep.sum().item())
            if k:
                at = first[keep]
                out, lead, cap = codec.alloc_stream(W, H, k)
                o, b = codec.encode_frames(images[keep].contiguous(), W, H, k, out, lead, cap,
                                           indices=res[at, 1].contiguous(), elapsed_ns=res[at, 2].contiguous())
                codec.sync()
                dst.write(out[lead: lead + int((o[k - 1] + b[k - 1]).item())].cpu().numpy().tobytes())
            written += k
            rejected += m - int(ok.sum().item())
            if m < n:
                end = int(offs[m].item())
            else:
                last = int(offs[n - 1].item())
                n64 = int.from_bytes(data[last + 28 + 2 * T: last + 32 + 2 * T], "little")
                end = last + 32 + 2 * T + 8 * n64
            carry = data[end:]
            if not fresh:
                break
        size = dst.tell()
    return written, rejected, size
