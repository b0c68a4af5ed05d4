"""Compressed-domain crop (dbde_hip_crop_frames) against the path it replaces, decode_roi + encode_frames.

    python profiles/crop_bench.py [--rounds 3] [--seconds 0.6] [--only mixed4k|noise4k|u16] [--out profiles/crop_bench.jsonl]

Datasets (each encoded on the device into one slot per frame): 1,024 mixed and 1,024 noise8 4096x3072 DBDE frames, and
128 DBDE16 frames of 4096x3072 with a per-tile depth uniform in 0..16 (profiles/roi16_bench.py's).  Cases: windows of
256x256, 1024x1024 and 2045x2043 (both edges cut tiles) at (1000, 696), the full frame, and one frame per call at
512x512.  Arms, timed with device events over repeated calls (at least --seconds of work per figure, after a warm-up),
alternated round by round so that the spread shows:
  a  crop_frames, concatenated output
  b  decode_roi, then encode_frames of the windows (the path the crop replaces), concatenated output
  c  decode_roi alone
  d  a torch device copy of as many bytes as the cropped frames hold (the floor)
Prints one JSON line per (dataset, case, arm, round):
  ms             time of one call
  read_bytes     bytes the call must read at least, computed here from the streams' depth arrays: the depth arrays
                 (the index), the window tiles' minima and payload (a, b, c; b also reads the windows back); d the copy
  written_bytes  the cropped frames (a, b, d; b also writes the windows), the windows (c)
  share_of_peak  (read_bytes + written_bytes) / time against 8 TB/s
The crop is checked once against arm b's bytes before any timing.
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12
CASES = [("256x256", 1000, 696, 256, 256, None), ("1024x1024", 1000, 696, 1024, 1024, None),
         ("2045x2043", 1000, 696, 2045, 2043, None), ("full", 0, 0, 4096, 3072, None),
         ("512x512 one frame", 1000, 696, 512, 512, 1)]


def timed(fn, seconds):
    """ms per call over at least `seconds` of calls (device events around the whole run)."""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    one = max(a.elapsed_time(b), 1e-3)
    reps = max(3, math.ceil(seconds * 1e3 / one))
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps, reps


def make8(codec, dv, content, W, H, n):
    import torch
    slot = (dv.max_frame_bytes(W, H) + 255) // 256 * 256
    buf = torch.empty(n * slot + 256, dtype=torch.uint8, device="cuda")
    offs = torch.empty(n, dtype=torch.int64, device="cuda")
    sizes = torch.empty(n, dtype=torch.int64, device="cuda")
    step = max(1, min(n, (1 << 28) // (W * H)))
    for f0 in range(0, n, step):   # synthesize and encode in groups
        k = min(step, n - f0)
        imgs = codec.synth_frames(content, 0xDBDE2016, f0, k, W, H)
        o, s = codec.encode_frames(imgs, W, H, k, buf, f0 * slot, (n - f0) * slot, first_index=f0, slot_stride=slot)
        offs[f0:f0 + k] = o + f0 * slot
        sizes[f0:f0 + k] = s
        del imgs
    codec.sync()
    return buf, offs, n * slot


def make16(codec, W, H, n):
    import torch
    w, h = W // 8, H // 8
    g = torch.Generator(device="cuda").manual_seed(1)
    d = torch.randint(0, 17, (n, h, w), device="cuda", generator=g)
    dd = d.repeat_interleave(8, 1).repeat_interleave(8, 2)
    mask = (torch.ones_like(dd) << dd) - 1
    noise = torch.randint(0, 65536, (n, H, W), device="cuda", generator=g) & mask
    base = torch.randint(0, 32768, (n, h, w), device="cuda", generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2)
    imgs = torch.minimum(base, 65535 - mask).add_(noise).to(torch.int32).to(torch.int16).contiguous()
    del d, dd, mask, noise, base
    slot = (int(codec.L.dbde16_hip_max_frame_bytes(W, H)) + 255) // 256 * 256
    buf = torch.empty(n * slot + 256, dtype=torch.uint8, device="cuda")
    offs, _ = codec.encode_frames16(imgs, W, H, n, buf, 0, n * slot, slot_stride=slot)
    codec.sync()
    return buf, offs, n * slot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.6)
    ap.add_argument("--only", default=None, help="one dataset: mixed4k, noise4k or u16")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    import torch
    import dbde_video_cpp_amd as dv

    codec = dv.Codec(0)
    W, H = 4096, 3072
    w, h = W // 8, H // 8
    T = w * h
    lines = []
    for name, content, bits, n_all in (("mixed4k", "mixed", 8, 1024), ("noise4k", "noise8", 8, 1024), ("u16", "u16", 16, 128)):
        if a.only and name != a.only:
            continue
        pix = bits // 8
        buf, offs_all, stream_bytes = make8(codec, dv, content, W, H, n_all) if bits == 8 else make16(codec, W, H, n_all)
        crop = codec.crop_frames if bits == 8 else codec.crop_frames16
        roi = codec.decode_roi if bits == 8 else codec.decode_roi16
        maxf = dv.max_frame_bytes if bits == 8 else (lambda rw, rh: int(codec.L.dbde16_hip_max_frame_bytes(rw, rh)))
        depth = torch.empty((n_all, T), dtype=torch.uint8, device="cuda")
        ar = torch.arange(T, device="cuda")
        for f0 in range(0, n_all, 64):
            k = min(64, n_all - f0)
            depth[f0:f0 + k] = buf[(offs_all[f0:f0 + k, None] + 24 + ar[None, :]).reshape(-1)].view(k, T)
        for case, x, y, rw, rh, nf in CASES:
            n = nf or n_all
            offs = offs_all[:n]
            cap = n * maxf(rw, rh)
            out_a = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
            out_b = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
            win = torch.empty((n, rh, rw), dtype=torch.uint8 if bits == 8 else torch.int16, device="cuda")
            oo = torch.empty(n, dtype=torch.int64, device="cuda")
            ob = torch.empty(n, dtype=torch.int64, device="cuda")
            eo, eb = torch.empty_like(oo), torch.empty_like(ob)
            res = torch.empty((n, 4), dtype=torch.int64, device="cuda")

            def arm_a():
                crop(buf, 0, stream_bytes, offs, W, H, n, x, y, rw, rh, out_a, 32, cap, out_offsets=oo, out_bytes=ob,
                     results=res)

            def arm_c():
                roi(buf, 0, stream_bytes, offs, W, H, n, x, y, rw, rh, out=win, results=res)

            def arm_b():
                arm_c()
                if bits == 8:
                    codec.encode_frames(win, rw, rh, n, out_b, 32, cap, offsets=eo, nbytes=eb)
                else:
                    codec.encode_frames16(win, rw, rh, n, out_b, 32, cap)

            arm_a()
            codec.sync()
            total = int((oo[-1] + ob[-1]).item())
            arm_b()
            codec.sync()
            assert torch.equal(out_a[32:32 + total], out_b[32:32 + total]), (name, case)
            src_copy = out_b[32:32 + total]
            dst_copy = torch.empty_like(src_copy)

            def arm_d():
                dst_copy.copy_(src_copy)

            pl = (dv.crop_plan if bits == 8 else dv.crop16_plan)(W, H, n, x, y, rw, rh)
            tx0, ty0, ntx, nty = pl["tile_x"], pl["tile_y"], pl["tiles_x"], pl["tiles_y"]
            pay = 8 * int(depth[:n].view(n, h, w)[:, ty0:ty0 + nty, tx0:tx0 + ntx].to(torch.int64).sum().item())
            src = n * T + n * ntx * nty * (1 + pix) + pay
            wbytes = n * rw * rh * pix
            rb = {"a": src, "b": src + wbytes, "c": src, "d": total}
            wb = {"a": total, "b": total + wbytes, "c": wbytes, "d": total}
            arms = [("a crop_frames", arm_a), ("b decode_roi + encode_frames", arm_b), ("c decode_roi", arm_c),
                    ("d torch copy of the output bytes", arm_d)]
            for _, fn in arms:   # warm-up
                fn()
            codec.sync()
            for rnd in range(a.rounds):
                order = arms if rnd % 2 == 0 else arms[::-1]
                for arm, fn in order:
                    ms, reps = timed(fn, a.seconds)
                    k = arm[0]
                    ln = dict(dataset=name, content=content, bits=bits, W=W, H=H, frames=n, case=case,
                              window=[x, y, rw, rh], recoded_tiles=pl["recoded_tiles"], arm=arm, round=rnd, reps=reps,
                              ms=ms, read_bytes=rb[k], written_bytes=wb[k], out_bytes=total,
                              share_of_peak=(rb[k] + wb[k]) / (ms * 1e-3) / PEAK, measured=True)
                    print(json.dumps(ln), flush=True)
                    lines.append(ln)
            del out_a, out_b, win, src_copy, dst_copy
            torch.cuda.empty_cache()
        del buf, depth
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    codec.close()


if __name__ == "__main__":
    main()
