"""Scaled float decode (dbde_hip_decode_scaled) against decoding the window and scaling it in torch.

    python profiles/scaled_bench.py [--rounds 3] [--seconds 0.6] [--only mixed4k] [--out profiles/scaled_bench.jsonl]

Datasets (each encoded on the device into one slot per frame): 256 mixed and 256 noise8 4096x3072 DBDE frames, and 64
DBDE16 4096x3072 frames (a per-frame mix of bit depths).  For each dataset: the full frame, 1024x1024 and 256x256
windows at (1000, 696), and 512x512 with one frame per call; outputs F32, F16 and BF16; both maps, and scalars only.
Arms, all in one process, timed with device events over repeated calls (at least --seconds of work per figure, after a
warm-up), alternated round by round so that the spread shows:
  a  decode_scaled
  b  the path it replaces: decode_roi (decode_frames for the full frame), then ((w.float() - dark_w) * gain_w).to(dtype)
     in torch (DBDE16: the int16 tensor the decoder writes holds U16 bits; it is widened the cheapest way the
     installed torch has, viewed as uint16 where .float() of uint16 exists on the device, else through
     int32 & 0xFFFF, which costs arm b two more passes; every u16 line says which in "widen")
  c  decode_roi (decode_frames) alone
  d  a torch device copy of as many bytes as the output holds
(c and d are timed in the rounds of the "maps" case only: they do not depend on the maps.)
Arm a's bits are checked against arm b's before any timing.
Prints one JSON line per (dataset, window, type, maps, arm, round), and with --out appends each line to that file as
it is measured (a run that ends early leaves what it measured; run each dataset once, e.g. with --only):
  ms             time of one call
  bytes          arm a only: the bytes the call must move at least, computed here from the streams: the depth arrays
                 (the index), the window tiles' minimum bytes, the depth bytes from each window tile row's index chunk
                 start to its first tile, the window tiles' payload, each map's window ONCE (which assumes the maps
                 stay cached across the frames of a call), and the output
  share_of_peak  bytes / time against 8 TB/s
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12
W, H = 4096, 3072
WINDOWS = [("full", (0, 0, W, H), None), ("1024", (1000, 696, 1024, 1024), None), ("256", (1000, 696, 256, 256), None),
           ("512x1", (1000, 696, 512, 512), 1)]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.6)
    ap.add_argument("--only", default=None, help="one dataset: mixed4k, noise4k or u16")
    ap.add_argument("--out", default=None, help="also append each JSON line to this file as it is measured")
    a = ap.parse_args()

    import torch
    import dbde_video_cpp_amd as dv

    codec = dv.Codec(0)
    w, h = W // 8, H // 8
    T = w * h
    g = torch.Generator(device="cuda").manual_seed(2016)
    dark = torch.rand((H, W), device="cuda", generator=g) * 300.0
    gain = torch.exp2(torch.rand((H, W), device="cuda", generator=g) * 16.0 - 8.0)
    gain = torch.where(torch.rand((H, W), device="cuda", generator=g) < 0.5, -gain, gain).contiguous()
    d0, g0 = 0.0, 1.0 / 255.0
    sink = open(a.out, "a") if a.out else None
    try:   # does this torch widen uint16 on the device?  (not every build has the kernel)
        torch.zeros(4, dtype=torch.int16, device="cuda").view(torch.uint16).float()
        widen = "uint16"
    except (RuntimeError, TypeError, AttributeError):
        widen = "int32"
    for name, content, pix, n_all in (("mixed4k", "mixed", 1, 256), ("noise4k", "noise8", 1, 256), ("u16", "u16", 2, 64)):
        if a.only and name != a.only:
            continue
        maxf = dv.max_frame_bytes(W, H) if pix == 1 else int(codec.L.dbde16_hip_max_frame_bytes(W, H))
        slot = (maxf + 255) // 256 * 256
        buf = torch.empty(n_all * slot + 256, dtype=torch.uint8, device="cuda")
        offs = torch.empty(n_all, dtype=torch.int64, device="cuda")
        step = 16
        for f0 in range(0, n_all, step):   # synthesize and encode in groups
            if pix == 1:
                imgs = codec.synth_frames(content, 0xDBDE2016, f0, step, W, H)
                o, _ = codec.encode_frames(imgs, W, H, step, buf, f0 * slot, (n_all - f0) * slot, first_index=f0,
                                           slot_stride=slot)
            else:
                imgs = torch.randint(-32768, 32768, (step, H, W), dtype=torch.int16, device="cuda", generator=g)
                for k in range(step):   # 16, 12, 8 and 4 significant bits, frame by frame
                    imgs[k] = ((imgs[k].to(torch.int32) & 0xFFFF) >> (4 * (k % 4))).to(torch.int16)
                o, _ = codec.encode_frames16(imgs, W, H, step, buf, f0 * slot, (n_all - f0) * slot, first_index=f0,
                                             slot_stride=slot)
            offs[f0:f0 + step] = o + f0 * slot
            del imgs
        codec.sync()
        stream_bytes = n_all * slot
        roi = codec.decode_roi if pix == 1 else codec.decode_roi16
        frames = codec.decode_frames if pix == 1 else codec.decode_frames16
        scaled = codec.decode_scaled if pix == 1 else codec.decode_scaled16
        plan = dv.roi_plan if pix == 1 else dv.roi16_plan
        ar = torch.arange(T, device="cuda")
        depth = torch.empty((n_all, T), dtype=torch.uint8, device="cuda")
        for f0 in range(0, n_all, 16):
            depth[f0:f0 + 16] = buf[(offs[f0:f0 + 16, None] + 24 + ar[None, :]).reshape(-1)].view(16, T)
        depth = depth.view(n_all, h, w)

        for wname, (x, y, rw, rh), per_call in WINDOWS:
            n = per_call or n_all
            full = (rw, rh) == (W, H)
            ofs = offs[:n].contiguous()
            pdt = torch.uint8 if pix == 1 else torch.int16
            pixels = torch.empty((n, rh, rw), dtype=pdt, device="cuda")
            res = torch.empty((n, 4), dtype=torch.int64, device="cuda")
            dark_w, gain_w = dark[y:y + rh, x:x + rw], gain[y:y + rh, x:x + rw]

            def decode():
                if full and pix == 1:
                    frames(buf, 0, stream_bytes, ofs, W, H, n, images=pixels, results=res)
                elif full:
                    frames(buf, 0, stream_bytes, ofs, W, H, n, images=pixels)
                else:
                    roi(buf, 0, stream_bytes, ofs, W, H, n, x, y, rw, rh, out=pixels, results=res)

            pl = plan(W, H, n, x, y, rw, rh)
            tx0, ty0, ntx, nty = pl["tile_x"], pl["tile_y"], pl["tiles_x"], pl["tiles_y"]
            pay = 8 * int(depth[:n, ty0:ty0 + nty, tx0:tx0 + ntx].to(torch.int64).sum().item())
            pre = n * nty * (tx0 % 512 if pl["chunk_pieces"] else 0)
            stream_read = n * T + pix * n * ntx * nty + pre + pay

            for t in (torch.float32, torch.float16, torch.bfloat16):
                es = 4 if t == torch.float32 else 2
                out = torch.empty((n, rh, rw), dtype=t, device="cuda")
                src_copy = torch.empty((n, rh, rw), dtype=t, device="cuda")
                dst_copy = torch.empty_like(src_copy)
                for mname, dk, gn, dkw, gnw in (("maps", dark, gain, dark_w, gain_w), ("scalars", d0, g0, d0, g0)):
                    holder = {}

                    def arm_a():
                        scaled(buf, 0, stream_bytes, ofs, W, H, n, x, y, rw, rh, dtype=t, dark=dk, gain=gn, out=out,
                               results=res)

                    def arm_b():
                        decode()
                        if pix == 1:
                            p = pixels
                        elif widen == "uint16":
                            p = pixels.view(torch.uint16)
                        else:
                            p = pixels.to(torch.int32) & 0xFFFF
                        holder["v"] = ((p.float() - dkw) * gnw).to(t)

                    def arm_d():
                        dst_copy.copy_(src_copy)

                    arms = [("a decode_scaled", arm_a), ("b decode + torch", arm_b)]
                    if mname == "maps":   # c and d do not depend on the maps: once per window and type
                        arms += [("c decode alone", decode), ("d device copy of the output's bytes", arm_d)]
                    arm_a()
                    arm_b()
                    codec.sync()
                    iv = torch.int32 if es == 4 else torch.int16
                    assert torch.equal(out.view(iv), holder["v"].view(iv)), (name, wname, str(t), mname)
                    for _, fn in arms:   # warm-up
                        fn()
                    codec.sync()
                    n_maps = 2 if mname == "maps" else 0
                    nbytes = stream_read + n_maps * rw * rh * 4 + n * rw * rh * es
                    for rnd in range(a.rounds):
                        order = arms if rnd % 2 == 0 else arms[::-1]
                        for arm, fn in order:
                            ms, reps = timed(fn, a.seconds)
                            ln = dict(dataset=name, window=wname, x=x, y=y, rw=rw, rh=rh, frames=n, dtype=str(t)[6:],
                                      maps=mname, arm=arm, round=rnd, reps=reps, ms=ms, measured=True)
                            if arm[0] == "a":
                                ln.update(bytes=nbytes, share_of_peak=nbytes / (ms * 1e-3) / PEAK)
                            if pix == 2 and arm[0] == "b":
                                ln.update(widen=widen)
                            print(json.dumps(ln), flush=True)
                            if sink:
                                sink.write(json.dumps(ln) + "\n")
                                sink.flush()
                    holder.clear()
                del out, src_copy, dst_copy
            del pixels
            torch.cuda.empty_cache()
        del buf, depth
        torch.cuda.empty_cache()
    if sink:
        sink.close()
    codec.close()


if __name__ == "__main__":
    main()
