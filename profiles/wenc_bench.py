"""Window encode (dbde_hip_encode_window) against the path it replaces, a strided copy of the window + encode_frames.

    python profiles/wenc_bench.py [--rounds 3] [--seconds 0.6] [--only mixed4k|noise4k|u16] [--out profiles/wenc_bench.jsonl]

Datasets (device-made images, never copied to the host): 1,024 mixed and 1,024 noise8 4096x3072 U8 images, and 128 U16
images of 4096x3072 with a per-tile depth uniform in 0..16 (profiles/roi16_bench.py's).  Cases: windows of 256x256,
1024x1024 and 2045x2043 at (1003, 697) of every image, the full frame of the same images held at a pitch of 4096 + 64
pixels, and one frame per call at 512x512.  Arms, timed with device events over repeated calls (at least --seconds of
work per figure, after a warm-up), alternated round by round so that the spread shows:
  a  encode_window on the strided view
  b  copy_ of the sliced view into a preallocated contiguous tensor, then encode_frames (the path a replaces)
  c  encode_frames alone on the contiguous copy (the floor)
  d  the strided copy alone
Prints one JSON line per (dataset, case, arm, round):
  ms             time of one call
  bytes          bytes the arm must move at least: P = the window's pixels, S = the packed bytes (from the reported
                 sizes): a and c P + S, b 3 P + S, d 2 P
  share_of_peak  bytes / time against 8 TB/s
Arm a is checked once against arm b's bytes before any timing.
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12
W, H, PAD = 4096, 3072, 64
CASES = [("256x256", 1003, 697, 256, 256, None, False), ("1024x1024", 1003, 697, 1024, 1024, None, False),
         ("2045x2043", 1003, 697, 2045, 2043, None, False), ("full at pitch 4160", 0, 0, W, H, None, True),
         ("512x512 one frame", 1003, 697, 512, 512, 1, False)]


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


def images8(codec, content, n, pitch):
    """(n, H, W) view of n synthetic images held at `pitch` pixels a row."""
    import torch
    store = torch.empty((n, H, pitch), dtype=torch.uint8, device="cuda")
    step = 16
    for f0 in range(0, n, step):
        k = min(step, n - f0)
        store[f0:f0 + k, :, :W].copy_(codec.synth_frames(content, 0xDBDE2016, f0, k, W, H))
    return store[:, :, :W]


def images16(n, pitch):
    import torch
    w, h = W // 8, H // 8
    g = torch.Generator(device="cuda").manual_seed(1)
    store = torch.empty((n, H, pitch), dtype=torch.int16, device="cuda")
    for f0 in range(0, n, 16):   # in groups: the generator's temporaries are 64-bit
        k = min(16, n - f0)
        d = torch.randint(0, 17, (k, h, w), device="cuda", generator=g)
        dd = d.repeat_interleave(8, 1).repeat_interleave(8, 2)
        mask = (torch.ones_like(dd) << dd) - 1
        noise = torch.randint(0, 65536, (k, H, W), device="cuda", generator=g) & mask
        base = torch.randint(0, 32768, (k, h, w), device="cuda", generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2)
        store[f0:f0 + k, :, :W].copy_(torch.minimum(base, 65535 - mask).add_(noise).to(torch.int32).to(torch.int16))
        del d, dd, mask, noise, base
    return store[:, :, :W]


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
    lines = []
    for name, content, bits, n_all in (("mixed4k", "mixed", 8, 1024), ("noise4k", "noise8", 8, 1024), ("u16", "u16", 16, 128)):
        if a.only and name != a.only:
            continue
        pix = bits // 8
        dtype = torch.uint8 if bits == 8 else torch.int16
        make = (lambda p: images8(codec, content, n_all, p)) if bits == 8 else (lambda p: images16(n_all, p))
        sources = {False: make(W), True: None}
        wenc = codec.encode_window if bits == 8 else codec.encode_window16
        maxf = dv.max_frame_bytes if bits == 8 else (lambda rw, rh: int(codec.L.dbde16_hip_max_frame_bytes(rw, rh)))
        for case, x, y, rw, rh, nf, pitched in CASES:
            if pitched and sources[True] is None:
                sources[True] = make(W + PAD)
                sources[True].copy_(sources[False])   # the same images at the padded pitch
            n = nf or n_all
            view = sources[pitched][:n, y:y + rh, x:x + rw]
            cap = n * maxf(rw, rh)
            out_a = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
            out_b = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
            win = torch.empty((n, rh, rw), dtype=dtype, device="cuda")
            oa, sa = torch.empty(n, dtype=torch.int64, device="cuda"), torch.empty(n, dtype=torch.int64, device="cuda")
            ob, sb = torch.empty_like(oa), torch.empty_like(sa)

            def arm_a():
                wenc(view, out_a, 32, cap, offsets=oa, nbytes=sa)

            def arm_d():
                win.copy_(view)

            def arm_c():
                if bits == 8:
                    codec.encode_frames(win, rw, rh, n, out_b, 32, cap, offsets=ob, nbytes=sb)
                else:
                    codec.encode_frames16(win, rw, rh, n, out_b, 32, cap)

            def arm_b():
                arm_d()
                arm_c()

            arm_a()
            codec.sync()
            total = int((oa[-1] + sa[-1]).item())
            arm_b()
            codec.sync()
            assert torch.equal(out_a[32:32 + total], out_b[32:32 + total]), (name, case)
            P = n * rw * rh * pix
            moved = {"a": P + total, "b": 3 * P + total, "c": P + total, "d": 2 * P}
            pl = (dv.window_encode_plan if bits == 8 else dv.window_encode16_plan)(
                W, H, n, x, y, rw, rh, pitch=view.stride(-2) * pix, frame_stride=view.stride(0) * pix)
            arms = [("a encode_window", arm_a), ("b strided copy + encode_frames", arm_b),
                    ("c encode_frames of the contiguous copy", arm_c), ("d strided copy", arm_d)]
            for _, fn in arms:   # warm-up
                fn()
            codec.sync()
            for rnd in range(a.rounds):
                order = arms if rnd % 2 == 0 else arms[::-1]
                for arm, fn in order:
                    ms, reps = timed(fn, a.seconds)
                    k = arm[0]
                    ln = dict(dataset=name, content=content, bits=bits, W=W, H=H, pitch=view.stride(-2) * pix, frames=n,
                              case=case, window=[x, y, rw, rh], chunks_per_frame=pl["chunks_per_frame"], grid=pl["grid"],
                              arm=arm, round=rnd, reps=reps, ms=ms, window_bytes=P, packed_bytes=total, bytes=moved[k],
                              share_of_peak=moved[k] / (ms * 1e-3) / PEAK, measured=True)
                    print(json.dumps(ln), flush=True)
                    lines.append(ln)
            del out_a, out_b, win, view
            torch.cuda.empty_cache()
        del sources
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    codec.close()


if __name__ == "__main__":
    main()
