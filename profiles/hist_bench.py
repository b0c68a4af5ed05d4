"""Per-frame histograms (dbde_hip_histogram) against decoding the batch and binning the images in torch;
profiles/project_bench.py's method.

    python profiles/hist_bench.py [--rounds 3] [--seconds 0.6] [--out profiles/hist_bench.jsonl]

Datasets (encoded on the device, one slot per frame): 1,024 4096x3072 frames each of mixed, noise8 and smooth
content, and 128 4096x3072 DBDE16 frames with per-tile depths uniform in 0..16 (project16_bench.py's mixed16).
Arms, timed with device events over repeated calls (at least --seconds of work per figure, after a warm-up),
alternated round by round so that the spread shows:
  a  decode_frames alone
  b  decode_frames + one torch.bincount per frame (256 bins)
  c  histogram, full frame, 256 bins per frame
  d  histogram of a 256x256 window at (1001, 999)
  e  decode_roi of that window
  DBDE16: a decode_frames16, b decode_frames16 + torch.bincount of v >> 4 per frame, f histogram16, 4096 bins, shift 4.
Prints one JSON line per (dataset, arm, round): ms per call and reps.  Every histogram is checked once against the
torch bincounts of the decoded frames before any timing.
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))

WIN = (1001, 999, 256, 256)


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


def encode(codec, dv, content, W, H, n, pix):
    import torch
    from project16_bench import frames16
    maxf = dv.max_frame_bytes(W, H) if pix == 1 else int(codec.L.dbde16_hip_max_frame_bytes(W, H))
    slot = (maxf + 255) // 256 * 256
    buf = torch.empty(n * slot + 256, dtype=torch.uint8, device="cuda")
    offs = torch.empty(n, dtype=torch.int64, device="cuda")
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0xDBDE)
    step = max(1, min(n, (1 << 28 if pix == 1 else 1 << 26) // (W * H)))
    for f0 in range(0, n, step):
        k = min(step, n - f0)
        if pix == 1:
            imgs = codec.synth_frames(content, 0xDBDE2016, f0, k, W, H)
            o, _ = codec.encode_frames(imgs, W, H, k, buf, f0 * slot, (n - f0) * slot, first_index=f0, slot_stride=slot)
        else:
            imgs = frames16(content, k, W, H, gen)
            o, _ = codec.encode_frames16(imgs, W, H, k, buf, f0 * slot, (n - f0) * slot, first_index=f0,
                                         slot_stride=slot)
        offs[f0:f0 + k] = o + f0 * slot
        del imgs
    codec.sync()
    return buf, offs, n * slot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.6)
    ap.add_argument("--only", default=None, help="one dataset: mixed4k, noise4k, smooth4k or mixed16_4k")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    import torch
    import dbde_video_cpp_amd as dv

    codec = dv.Codec(0)
    datasets = [("mixed4k", "mixed", 4096, 3072, 1024, 1), ("noise4k", "noise8", 4096, 3072, 1024, 1),
                ("smooth4k", "smooth", 4096, 3072, 1024, 1), ("mixed16_4k", "mixed16", 4096, 3072, 128, 2)]
    lines = []
    for name, content, W, H, n, pix in datasets:
        if a.only and name != a.only:
            continue
        buf, offs, stream_bytes = encode(codec, dv, content, W, H, n, pix)
        images = torch.empty((n, H, W), dtype=torch.uint8 if pix == 1 else torch.int16, device="cuda")
        res = torch.empty((n, 4), dtype=torch.int64, device="cuda")
        shift, bins = (0, 256) if pix == 1 else (4, 4096)
        ref = torch.zeros((n, bins), dtype=torch.int64, device="cuda")

        def decode():
            if pix == 1:
                codec.decode_frames(buf, 0, stream_bytes, offs, W, H, n, images=images, results=res)
            else:
                codec.decode_frames16(buf, 0, stream_bytes, offs, W, H, n, images=images)

        def decode_bincount():
            decode()
            for f in range(n):
                v = images[f].reshape(-1)
                v = v.to(torch.int64) if pix == 1 else (v.to(torch.int64) & 0xFFFF) >> shift
                ref[f] = torch.bincount(v, minlength=bins)

        full = dv.Histograms.empty(n, bins, "cuda", shift=shift)
        arms = [("a decode_frames", decode), ("b decode_frames + torch.bincount per frame", decode_bincount)]
        if pix == 1:
            x, y, rw, rh = WIN
            win = dv.Histograms.empty(n, bins, "cuda")
            roi = torch.empty((n, rh, rw), dtype=torch.uint8, device="cuda")
            arms += [("c histogram full frame", lambda: codec.histogram(buf, 0, stream_bytes, offs, W, H, n, out=full,
                                                                        results=res)),
                     ("d histogram 256x256 window", lambda: codec.histogram(buf, 0, stream_bytes, offs, W, H, n, *WIN,
                                                                            out=win, results=res)),
                     ("e decode_roi 256x256 window", lambda: codec.decode_roi(buf, 0, stream_bytes, offs, W, H, n, *WIN,
                                                                              out=roi, results=res))]
        else:
            arms += [("f histogram16 4096 bins shift 4", lambda: codec.histogram16(buf, 0, stream_bytes, offs, W, H, n,
                                                                                   shift=4, bins=4096, out=full))]
        # check once against the torch bincounts
        decode_bincount()
        for _, fn in arms[2:]:
            fn()
        codec.sync()
        assert torch.equal(full.counts.to(torch.int64), ref), name
        if pix == 1:
            wref = torch.stack([torch.bincount(images[f, y:y + rh, x:x + rw].reshape(-1).to(torch.int64), minlength=256)
                                for f in range(n)])
            assert torch.equal(win.counts.to(torch.int64), wref), name
        for _, fn in arms:   # warm-up
            fn()
        codec.sync()
        for rnd in range(a.rounds):
            order = arms if rnd % 2 == 0 else arms[::-1]
            for arm, fn in order:
                ms, reps = timed(fn, a.seconds)
                ln = dict(dataset=name, content=content, W=W, H=H, frames=n, arm=arm, round=rnd, reps=reps, ms=ms,
                          measured=True)
                print(json.dumps(ln), flush=True)
                lines.append(ln)
        del buf, images, ref, full
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    codec.close()


if __name__ == "__main__":
    main()
