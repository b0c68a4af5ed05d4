"""Patch moments (eight thresholded sums per tracked window, straight from the stream) against decoding the patches.

    python profiles/moments_bench.py [--only mixed4k|u16|small|tracker] [--frames N] [--steps 5] [--warmup 2] [--out FILE]

Datasets: 1,024 mixed 4096x3072 frames (synth), 128 DBDE16 4096x3072 frames (16, 12, 8 and 4 significant bits, frame by
frame), 1,024 mixed 512x512 frames, and "tracker": 256 frames of 4096x3072 with 512 bright discs (radius 5, value 200) on
a dark level of 16..23, the patches centred on the discs (so that most tiles of a patch lie below the band and the
header shortcut shows next to mixed content, where it rarely applies).  For each: patches of 16x16, 32x32, 64x64 and
128x128, K = 1, 8, 64 and 512 per frame (mixed4k, u16, small: uniformly random origins inside the frame), and one frame
per call with K = 64.  Band and weight: [128, 255] (u16: [1000, 65535]; tracker: [64, 255]), weight "above".  Timed
with device events around each of `steps` calls after `warmup` untimed ones, the median reported.  Arms, all in this
build:
  a  one patch_moments call (CLAMP);
  b  decode_patches plus the same eight sums in torch (int64), in runs of frames of at most 2^26 patch pixels (torch
     holds several int64 temporaries of the patches' size);
  c  decode_patches alone, the floor arm a should approach or beat since it writes 64 bytes a patch and no pixel.
One JSON line per case: ms_moments, ms_patches_torch, ms_patches, the ratios b / a and c / a, and the timing hook's split
of arm a into index and moments kernel.  Arm a's sums are checked against arm b's once per case.
The lines are printed; they are also appended to FILE only with --out.  profiles/moments_bench.jsonl was written by
    python profiles/moments_bench.py --steps 3 --warmup 1 --out profiles/moments_bench.jsonl
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TORCH_LIMIT = 1 << 26


def timed(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def torch_sums(v, lo, hi):
    """The eight sums of patches v (n, K, p, p) int64, weight "above", as (n, K, 8) int64."""
    import torch
    p = v.shape[-1]
    sel = (v >= lo) & (v <= hi)
    w = torch.where(sel, v - lo, torch.zeros((), dtype=torch.int64, device=v.device))
    j = torch.arange(p, device=v.device, dtype=torch.int64)
    i = j[:, None]
    wj, wi = w * j, w * i
    parts = (sel.to(torch.int64), w, wj, wi, wj * j, wj * i, wi * i, w * w)
    return torch.stack([t.sum(dim=(2, 3)) for t in parts], dim=-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, help="one dataset: mixed4k, u16, small or tracker")
    ap.add_argument("--frames", type=int, default=0, help="frames per dataset (default 1024; u16: 128; tracker: 256)")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    import torch
    import dbde_video_cpp_amd as dv

    codec = dv.Codec(0)
    g = torch.Generator(device="cuda").manual_seed(2016)
    rng = np.random.default_rng(2016)

    def emit(line):
        print(json.dumps(line), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")

    disc = np.array([(dx, dy) for dy in range(-5, 6) for dx in range(-5, 6) if dx * dx + dy * dy <= 25], np.int64)
    for name, content, pix, W, H, n_all, lo, hi in (("mixed4k", "mixed", 1, 4096, 3072, 1024, 128, 255),
                                                    ("u16", "u16", 2, 4096, 3072, 128, 1000, 65535),
                                                    ("small", "mixed", 1, 512, 512, 1024, 128, 255),
                                                    ("tracker", "tracker", 1, 4096, 3072, 256, 64, 255)):
        if a.only and a.only != name:
            continue
        n_all = a.frames or n_all
        maxf = dv.max_frame_bytes(W, H) if pix == 1 else int(codec.L.dbde16_hip_max_frame_bytes(W, H))
        slot = (maxf + 255) // 256 * 256
        buf = torch.empty(n_all * slot + 256, dtype=torch.uint8, device="cuda")
        offs = torch.empty(n_all, dtype=torch.int64, device="cuda")
        centres = rng.integers(70, (W - 70, H - 70), (n_all, 512, 2)) if content == "tracker" else None
        step = min(16, n_all)
        for f0 in range(0, n_all, step):   # synthesize and encode in groups (the images of the whole batch need not fit)
            k = min(step, n_all - f0)
            if content == "tracker":
                imgs = torch.randint(16, 24, (k, H, W), dtype=torch.uint8, device="cuda", generator=g)
                c = torch.from_numpy(centres[f0:f0 + k]).cuda()               # (k, 512, 2)
                d = torch.from_numpy(disc).cuda()                              # (81, 2)
                fi = torch.arange(k, device="cuda")[:, None, None]
                imgs[fi, c[:, :, 1, None] + d[None, None, :, 1], c[:, :, 0, None] + d[None, None, :, 0]] = 200
                o, _ = codec.encode_frames(imgs, W, H, k, buf, f0 * slot, (n_all - f0) * slot, first_index=f0, slot_stride=slot)
            elif pix == 1:
                imgs = codec.synth_frames(content, 0xDBDE2016, f0, k, W, H)
                o, _ = codec.encode_frames(imgs, W, H, k, buf, f0 * slot, (n_all - f0) * slot, first_index=f0, slot_stride=slot)
            else:
                imgs = torch.randint(-32768, 32768, (k, H, W), dtype=torch.int16, device="cuda", generator=g)
                for j in range(k):   # 16, 12, 8 and 4 significant bits, frame by frame
                    imgs[j] = ((imgs[j].to(torch.int32) & 0xFFFF) >> (4 * (j % 4))).to(torch.int16)
                o, _ = codec.encode_frames16(imgs, W, H, k, buf, f0 * slot, (n_all - f0) * slot, first_index=f0, slot_stride=slot)
            offs[f0:f0 + k] = o + f0 * slot
            del imgs
        codec.sync()
        stream_bytes = n_all * slot
        pdt = torch.uint8 if pix == 1 else torch.int16
        moments_fn = codec.patch_moments if pix == 1 else codec.patch_moments16
        patches_fn = codec.decode_patches if pix == 1 else codec.decode_patches16
        res = torch.empty((n_all, 4), dtype=torch.int64, device="cuda")

        cases = [(n_all, p, K) for p in (16, 32, 64, 128) for K in (1, 8, 64, 512)]
        cases += [(1, p, 64) for p in (16, 32, 64, 128)]
        for nf, p, K in cases:
            if content == "tracker":   # the patches follow the discs
                org_h = centres[:nf, :K] - p // 2
            else:
                org_h = np.stack([rng.integers(0, W - p + 1, (nf, K)), rng.integers(0, H - p + 1, (nf, K))], -1)
            org = torch.from_numpy(org_h.astype(np.int32)).cuda()
            mom = torch.empty((nf, K, 8), dtype=torch.int64, device="cuda")
            used = torch.empty((nf, K, 2), dtype=torch.int32, device="cuda")
            run = max(1, min(nf, TORCH_LIMIT // (K * p * p)))   # frames per run of arm b
            out = torch.empty((nf, K, p, p), dtype=pdt, device="cuda")
            sums = torch.empty((nf, K, 8), dtype=torch.int64, device="cuda")
            o_f, r_f = offs[:nf], res[:nf]

            def arm_a():
                moments_fn(buf, 0, stream_bytes, o_f, W, H, nf, p, p, org, lo, hi, weight="above", out=mom, used=used,
                           results=r_f)

            def arm_c():
                patches_fn(buf, 0, stream_bytes, o_f, W, H, nf, p, p, org, out=out, results=r_f)

            def arm_b():
                for f0 in range(0, nf, run):
                    f1 = min(nf, f0 + run)
                    patches_fn(buf, 0, stream_bytes, offs[f0:f1], W, H, f1 - f0, p, p, org[f0:f1], out=out[f0:f1],
                               results=res[f0:f1])
                    v = out[f0:f1].to(torch.int64)
                    if pix == 2:
                        v = v & 0xFFFF
                    sums[f0:f1] = torch_sums(v, lo, hi)

            ms_a = timed(arm_a, a.steps, a.warmup)
            codec.timing(True)
            codec.timing_read(reset=True)
            for _ in range(a.steps):
                arm_a()
            codec.sync()
            t = codec.timing_read(reset=True)
            codec.timing(False)
            ms_c = timed(arm_c, a.steps, a.warmup)
            ms_b = timed(arm_b, a.steps, a.warmup)
            assert torch.equal(mom, sums), "patch_moments differs from decode_patches plus the sums in torch"
            emit(dict(dataset=name, W=W, H=H, frames_per_call=nf, patch=p, K=K, lo=lo, hi=hi, ms_moments=ms_a,
                      ms_index=t["decode_index"][0] / a.steps, ms_moments_kernel=t["decode"][0] / a.steps,
                      ms_patches_torch=ms_b, ms_patches=ms_c, patches_torch_over_moments=ms_b / ms_a,
                      patches_over_moments=ms_c / ms_a, selected_fraction=float(mom[..., 0].sum().item()) / (nf * K * p * p)))
            del out, sums, mom
        del buf
    codec.close()


if __name__ == "__main__":
    main()
