"""Patch decode (K small windows per frame in one call) against the two ways to get the same patches without it.

    python profiles/patch_bench.py [--only mixed4k|u16|small] [--frames N] [--steps 7] [--warmup 2] [--out FILE]

Datasets: 1,024 mixed 4096x3072 frames (synth), 128 DBDE16 4096x3072 frames (16, 12, 8 and 4 significant bits, frame by
frame), 1,024 mixed 512x512 frames.  For each: patches of 16x16, 32x32, 64x64 and 128x128, K = 1, 8, 64 and 512 per
frame at uniformly random origins inside the frame; one frame per call with K = 64; FILL mode with a quarter of the
patches straddling a frame edge.  (512x512 frames: 64 patches of 32x32 only.)  Timed with device events around each of
`steps` calls after `warmup` untimed ones, the median reported.  Arms, all in this build:
  a  one decode_patches call (CLAMP unless the case says fill);
  b  K decode_roi calls with origins[:, k], plus the permute of the (K, n, ph, pw) stack into (n, K, ph, pw);
  c  decode_frames of the whole batch plus a torch advanced-indexing gather of the patches (only where the gather's
     index arithmetic stays below 2^27 pixels: torch materialises int64 indices of the output's size).
One JSON line per case: ms_patches, ms_roi_calls, ms_roi_one (ONE decode_roi call, the K = 1 comparison), ms_frames_gather
(ms_frames + ms_gather), the ratios b / a and c / a, and the timing hook's split of arm a into index and patch kernel.
Arm a's output is checked against arm b's once per case.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GATHER_LIMIT = 1 << 27


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, help="one dataset: mixed4k, u16 or small")
    ap.add_argument("--frames", type=int, default=0, help="frames per dataset (default 1024; u16: 128)")
    ap.add_argument("--steps", type=int, default=7)
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

    for name, content, pix, W, H, n_all in (("mixed4k", "mixed", 1, 4096, 3072, 1024), ("u16", "u16", 2, 4096, 3072, 128),
                                            ("small", "mixed", 1, 512, 512, 1024)):
        if a.only and a.only != name:
            continue
        n_all = a.frames or n_all
        maxf = dv.max_frame_bytes(W, H) if pix == 1 else int(codec.L.dbde16_hip_max_frame_bytes(W, H))
        slot = (maxf + 255) // 256 * 256
        buf = torch.empty(n_all * slot + 256, dtype=torch.uint8, device="cuda")
        offs = torch.empty(n_all, dtype=torch.int64, device="cuda")
        step = min(16, n_all)
        for f0 in range(0, n_all, step):   # synthesize and encode in groups (the images of the whole batch need not fit)
            k = min(step, n_all - f0)
            if pix == 1:
                imgs = codec.synth_frames(content, 0xDBDE2016, f0, k, W, H)
                o, _ = codec.encode_frames(imgs, W, H, k, buf, f0 * slot, (n_all - f0) * slot, first_index=f0,
                                           slot_stride=slot)
            else:
                imgs = torch.randint(-32768, 32768, (k, H, W), dtype=torch.int16, device="cuda", generator=g)
                for j in range(k):   # 16, 12, 8 and 4 significant bits, frame by frame
                    imgs[j] = ((imgs[j].to(torch.int32) & 0xFFFF) >> (4 * (j % 4))).to(torch.int16)
                o, _ = codec.encode_frames16(imgs, W, H, k, buf, f0 * slot, (n_all - f0) * slot, first_index=f0,
                                             slot_stride=slot)
            offs[f0:f0 + k] = o + f0 * slot
            del imgs
        codec.sync()
        stream_bytes = n_all * slot
        pdt = torch.uint8 if pix == 1 else torch.int16
        patches_fn = codec.decode_patches if pix == 1 else codec.decode_patches16
        roi_fn = codec.decode_roi if pix == 1 else codec.decode_roi16
        frames_fn = codec.decode_frames if pix == 1 else codec.decode_frames16
        res = torch.empty((n_all, 4), dtype=torch.int64, device="cuda")
        full = torch.empty((n_all, H, W), dtype=pdt, device="cuda")
        ms_frames = {}
        for nf in (n_all, 1):
            kw = dict(results=res[:nf]) if pix == 1 else {}   # (decode_frames16 allocates its results)
            ms_frames[nf] = timed(lambda: frames_fn(buf, 0, stream_bytes, offs[:nf], W, H, nf, images=full[:nf], **kw),
                                  a.steps, a.warmup)

        if name == "small":
            cases = [(n_all, 32, 64, "clamp"), (n_all, 32, 64, "fill"), (1, 32, 64, "clamp")]
        else:
            cases = [(n_all, p, K, "clamp") for p in (16, 32, 64, 128) for K in (1, 8, 64, 512)]
            cases += [(1, p, 64, "clamp") for p in (16, 32, 64, 128)]
            cases += [(n_all, 32, K, "fill") for K in (8, 64, 512)]
        for nf, p, K, edge in cases:
            ox = rng.integers(0, W - p + 1, (nf, K))
            oy = rng.integers(0, H - p + 1, (nf, K))
            if edge == "fill":   # a quarter of the patches straddle an edge
                q = rng.random((nf, K)) < 0.25
                side = rng.integers(0, 4, (nf, K))
                cut = rng.integers(1, p, (nf, K))
                ox = np.where(q & (side == 0), -cut, np.where(q & (side == 1), W - cut, ox))
                oy = np.where(q & (side == 2), -cut, np.where(q & (side == 3), H - cut, oy))
            org = torch.from_numpy(np.stack([ox, oy], -1).astype(np.int32)).cuda()
            org_k = org.permute(1, 0, 2).contiguous()   # (K, nf, 2): one decode_roi call's origins each
            out = torch.empty((nf, K, p, p), dtype=pdt, device="cuda")
            stack = torch.empty((K, nf, p, p), dtype=pdt, device="cuda")
            o_f, r_f = offs[:nf], res[:nf]

            def arm_a():
                patches_fn(buf, 0, stream_bytes, o_f, W, H, nf, p, p, org, edge=edge, fill=0, out=out, results=r_f)

            def arm_b():
                for k in range(K):
                    roi_fn(buf, 0, stream_bytes, o_f, W, H, nf, 0, 0, p, p, origins=org_k[k], out=stack[k], results=r_f)
                return stack.permute(1, 0, 2, 3).contiguous()

            def roi_one():
                roi_fn(buf, 0, stream_bytes, o_f, W, H, nf, 0, 0, p, p, origins=org_k[0], out=stack[0], results=r_f)

            ms_a = timed(arm_a, a.steps, a.warmup)
            codec.timing(True)
            codec.timing_read(reset=True)
            for _ in range(a.steps):
                arm_a()
            codec.sync()
            t = codec.timing_read(reset=True)
            codec.timing(False)
            line = dict(dataset=name, W=W, H=H, frames_per_call=nf, patch=p, K=K, edge=edge, ms_patches=ms_a,
                        ms_index=t["decode_index"][0] / a.steps, ms_patch_kernel=t["decode"][0] / a.steps)
            if edge == "clamp":
                line["ms_roi_calls"] = timed(arm_b, a.steps, a.warmup)
                line["ms_roi_one"] = timed(roi_one, a.steps, a.warmup)
                line["roi_calls_over_patches"] = line["ms_roi_calls"] / ms_a
                assert torch.equal(arm_b(), out), "decode_patches differs from K decode_roi calls"
            if nf * K * p * p <= GATHER_LIMIT:
                ar = torch.arange(p, device="cuda")
                fi = torch.arange(nf, device="cuda")[:, None, None, None]
                o64 = org.to(torch.int64)
                if edge == "fill":   # (the gather's own fill: clamp the index, then mask)
                    def gather():
                        yy, xx = o64[:, :, 1, None, None] + ar[:, None], o64[:, :, 0, None, None] + ar[None, :]
                        inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
                        return torch.where(inside, full[fi, yy.clamp(0, H - 1), xx.clamp(0, W - 1)], torch.zeros((), dtype=pdt, device="cuda"))
                else:
                    def gather():
                        return full[fi, o64[:, :, 1, None, None] + ar[:, None], o64[:, :, 0, None, None] + ar[None, :]]
                line["ms_frames"] = ms_frames[nf]
                line["ms_gather"] = timed(gather, a.steps, a.warmup)
                line["ms_frames_gather"] = line["ms_frames"] + line["ms_gather"]
                line["frames_gather_over_patches"] = line["ms_frames_gather"] / ms_a
                assert torch.equal(gather(), out), "decode_patches differs from the gather"
            emit(line)
            del out, stack
        del buf, full
    codec.close()


if __name__ == "__main__":
    main()
