"""Weighted temporal projection (R regressor maps per pixel in one pass over the compressed stream) against the nearest
existing kernel and against the only route there was without it.

    python profiles/wproject_bench.py [--only mixed4k|small|u16] [--frames N] [--steps 20] [--warmup 3] [--out FILE]

Datasets: 1,024 mixed 4096x3072 frames (synth), 65,536 mixed 64x64 frames, 128 DBDE16 4096x3072 frames (16, 12, 8 and 4
significant bits, frame by frame).  Cases: the full frame and a 1024x1024 window with R = 1, 2, 4 and 8, a 256x256
window, one frame per call, the small frames and the DBDE16 frames.  Every arm of a case runs in this process on the same
inputs, `warmup` untimed calls and then `steps` timed ones between device events on the context's stream, the arms
interleaved call by call; the median is reported.  Arms:
  w      project_weighted with standard normal weights (the timed output);
  ones   project_weighted with R = 1 and all-ones weights: like for like with arm a;
  a      project(stats=("sum",)), the nearest existing kernel;
  b      decode_frames in chunks that fit memory, `.float()`, and weights @ frames.flatten(1) accumulated in torch (for a
         window: the same on the slice of the decoded frames); b_roi: decode_roi of the window in place of decode_frames.
One JSON line per case with the medians, the ratios, the plan's segments, the timing hook's split of arm w into index
and projection kernels, and the check: the timed output against a one_segment run of the same inputs within the
reassociation bound of the F32 chains, |diff| <= 2 n 2^-24 sum_f |w_f| p_max (derived: each of at most n additions of
either order rounds by at most 2^-24 of a partial sum that never exceeds sum_f |w_f| p_max; not tuned).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(arms, steps, warmup):
    """{name: fn} -> {name: median ms}; the arms alternate call by call, each between its own pair of events."""
    import torch
    for _ in range(warmup):
        for fn in arms.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(steps):
        for k, fn in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: float(np.median(v)) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, help="one dataset: mixed4k, small or u16")
    ap.add_argument("--frames", type=int, default=0, help="frames per dataset (default 1024; small: 65536; u16: 128)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    import torch
    import dbde_video_cpp_amd as dv

    codec = dv.Codec(0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    g = torch.Generator(device="cuda").manual_seed(2016)

    def emit(line):
        print(json.dumps(line), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")

    for name, pix, W, H, n_all in (("mixed4k", 1, 4096, 3072, 1024), ("small", 1, 64, 64, 65536), ("u16", 2, 4096, 3072, 128)):
        if a.only and a.only != name:
            continue
        n_all = a.frames or n_all
        maxf = dv.max_frame_bytes(W, H) if pix == 1 else int(codec.L.dbde16_hip_max_frame_bytes(W, H))
        slot = (maxf + 255) // 256 * 256
        buf = torch.empty(n_all * slot + 256, dtype=torch.uint8, device="cuda")
        offs = torch.empty(n_all, dtype=torch.int64, device="cuda")
        step = min(16 if W > 64 else 4096, n_all)
        for f0 in range(0, n_all, step):   # synthesize and encode in groups (the images of the whole batch need not fit)
            k = min(step, n_all - f0)
            if pix == 1:
                imgs = codec.synth_frames("mixed", 0xDBDE2016, f0, k, W, H)
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
        pmax = 255 if pix == 1 else 65535
        wproj = codec.project_weighted if pix == 1 else codec.project_weighted16
        proj = codec.project if pix == 1 else codec.project16
        frames_fn = codec.decode_frames if pix == 1 else codec.decode_frames16
        roi_fn = codec.decode_roi if pix == 1 else codec.decode_roi16
        plan_fn = dv.wproject_plan if pix == 1 else dv.wproject16_plan
        chunk = max(1, min(n_all, (1 << 28) // (W * H)))   # frames per chunk of arm b: at most 2^28 pixels, 1 GiB as F32
        full = torch.empty((chunk, H, W), dtype=pdt, device="cuda")
        res = torch.empty((n_all, 4), dtype=torch.int64, device="cuda")
        wall = torch.randn((8, n_all), dtype=torch.float32, device="cuda", generator=g)
        ones = torch.ones((1, n_all), dtype=torch.float32, device="cuda")

        if name == "mixed4k":
            cases = [(n_all, win, R) for win in ((0, 0, W, H), (1536, 1024, 1024, 1024)) for R in (1, 2, 4, 8)]
            cases += [(n_all, (1920, 1408, 256, 256), R) for R in (1, 8)]
            cases += [(1, (0, 0, W, H), R) for R in (1, 4, 8)]
        elif name == "small":
            cases = [(n_all, (0, 0, W, H), R) for R in (1, 4, 8)]
        else:
            cases = [(n_all, (0, 0, W, H), R) for R in (1, 4, 8)]
        for nf, (x, y, rw, rh), R in cases:
            w = wall[:R, :nf]
            o_f, r_f = offs[:nf], res[:nf]
            out = dv.WeightedProjection.empty(R, rh, rw, codec.device)
            out1 = dv.WeightedProjection.empty(1, rh, rw, codec.device)
            pr = dv.Projection.empty(rh, rw, ("sum",), codec.device, pix=pix)
            acc = torch.empty((R, rh * rw), dtype=torch.float32, device="cuda")
            window = (x, y, rw, rh) != (0, 0, W, H)
            roi = torch.empty((min(chunk * ((W * H) // (rw * rh)), nf), rh, rw), dtype=pdt, device="cuda") if window else None

            def as_float(t):
                return t.float() if pix == 1 else (t.to(torch.int32) & 0xFFFF).float()

            def arm_w():
                wproj(buf, 0, stream_bytes, o_f, W, H, nf, w, x, y, rw, rh, out=out, results=r_f)

            def arm_ones():
                wproj(buf, 0, stream_bytes, o_f, W, H, nf, ones[:, :nf], x, y, rw, rh, out=out1, results=r_f)

            def arm_a():
                proj(buf, 0, stream_bytes, o_f, W, H, nf, x, y, rw, rh, out=pr, results=r_f)

            def arm_b():
                acc.zero_()
                for f0 in range(0, nf, chunk):
                    k = min(chunk, nf - f0)
                    kw = dict(results=r_f[f0:f0 + k]) if pix == 1 else {}
                    frames_fn(buf, 0, stream_bytes, o_f[f0:f0 + k], W, H, k, images=full[:k], **kw)
                    acc.addmm_(w[:, f0:f0 + k], as_float(full[:k, y:y + rh, x:x + rw]).flatten(1))

            def arm_b_roi():
                acc.zero_()
                for f0 in range(0, nf, roi.shape[0]):
                    k = min(roi.shape[0], nf - f0)
                    roi_fn(buf, 0, stream_bytes, o_f[f0:f0 + k], W, H, k, x, y, rw, rh, out=roi[:k], results=r_f[f0:f0 + k])
                    acc.addmm_(w[:, f0:f0 + k], as_float(roi[:k]).flatten(1))

            arms = dict(w=arm_w, ones=arm_ones, a=arm_a, b=arm_b)
            if window:
                arms["b_roi"] = arm_b_roi
            ms = timed(arms, a.steps, a.warmup)
            codec.timing(True)
            codec.timing_read(reset=True)
            for _ in range(a.steps):
                arm_w()
            codec.sync()
            t = codec.timing_read(reset=True)
            codec.timing(False)

            # the timed output against the one_segment chain, within the reassociation bound (asserted); the distance
            # to arm b's sum, whose order is torch's, is reported
            arm_w()
            one, _ = wproj(buf, 0, stream_bytes, o_f, W, H, nf, w, x, y, rw, rh, one_segment=True)
            arm_b()
            codec.sync()
            bound = 2.0 * nf * 2.0 ** -24 * w.abs().to(torch.float64).sum(1) * pmax
            diff = (out.out.to(torch.float64) - one.out.to(torch.float64)).abs().flatten(1).amax(1)
            diff_b = (out.out.to(torch.float64).flatten(1) - acc.to(torch.float64)).abs().amax(1)
            assert bool((diff <= bound).all()), (diff.tolist(), bound.tolist())
            p = plan_fn(W, H, nf, x, y, rw, rh, regressors=R, n_cu=cus)
            line = dict(dataset=name, W=W, H=H, frames_per_call=nf, window=[x, y, rw, rh], R=R, segments=p["segments"],
                        ms_weighted=ms["w"], ms_weighted_ones_r1=ms["ones"], ms_project_sum=ms["a"],
                        ms_frames_matmul=ms["b"], weighted_over_project_sum=ms["w"] / ms["a"],
                        ones_r1_over_project_sum=ms["ones"] / ms["a"], frames_matmul_over_weighted=ms["b"] / ms["w"],
                        ms_index=t["decode_index"][0] / a.steps, ms_kernels=t["decode"][0] / a.steps,
                        max_diff_vs_one_segment=float(diff.max()), max_diff_vs_matmul=float(diff_b.max()),
                        bound_min=float(bound.min()), matmul_within_bound=bool((diff_b <= bound).all()))
            if window:
                line["ms_roi_matmul"] = ms["b_roi"]
                line["roi_matmul_over_weighted"] = ms["b_roi"] / ms["w"]
            emit(line)
            del out, out1, pr, acc, roi, one
        del buf, full, wall
    codec.close()


if __name__ == "__main__":
    main()
