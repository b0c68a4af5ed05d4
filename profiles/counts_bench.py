"""Count projection (K per-pixel counts of frames at or below a threshold, in one pass over the compressed stream) and
the exact temporal median built on it, against the nearest existing kernels and the only route there was without them.

    python profiles/counts_bench.py [--only mixed4k|small|u16|quantile|quantile16] [--frames N] [--steps 20]
                                    [--warmup 3] [--qsteps 5] [--out FILE]

Datasets: 1,024 mixed 4096x3072 frames (synth), 65,536 mixed 64x64 frames, 128 DBDE16 4096x3072 frames (16, 12, 8 and 4
significant bits, frame by frame).  Cases: the full frame, a 1024x1024 and a 256x256 window, one frame per call, the
small frames and the DBDE16 frames, each with K = 1, 3, 7 and 8 levels as scalars and as maps.  Every arm of a case runs
in this process on the same inputs, `warmup` untimed calls and then `steps` timed ones between device events on the
context's stream, the arms interleaved call by call; the median is reported.  Arms:
  k   project_counts (the timed output);
  a   project(stats=("sum",)), the nearest existing kernel;
  b   project_weighted with R = K regressors;
  c   decode_frames in chunks that fit memory and (img <= thr).sum(0) accumulated in torch (for a window: on the slice).
One JSON line per case with the medians, the ratios, the plan's segments, the timing hook's split of arm k into index and
projection kernels, and the check: the timed planes equal arm c's, element for element.

The quantile cases time quantiles.temporal_median (3 passes for DBDE, 6 for DBDE16) against decode_roi of row strips over
all frames plus torch.kthvalue along the frame axis, in the largest strips that keep the decoded pixels near 1 GiB
(kthvalue also returns int64 indices, eight times the pixels); `qsteps` timed runs after one warm-up, peak device memory of
each arm on top of the stream, and the two medians compared for equality.
"""
import argparse
import json
import os
import sys
from importlib import import_module

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
    ap.add_argument("--only", default=None, help="one part: mixed4k, small, u16, quantile or quantile16")
    ap.add_argument("--frames", type=int, default=0, help="frames per dataset (default 1024; small: 65536; u16: 128)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--qsteps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    import torch
    import dbde_video_cpp_amd as dv
    qt = import_module("dbde_video_cpp_amd.quantiles")

    codec = dv.Codec(0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    g = torch.Generator(device="cuda").manual_seed(2016)

    def emit(line):
        print(json.dumps(line), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")

    def dataset(pix, W, H, n_all):
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
        return buf, offs, n_all * slot

    for name, pix, W, H, n_all in (("mixed4k", 1, 4096, 3072, 1024), ("small", 1, 64, 64, 65536), ("u16", 2, 4096, 3072, 128)):
        if a.only and a.only != name:
            continue
        n_all = a.frames or n_all
        buf, offs, stream_bytes = dataset(pix, W, H, n_all)
        pdt = torch.uint8 if pix == 1 else torch.int16
        top = 256 if pix == 1 else 65536
        counts = codec.project_counts if pix == 1 else codec.project_counts16
        wproj = codec.project_weighted if pix == 1 else codec.project_weighted16
        proj = codec.project if pix == 1 else codec.project16
        frames_fn = codec.decode_frames if pix == 1 else codec.decode_frames16
        plan_fn = dv.counts_plan if pix == 1 else dv.counts16_plan
        chunk = max(1, min(n_all, (1 << 28) // (W * H)))   # frames per chunk of arm c: at most 2^28 pixels
        full = torch.empty((chunk, H, W), dtype=pdt, device="cuda")
        res = torch.empty((n_all, 4), dtype=torch.int64, device="cuda")
        wall = torch.randn((8, n_all), dtype=torch.float32, device="cuda", generator=g)

        if name == "mixed4k":
            wins = [(n_all, (0, 0, W, H)), (n_all, (1536, 1024, 1024, 1024)), (n_all, (1920, 1408, 256, 256)),
                    (1, (0, 0, W, H))]
        else:
            wins = [(n_all, (0, 0, W, H))]
        for nf, (x, y, rw, rh) in wins:
            for K in (1, 3, 7, 8):
                for maps in (False, True):
                    tv = torch.randint(0, top, (K, rh, rw) if maps else (K,), device="cuda", generator=g)   # int64 values
                    thr = tv.to(torch.uint8) if pix == 1 else torch.where(tv >= 32768, tv - 65536, tv).to(torch.int16)
                    tcmp = (tv if maps else tv.view(K, 1, 1)).to(torch.int32).unsqueeze(1)                # (K, 1, rh|1, rw|1)
                    w = wall[:K, :nf]
                    o_f, r_f = offs[:nf], res[:nf]
                    out = dv.CountProjection.empty(K, rh, rw, codec.device)
                    wout = dv.WeightedProjection.empty(K, rh, rw, codec.device)
                    pr = dv.Projection.empty(rh, rw, ("sum",), codec.device, pix=pix)
                    acc = torch.empty((K, rh, rw), dtype=torch.int32, device="cuda")

                    def values(t):
                        return t.to(torch.int32) if pix == 1 else t.to(torch.int32) & 0xFFFF

                    def arm_k():
                        counts(buf, 0, stream_bytes, o_f, W, H, nf, thr, x, y, rw, rh, out=out, results=r_f)

                    def arm_a():
                        proj(buf, 0, stream_bytes, o_f, W, H, nf, x, y, rw, rh, out=pr, results=r_f)

                    def arm_b():
                        wproj(buf, 0, stream_bytes, o_f, W, H, nf, w, x, y, rw, rh, out=wout, results=r_f)

                    def arm_c():
                        acc.zero_()
                        for f0 in range(0, nf, chunk):
                            k = min(chunk, nf - f0)
                            kw = dict(results=r_f[f0:f0 + k]) if pix == 1 else {}
                            frames_fn(buf, 0, stream_bytes, o_f[f0:f0 + k], W, H, k, images=full[:k], **kw)
                            px = values(full[:k, y:y + rh, x:x + rw])
                            for j in range(K):   # level by level: the (K, k, rh, rw) mask need not fit
                                acc[j] += (px <= tcmp[j]).sum(0, dtype=torch.int32)

                    ms = timed(dict(k=arm_k, a=arm_a, b=arm_b, c=arm_c), a.steps, a.warmup)
                    codec.timing(True)
                    codec.timing_read(reset=True)
                    for _ in range(a.steps):
                        arm_k()
                    codec.sync()
                    t = codec.timing_read(reset=True)
                    codec.timing(False)
                    arm_k()
                    arm_c()
                    codec.sync()
                    assert torch.equal(out.out, acc), "the timed planes differ from decode_frames + compare"
                    p = plan_fn(W, H, nf, x, y, rw, rh, levels=K, n_cu=cus, maps=maps)
                    emit(dict(dataset=name, W=W, H=H, frames_per_call=nf, window=[x, y, rw, rh], K=K,
                              mode="maps" if maps else "scalars", segments=p["segments"], ms_counts=ms["k"],
                              ms_project_sum=ms["a"], ms_weighted=ms["b"], ms_frames_compare=ms["c"],
                              counts_over_project_sum=ms["k"] / ms["a"], counts_over_weighted=ms["k"] / ms["b"],
                              frames_compare_over_counts=ms["c"] / ms["k"],
                              ms_index=t["decode_index"][0] / a.steps, ms_kernels=t["decode"][0] / a.steps,
                              equal_to_frames_compare=True))
                    del out, wout, pr, acc, thr, tv, tcmp
        del buf, full, wall, offs

    for name, pix, W, H, n_all in (("quantile", 1, 4096, 3072, 1024), ("quantile16", 2, 4096, 3072, 1024)):
        if a.only and a.only != name:
            continue
        n_all = a.frames or n_all
        buf, offs, stream_bytes = dataset(pix, W, H, n_all)
        bits = 8 * pix
        roi_fn = codec.decode_roi if pix == 1 else codec.decode_roi16
        pdt = torch.uint8 if pix == 1 else torch.int16
        rows = max(8, ((1 << 30) // (n_all * W * pix)) // 8 * 8)   # strip height of the kthvalue arm: ~1 GiB of pixels
        r = (n_all - 1) // 2
        kth = torch.empty((H, W), dtype=pdt, device="cuda")
        state = {}

        def arm_q():
            state["q"] = qt.temporal_median(codec, buf, 0, stream_bytes, offs, W, H, n_all, bits=bits)[0]

        def arm_kth():
            for y0 in range(0, H, rows):
                rh = min(rows, H - y0)
                strip, _ = roi_fn(buf, 0, stream_bytes, offs, W, H, n_all, 0, y0, W, rh)
                v = strip if pix == 1 else (strip.to(torch.int32) & 0xFFFF)
                kth[y0:y0 + rh] = torch.kthvalue(v, r + 1, dim=0).values.to(pdt)
                del strip, v

        ms, peak = {}, {}
        for key, fn in (("q", arm_q), ("kth", arm_kth)):
            fn()
            codec.sync()
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            ts = []
            for _ in range(a.qsteps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1))
            ms[key] = float(np.median(ts))
            peak[key] = int(torch.cuda.max_memory_allocated() - base)
        assert torch.equal(state["q"], kth), "the median differs from decode_roi + kthvalue"
        emit(dict(dataset=name, W=W, H=H, frames=n_all, bits=bits, passes=qt.passes(bits), rank=r, strip_rows=rows,
                  ms_temporal_median=ms["q"], ms_roi_kthvalue=ms["kth"], kthvalue_over_median=ms["kth"] / ms["q"],
                  peak_bytes_temporal_median=peak["q"], peak_bytes_roi_kthvalue=peak["kth"],
                  stream_bytes=int(stream_bytes), decoded_bytes=int(n_all) * W * H * pix, equal=True))
        del buf, offs, kth
    codec.close()


if __name__ == "__main__":
    main()
