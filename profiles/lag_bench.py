"""Lag projection (per-pixel products and differences of frames `lag` apart, in one pass over the compressed stream)
against the floor (project's sum and sumsq) and the only route there was without it.

    python profiles/lag_bench.py [--only mixed4k|small|u16] [--frames N] [--steps 10] [--warmup 2] [--out FILE]

Datasets (profiles/pairs_bench.py's): 1,024 mixed 4096x3072 frames (synth), 65,536 mixed 64x64 frames, 128 DBDE16
4096x3072 frames (16, 12, 8 and 4 significant bits, frame by frame).  Cases: the full frame, a 1024x1024 and a 256x256
window, lag + 1 frames per call (one frame per call means nothing for a lag), the small frames and the DBDE16 frames,
each at lag 1 and lag 8 with sqdiff alone, product + pairsum, and all five statistics.  Every arm of a case runs in this
process on the same inputs, `warmup` untimed calls and then `steps` timed ones between device events on the context's
stream, the arms interleaved call by call; the median is reported with min and max.  Arms:
  k   project_lag (the timed output);
  b   project(stats=("sum", "sumsq")), the floor: the same frames reduced pixel by pixel, no history;
  a   the same planes through pixels: decode_frames (the full frame) or decode_roi (a window) in chunks of frames that
      keep the decoded pixels at 2^28 at most, the chunks overlapping by `lag` frames, and the shifted arithmetic on two
      views of the chunk summed into int64 planes in torch.  chunk_frames and the arm's peak device memory on top of the
      stream are recorded.
One JSON line per case with the medians, the ratios k / b and a / k, the per-plane cost over the floor
((k - b) / planes) and the plan (instance, segments, history frames).  The check: the timed planes and the pair count
equal arm a's, element for element.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETS = (("sqdiff",), ("product", "pairsum"), ("product", "pairsum", "absdiff", "sqdiff", "maxdiff"))


def timed(arms, steps, warmup):
    """{name: fn} -> {name: median ms, name + "_minmax": [min, max]}; the arms alternate call by call, each between its
    own pair of events."""
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
    out = {k: float(np.median(v)) for k, v in ms.items()}
    out.update({k + "_minmax": [float(min(v)), float(max(v))] for k, v in ms.items()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, help="one part: mixed4k, small or u16")
    ap.add_argument("--frames", type=int, default=0, help="frames per dataset (default 1024; small: 65536; u16: 128)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
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

    class Pixels:
        """Arm a: the planes of `stats` at `lag` of nf frames through decoded pixels, in chunks overlapping by lag."""

        def __init__(self, pix, buf, stream_bytes, offs, W, H, nf, win, lag, stats):
            self.pix, self.buf, self.sb, self.offs, self.W, self.H, self.nf = pix, buf, stream_bytes, offs, W, H, nf
            self.win, self.lag, self.stats = win, lag, stats
            x, y, rw, rh = win
            self.whole = (rw, rh) == (W, H)
            self.chunk = max(1, min(nf, (1 << 28) // (rw * rh) - lag))
            pdt = torch.uint8 if pix == 1 else torch.int16
            self.pixels = torch.empty((min(self.chunk + lag, nf), rh, rw), dtype=pdt, device="cuda")
            self.acc = {k: torch.empty((rh, rw), dtype=torch.int64, device="cuda") for k in stats}

        def __call__(self):
            x, y, rw, rh = self.win
            lag = self.lag
            for t in self.acc.values():
                t.zero_()
            for f0 in range(0, self.nf, self.chunk):
                s, e = max(f0 - lag, 0), min(f0 + self.chunk, self.nf)
                k = e - s
                o = self.offs[s:e]
                if self.whole and self.pix == 1:
                    codec.decode_frames(self.buf, 0, self.sb, o, self.W, self.H, k, images=self.pixels[:k])
                elif self.whole:
                    codec.decode_frames16(self.buf, 0, self.sb, o, self.W, self.H, k, images=self.pixels[:k])
                else:
                    roi = codec.decode_roi if self.pix == 1 else codec.decode_roi16
                    roi(self.buf, 0, self.sb, o, self.W, self.H, k, x, y, rw, rh, out=self.pixels[:k])
                if k <= lag:
                    continue
                px = self.pixels[:k].to(torch.int32)
                if self.pix == 2:
                    px &= 0xFFFF
                    px = px.to(torch.int64)      # a U16 product needs more than int32
                pa, pb = px[:k - lag], px[lag:]
                if "product" in self.acc:
                    self.acc["product"] += (pa * pb).sum(0, dtype=torch.int64)
                if "pairsum" in self.acc:
                    self.acc["pairsum"] += (pa + pb).sum(0, dtype=torch.int64)
                if {"absdiff", "sqdiff", "maxdiff"} & set(self.acc):
                    d = (pb - pa).abs_()
                    if "absdiff" in self.acc:
                        self.acc["absdiff"] += d.sum(0, dtype=torch.int64)
                    if "sqdiff" in self.acc:
                        self.acc["sqdiff"] += (d * d).sum(0, dtype=torch.int64)
                    if "maxdiff" in self.acc:
                        self.acc["maxdiff"] = torch.maximum(self.acc["maxdiff"], d.amax(0).to(torch.int64))
                    del d
                del px, pa, pb

    def peak_of(fn):
        fn()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return int(torch.cuda.max_memory_allocated() - base)

    for name, pix, W, H, n_all in (("mixed4k", 1, 4096, 3072, 1024), ("small", 1, 64, 64, 65536), ("u16", 2, 4096, 3072, 128)):
        if a.only and a.only != name:
            continue
        n_all = a.frames or n_all
        buf, offs, stream_bytes = dataset(pix, W, H, n_all)
        lagp = codec.project_lag if pix == 1 else codec.project_lag16
        proj = codec.project if pix == 1 else codec.project16
        plan_fn = dv.lag_plan if pix == 1 else dv.lag16_plan
        res = torch.empty((n_all, 4), dtype=torch.int64, device="cuda")
        if name == "mixed4k":
            wins = [(n_all, (0, 0, W, H)), (n_all, (1536, 1024, 1024, 1024)), (n_all, (1920, 1408, 256, 256)),
                    (None, (0, 0, W, H))]      # None: lag + 1 frames per call
        else:
            wins = [(n_all, (0, 0, W, H))]
        for nf0, (x, y, rw, rh) in wins:
            for lag in (1, 8):
                nf = lag + 1 if nf0 is None else nf0
                for stats in SETS:
                    o_f, r_f = offs[:nf], res[:nf]
                    out = dv.LagProjection.empty(stats, rh, rw, codec.device, lag=lag, bits=8 * pix)
                    pr = dv.Projection.empty(rh, rw, ("sum", "sumsq"), codec.device, pix=pix)
                    px_arm = Pixels(pix, buf, stream_bytes, o_f, W, H, nf, (x, y, rw, rh), lag, stats)

                    def arm_k():
                        lagp(buf, 0, stream_bytes, o_f, W, H, nf, lag, stats, 0, x, y, rw, rh, out=out, results=r_f)

                    def arm_b():
                        proj(buf, 0, stream_bytes, o_f, W, H, nf, x, y, rw, rh, out=pr, results=r_f)

                    ms = timed(dict(k=arm_k, b=arm_b, a=px_arm), a.steps, a.warmup)
                    codec.timing(True)
                    codec.timing_read(reset=True)
                    for _ in range(a.steps):
                        arm_k()
                    codec.sync()
                    t = codec.timing_read(reset=True)
                    codec.timing(False)
                    peak_a = peak_of(px_arm)
                    arm_k()
                    codec.sync()
                    for k in stats:
                        got = getattr(out, k)
                        got = got.to(torch.int64) & (0xFF if pix == 1 else 0xFFFF) if k == "maxdiff" else got
                        assert torch.equal(got, px_arm.acc[k]), f"the timed {k} plane differs from the one through pixels"
                    assert int(out.pairs.item()) == max(nf - lag, 0) and int(out.count.item()) == nf
                    p = plan_fn(W, H, nf, x, y, rw, rh, lag=lag, stats=dv.lag_mask(stats), n_cu=cus)
                    emit(dict(dataset=name, W=W, H=H, frames_per_call=nf, window=[x, y, rw, rh], lag=lag,
                              stats=list(stats), planes=p["planes"], instance=p["instance"], pieces_x=p["pieces_x"],
                              segments=p["segments"], history_frames=p["history_frames"], ms_lag=ms["k"],
                              ms_project_sum_sumsq=ms["b"], ms_pixels_route=ms["a"], lag_over_floor=ms["k"] / ms["b"],
                              ms_per_plane_over_floor=(ms["k"] - ms["b"]) / p["planes"],
                              pixels_route_over_lag=ms["a"] / ms["k"], ms_lag_minmax=ms["k_minmax"],
                              ms_floor_minmax=ms["b_minmax"], ms_pixels_route_minmax=ms["a_minmax"],
                              chunk_frames=px_arm.chunk, peak_bytes_pixels_route=peak_a,
                              ms_index=t["decode_index"][0] / a.steps, ms_kernels=t["decode"][0] / a.steps,
                              equal_to_pixels_route=True))
                    del out, pr, px_arm
        del buf, offs, res
    codec.close()


if __name__ == "__main__":
    main()
