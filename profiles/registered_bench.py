"""Registered projection (project's statistics of a window whose origin moves with the frames, in one pass over the
compressed stream) against the floor (project on the same window, no shifts) and the route it replaces.

    python profiles/registered_bench.py [--only mixed4k|one|small|u16] [--frames N] [--steps 10] [--warmup 2] [--out FILE]

Each part is a process of its own, meant to run under a time limit of its own (timeout -k 10 900 python ... --only X).
Datasets: 1,024 mixed 4096x3072 frames (synth), the same with one frame per call, 65,536 mixed 512x512 frames, 128 DBDE16
4096x3072 frames (16, 12, 8 and 4 significant bits, frame by frame).  The shifts are uniform random integers in +-16
(seeded), the window is registration.origins_from_shifts' common window; mixed4k runs four variants -- all-zero
shifts, x only, y only (which separates the re-alignment of the columns from the second tile row's prefix), both --
the other parts run `both`.  Each with sum alone and with all four statistics.  Every arm of a case runs in this
process on the same inputs, `warmup` untimed calls and then `steps` timed ones between device events on the context's
stream, the arms interleaved call by call (profiles/lag_bench.py's method); the median is reported with min and max.
Arms:
  k   project_registered (the timed output);
  b   project on the common window at its place for zero shift, the floor: the same frames and statistics, no origins;
  a   the same planes through pixels: decode_roi(origins=...) in chunks of frames that keep the decoded pixels at 2^28
      at most, reduced in torch into the planes.  chunk_frames and the arm's peak device memory on top of the stream
      are recorded.
One JSON line per case with the medians, the ratios k / b and a / k and the plan.  The check: the timed planes equal
arm a's, element for element.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETS = (("sum",), ("max", "min", "sum", "sumsq"))
VARIANTS = ("zero", "x", "y", "both")


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


def shifts_of(variant, n, seed=2016):
    s = np.random.default_rng(seed).integers(-16, 17, (n, 2))
    if variant == "zero":
        s[:] = 0
    elif variant == "x":
        s[:, 1] = 0
    elif variant == "y":
        s[:, 0] = 0
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, help="one part: mixed4k, one, small or u16")
    ap.add_argument("--frames", type=int, default=0, help="frames per dataset (default 1024; small: 65536; u16: 128)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    import torch
    import dbde_video_cpp_amd as dv
    from dbde_video_cpp_amd import registration as reg

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
        step = min(16 if W > 512 else 1024, n_all)
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
        """Arm a: the planes of `stats` of nf frames through decode_roi(origins) and torch reductions, in chunks."""

        def __init__(self, pix, buf, stream_bytes, offs, W, H, nf, rw, rh, origins, stats):
            self.pix, self.buf, self.sb, self.offs, self.W, self.H, self.nf = pix, buf, stream_bytes, offs, W, H, nf
            self.rw, self.rh, self.origins, self.stats = rw, rh, origins, stats
            self.chunk = max(1, min(nf, (1 << 28) // (rw * rh)))
            pdt = torch.uint8 if pix == 1 else torch.int16
            self.pixels = torch.empty((self.chunk, rh, rw), dtype=pdt, device="cuda")
            self.acc = {k: torch.empty((rh, rw), dtype=torch.int64, device="cuda") for k in stats}

        def __call__(self):
            top = 0xFF if self.pix == 1 else 0xFFFF
            for k, t in self.acc.items():
                t.fill_(top if k == "min" else 0)
            roi = codec.decode_roi if self.pix == 1 else codec.decode_roi16
            for f0 in range(0, self.nf, self.chunk):
                k = min(self.chunk, self.nf - f0)
                roi(self.buf, 0, self.sb, self.offs[f0:f0 + k], self.W, self.H, k, 0, 0, self.rw, self.rh,
                    origins=self.origins[f0:f0 + k], out=self.pixels[:k])
                px = self.pixels[:k]
                if self.pix == 2:
                    px = px.to(torch.int32) & 0xFFFF
                if "max" in self.acc:
                    self.acc["max"] = torch.maximum(self.acc["max"], px.amax(0).to(torch.int64))
                if "min" in self.acc:
                    self.acc["min"] = torch.minimum(self.acc["min"], px.amin(0).to(torch.int64))
                if "sum" in self.acc:
                    self.acc["sum"] += px.sum(0, dtype=torch.int64)
                if "sumsq" in self.acc:
                    p64 = px.to(torch.int64) if self.pix == 2 else px.to(torch.int32)
                    self.acc["sumsq"] += (p64 * p64).sum(0, dtype=torch.int64)
                    del p64
                del px

    def peak_of(fn):
        fn()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return int(torch.cuda.max_memory_allocated() - base)

    parts = (("mixed4k", 1, 4096, 3072, 1024, None, VARIANTS), ("one", 1, 4096, 3072, 16, 1, ("both",)),
             ("small", 1, 512, 512, 65536, None, ("both",)), ("u16", 2, 4096, 3072, 128, None, ("both",)))
    for name, pix, W, H, n_all, per_call, variants in parts:
        if a.only and a.only != name:
            continue
        n_all = a.frames or n_all
        nf = per_call or n_all
        buf, offs, stream_bytes = dataset(pix, W, H, n_all)
        regp = codec.project_registered if pix == 1 else codec.project_registered16
        proj = codec.project if pix == 1 else codec.project16
        plan_fn = dv.registered_plan if pix == 1 else dv.registered16_plan
        res = torch.empty((n_all, 4), dtype=torch.int64, device="cuda")
        for variant in variants:
            # the window of the `both` shifts for every variant, so that the variants reduce the same number of pixels
            _, rw, rh, (X0, Y0) = reg.origins_from_shifts(shifts_of("both", n_all), W, H)
            s = shifts_of(variant, n_all)
            origins = torch.from_numpy((s + (X0, Y0)).astype(np.int32)).cuda().contiguous()
            for stats in SETS:
                o_f, r_f, org = offs[:nf], res[:nf], origins[:nf]
                out = dv.Projection.empty(rh, rw, stats, codec.device, pix=pix)
                pr = dv.Projection.empty(rh, rw, stats, codec.device, pix=pix)
                px_arm = Pixels(pix, buf, stream_bytes, o_f, W, H, nf, rw, rh, org, stats)

                def arm_k():
                    regp(buf, 0, stream_bytes, o_f, W, H, nf, rw, rh, org, out=out, results=r_f)

                def arm_b():
                    proj(buf, 0, stream_bytes, o_f, W, H, nf, X0, Y0, rw, rh, out=pr, results=r_f)

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
                top = 0xFF if pix == 1 else 0xFFFF
                for k in stats:
                    got = getattr(out, k)
                    got = got.to(torch.int64) & top if k in ("max", "min") else got
                    assert torch.equal(got, px_arm.acc[k]), f"the timed {k} plane differs from the one through pixels"
                assert int(out.count.item()) == nf
                p = plan_fn(W, H, nf, rw, rh, stats=stats, n_cu=cus)
                emit(dict(dataset=name, W=W, H=H, frames_per_call=nf, window=[rw, rh], shifts=variant, stats=list(stats),
                          instance=p["instance"], pieces_x=p["pieces_x"], bands=p["bands"], segments=p["segments"],
                          ms_registered=ms["k"], ms_project_floor=ms["b"], ms_pixels_route=ms["a"],
                          registered_over_floor=ms["k"] / ms["b"], pixels_route_over_registered=ms["a"] / ms["k"],
                          ms_registered_minmax=ms["k_minmax"], ms_floor_minmax=ms["b_minmax"],
                          ms_pixels_route_minmax=ms["a_minmax"], chunk_frames=px_arm.chunk,
                          peak_bytes_pixels_route=peak_a, ms_index=t["decode_index"][0] / a.steps,
                          ms_kernels=t["decode"][0] / a.steps, equal_to_pixels_route=True))
                del out, pr, px_arm
        del buf, offs, res
    codec.close()


if __name__ == "__main__":
    main()
