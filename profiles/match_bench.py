"""Patch match (the correlation surfaces of K templates over a shift search, straight from the compressed stream) against
the route it replaces and against its floor.

    python profiles/match_bench.py [--only mixed4k|one|u16|largest] [--frames N] [--steps 10] [--warmup 2] [--out FILE]

Each part is a process of its own, meant to run under a time limit of its own (timeout -k 10 900 python ... --only X).
Datasets: 1,024 mixed 4096x3072 frames (synth), the same with one frame per call, 128 DBDE16 4096x3072 frames (16, 12, 8
and 4 significant bits, frame by frame).  The K templates are cut out of frame 0 at seeded random positions
(decode_patches); every frame's search patches sit at those positions less S, moved by a seeded jitter of +-4 pixels per
frame and patch; CLAMP mode.  Cases: K = 16, 64 and 256 templates of 32 x 32 at S = 8 and of 64 x 64 at S = 16, and the
largest legal case, 128 x 128 at S = 16 with K = 64; each with all three surfaces and with prod alone.  Every arm of a
case runs in this process on the same inputs, `warmup` untimed calls and then `steps` timed ones between device events
on the context's stream, the arms interleaved call by call (profiles/registered_bench.py's method); the median is
reported with min and max.
Arms:
  k   match_patches (the timed output);
  b   decode_patches of the same search patches, the floor: the same tiles decoded and written out as pixels;
  a   the route through pixels: decode_patches of the search patches in chunks of frames that keep the decoded pixels at
      2^28 at most, then torch.nn.functional.conv2d in float64 (one group per patch: exact below 2^53) of the patch with
      its template for prod, of the patch and of its square with a kernel of ones for sum and sq.
One JSON line per case with the medians, the ratios k / a and k / b and the plan.  The check: the timed surfaces equal
arm a's, element for element.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETS = (("prod", "sum", "sq"), ("prod",))
SIZES = ((32, 8), (64, 16))
COUNTS = (16, 64, 256)


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


def surfaces_through_pixels(P, T, stats, top):
    """The surfaces of patches P (m, K, ph, pw) and templates T (K, th, tw) as int64 (m, K, D, D), by grouped conv2d in
    float64 (torch's conv2d is a correlation: no flip)."""
    import torch
    import torch.nn.functional as F
    m, K, ph, pw = P.shape
    th, tw = T.shape[1:]
    x = (P.to(torch.int32) & top).to(torch.float64).reshape(1, m * K, ph, pw)
    out = {}
    if "prod" in stats:
        w = (T.to(torch.int32) & top).to(torch.float64)[None].expand(m, K, th, tw).reshape(m * K, 1, th, tw)
        out["prod"] = F.conv2d(x, w, groups=m * K)
    ones = torch.ones((m * K, 1, th, tw), dtype=torch.float64, device=P.device)
    if "sum" in stats:
        out["sum"] = F.conv2d(x, ones, groups=m * K)
    if "sq" in stats:
        out["sq"] = F.conv2d(x * x, ones, groups=m * K)
    return {k: v.reshape(m, K, v.shape[2], v.shape[3]).to(torch.int64) for k, v in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, help="one part: mixed4k, one, u16 or largest")
    ap.add_argument("--frames", type=int, default=0, help="frames per dataset (default 1024; one: 16; u16: 128)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    import torch
    import dbde_video_cpp_amd as dv

    codec = dv.Codec(0)
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
        step = min(16, n_all)
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

    parts = (("mixed4k", 1, 4096, 3072, 1024, None, [(t, S, K) for t, S in SIZES for K in COUNTS]),
             ("one", 1, 4096, 3072, 16, 1, [(t, S, K) for t, S in SIZES for K in COUNTS]),
             ("u16", 2, 4096, 3072, 128, None, [(t, S, 64) for t, S in SIZES]),
             ("largest", 1, 4096, 3072, 1024, None, [(128, 16, 64)]))
    for name, pix, W, H, n_all, per_call, cases in parts:
        if a.only and a.only != name:
            continue
        n_all = a.frames or n_all
        nf = per_call or n_all
        top = 0xFF if pix == 1 else 0xFFFF
        buf, offs, stream_bytes = dataset(pix, W, H, n_all)
        match = codec.match_patches if pix == 1 else codec.match_patches16
        patches = codec.decode_patches if pix == 1 else codec.decode_patches16
        plan_fn = dv.match_plan if pix == 1 else dv.match16_plan
        pdt = torch.uint8 if pix == 1 else torch.int16
        res = torch.empty((nf, 4), dtype=torch.int64, device="cuda")
        o_f = offs[:nf]
        for t, S, K in cases:
            rng = np.random.default_rng(2016 + t + K)
            pw = t + 2 * S
            D = 2 * S + 1
            pos = np.stack([rng.integers(S + 4, W - t - S - 4, K), rng.integers(S + 4, H - t - S - 4, K)], -1)
            T, _ = patches(buf, 0, stream_bytes, offs[:1], W, H, 1, t, t, torch.from_numpy(pos[None].astype(np.int32)).cuda())
            T = T[0].contiguous()
            org = pos[None] - S + rng.integers(-4, 5, (nf, K, 2))
            d_org = torch.from_numpy(org.astype(np.int32)).cuda().contiguous()
            chunk = max(1, min(nf, (1 << 28) // (K * pw * pw)))
            px = torch.empty((chunk, K, pw, pw), dtype=pdt, device="cuda")
            floor_out = torch.empty((nf, K, pw, pw), dtype=pdt, device="cuda")
            for stats in SETS:
                out = {s: torch.empty((nf, K, D, D), dtype=torch.int64, device="cuda") for s in stats}
                ref = {s: torch.empty((nf, K, D, D), dtype=torch.int64, device="cuda") for s in stats}

                def arm_k():
                    match(buf, 0, stream_bytes, o_f, W, H, nf, T, S, d_org, stats=stats, out=out, results=res)

                def arm_b():
                    patches(buf, 0, stream_bytes, o_f, W, H, nf, pw, pw, d_org, out=floor_out, results=res)

                def arm_a():
                    for f0 in range(0, nf, chunk):
                        m = min(chunk, nf - f0)
                        patches(buf, 0, stream_bytes, o_f[f0:f0 + m], W, H, m, pw, pw, d_org[f0:f0 + m], out=px[:m],
                                results=res[f0:f0 + m])
                        for s, v in surfaces_through_pixels(px[:m], T, stats, top).items():
                            ref[s][f0:f0 + m] = v

                ms = timed(dict(k=arm_k, b=arm_b, a=arm_a), a.steps, a.warmup)
                codec.timing(True)
                codec.timing_read(reset=True)
                for _ in range(a.steps):
                    arm_k()
                codec.sync()
                tm = codec.timing_read(reset=True)
                codec.timing(False)
                arm_k()
                codec.sync()
                for s in stats:
                    assert torch.equal(out[s], ref[s]), f"the timed {s} surface differs from the one through pixels"
                p = plan_fn(W, H, nf, t, t, S, K, stats=stats)
                emit(dict(dataset=name, W=W, H=H, bits=8 * pix, frames_per_call=nf, templates=K, template=[t, t], S=S,
                          stats=list(stats), lds_bytes=p["lds_bytes"], row_slices=p["row_slices"],
                          decode_waves=p["decode_waves"], steps_per_patch=p["steps_per_patch"],
                          ms_match=ms["k"], ms_pixels_route=ms["a"], ms_decode_patches_floor=ms["b"],
                          match_over_pixels_route=ms["k"] / ms["a"], match_over_floor=ms["k"] / ms["b"],
                          ms_match_minmax=ms["k_minmax"], ms_pixels_route_minmax=ms["a_minmax"],
                          ms_floor_minmax=ms["b_minmax"], chunk_frames=chunk, ms_index=tm["decode_index"][0] / a.steps,
                          ms_kernel=tm["decode"][0] / a.steps, equal_to_pixels_route=True))
                del out, ref
            del px, floor_out, d_org
        del buf, offs, res
    codec.close()


if __name__ == "__main__":
    main()
