"""Region traces (dbde_hip_traces / dbde16_hip_traces) against decoding the batch and reducing the images over the label
map in torch; profiles/project_bench.py's method.

    python profiles/trace_bench.py [--rounds 3] [--seconds 0.6] [--out profiles/trace_bench.jsonl]

Datasets (encoded on the device, one slot per frame): 1,024 mixed and 1,024 noise8 4096x3072 frames, and 128 DBDE16
4096x3072 frames with per-tile depths uniform in 0..16 (project16_bench.py's mixed16).  Label maps:
  dense   2,000 random discs of radius 16..32 (about 30 % of the pixels)
  sparse  random discs of radius 16..32 until about 5 % of the tiles are active
  blocks  64x64 blocks, one label each: every tile whole
Arms, timed with device events over repeated calls (at least --seconds of work per figure, after a warm-up), alternated
round by round:
  a  decode_frames alone
  b  decode_frames + torch reductions (scatter_reduce amax / amin, scatter_add) over the dense map, int64
  c  traces, all four statistics, dense map
  d  traces, all four statistics, sparse map
  e  traces, all four statistics, blocks map
  f  project, all four statistics, whole frame (the §4.7 arm, for target e)
Prints one JSON line per (dataset, arm, round): ms, read_bytes (a, b, f the frames' bytes, b also the images once; c, d,
e the depth arrays plus the active tiles' minima and payload), written_bytes (the images for a and b), share_of_peak
against 8 TB/s, and for c, d, e the map's active-tile share.  The traces are checked once against (b) before any timing.
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))

PEAK = 8.0e12
ALL = ("max", "min", "sum", "sumsq")


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


def discs(W, H, count, seed):
    rng = np.random.default_rng(seed)
    lab = np.zeros((H, W), np.int32)
    for k in range(count):
        cx, cy, r = int(rng.integers(0, W)), int(rng.integers(0, H)), int(rng.integers(16, 33))
        y0, y1, x0, x1 = max(0, cy - r), min(H, cy + r + 1), max(0, cx - r), min(W, cx + r + 1)
        yy, xx = np.mgrid[y0:y1, x0:x1]
        lab[y0:y1, x0:x1][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = k + 1
    return lab


def maps(dv, W, H):
    dense = discs(W, H, 2000, 1)
    count = 20
    while True:   # sparse: about 5 % of the tiles active
        sparse = discs(W, H, count, 2)
        s = dv.trace_map_summary(sparse, count)
        if s["tiles_active"] >= 0.05 * s["tiles"]:
            break
        count += 20
    by, bx = np.mgrid[0:H, 0:W]
    blocks = ((by // 64) * ((W + 63) // 64) + bx // 64 + 1).astype(np.int32)
    return {"dense": (dense, 2000), "sparse": (sparse, count), "blocks": (blocks, int(blocks.max()))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.6)
    ap.add_argument("--only", default=None, help="one dataset: mixed4k, noise4k or mixed16_4k")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    import torch
    import dbde_video_cpp_amd as dv
    from project16_bench import frames16

    codec = dv.Codec(0)
    W, H = 4096, 3072
    w, h = (W + 7) // 8, (H + 7) // 8
    T = w * h
    the_maps = maps(dv, W, H)
    tmaps = {k: codec.trace_map(lab, L) for k, (lab, L) in the_maps.items()}
    datasets = [("mixed4k", "mixed", 1024, 1), ("noise4k", "noise8", 1024, 1), ("mixed16_4k", "mixed16", 128, 2)]
    lines = []
    for name, content, n, pix in datasets:
        if a.only and name != a.only:
            continue
        maxf = dv.max_frame_bytes(W, H) if pix == 1 else int(codec.L.dbde16_hip_max_frame_bytes(W, H))
        slot = (maxf + 255) // 256 * 256
        buf = torch.empty(n * slot + 256, dtype=torch.uint8, device="cuda")
        offs = torch.empty(n, dtype=torch.int64, device="cuda")
        sizes = torch.empty(n, dtype=torch.int64, device="cuda")
        step = max(1, min(n, (1 << 28) // (W * H)))
        gen = torch.Generator(device="cuda").manual_seed(16)
        for f0 in range(0, n, step):   # synthesize and encode in groups
            k = min(step, n - f0)
            if pix == 1:
                imgs = codec.synth_frames(content, 0xDBDE2016, f0, k, W, H)
                o, s = codec.encode_frames(imgs, W, H, k, buf, f0 * slot, (n - f0) * slot, first_index=f0,
                                           slot_stride=slot)
            else:
                imgs = frames16("mixed16", k, W, H, gen)
                o, s = codec.encode_frames16(imgs, W, H, k, buf, f0 * slot, (n - f0) * slot, first_index=f0,
                                             slot_stride=slot)
            offs[f0:f0 + k] = o + f0 * slot
            sizes[f0:f0 + k] = s
            del imgs
        codec.sync()
        stream_bytes = n * slot
        frame_bytes = int(sizes.sum().item())
        images = torch.empty((n, H, W), dtype=torch.uint8 if pix == 1 else torch.int16, device="cuda")
        res = torch.empty((n, 4), dtype=torch.int64, device="cuda")

        def decode():
            if pix == 1:
                codec.decode_frames(buf, 0, stream_bytes, offs, W, H, n, images=images, results=res)
            else:
                codec.decode_frames16(buf, 0, stream_bytes, offs, W, H, n, images=images)

        dense, Ld = the_maps["dense"]
        lab = torch.from_numpy(dense.astype(np.int64)).cuda().reshape(-1)
        keep = lab > 0
        idx = (lab[keep] - 1).unsqueeze(0)
        ref = {}
        chunk = 16

        def decode_reduce():
            decode()
            mx = torch.zeros((n, Ld), dtype=torch.int64, device="cuda")
            mn = torch.full((n, Ld), 255 if pix == 1 else 65535, dtype=torch.int64, device="cuda")
            sm = torch.zeros((n, Ld), dtype=torch.int64, device="cuda")
            sq = torch.zeros((n, Ld), dtype=torch.int64, device="cuda")
            for f0 in range(0, n, chunk):
                k = min(chunk, n - f0)
                v = images[f0:f0 + k].reshape(k, -1)[:, keep].to(torch.int64)
                if pix == 2:
                    v &= 0xFFFF
                ix = idx.expand(k, -1)
                mx[f0:f0 + k] = mx[f0:f0 + k].scatter_reduce(1, ix, v, "amax", include_self=True)
                mn[f0:f0 + k] = mn[f0:f0 + k].scatter_reduce(1, ix, v, "amin", include_self=True)
                sm[f0:f0 + k].scatter_add_(1, ix, v)
                sq[f0:f0 + k].scatter_add_(1, ix, v * v)
            ref.update(max=mx, min=mn, sum=sm, sumsq=sq)

        run = codec.traces if pix == 1 else codec.traces16
        outs = {k: dv.Traces.empty(n, tm.n_labels, ALL, "cuda", pix=pix, pixels=tm.pixels) for k, tm in tmaps.items()}
        proj = dv.Projection.empty(H, W, ALL, "cuda", pix=pix)
        project = codec.project if pix == 1 else codec.project16

        def tr(k):
            return lambda: run(buf, 0, stream_bytes, offs, W, H, n, tmaps[k], out=outs[k], results=res)

        arms = [("a decode_frames", decode), ("b decode_frames + torch reductions over the dense map", decode_reduce),
                ("c traces dense map", tr("dense")), ("d traces sparse map", tr("sparse")),
                ("e traces blocks map", tr("blocks")),
                ("f project all four", lambda: project(buf, 0, stream_bytes, offs, W, H, n, out=proj, results=res))]

        # check the dense traces against the torch reductions once
        decode_reduce()
        tr("dense")()
        codec.sync()
        for s in ALL:
            got = getattr(outs["dense"], s).to(torch.int64)
            if pix == 2 and s in ("max", "min"):
                got &= 0xFFFF
            assert torch.equal(got, ref[s]), (name, s)

        # bytes each arm must read / write
        depth = torch.empty((n, T), dtype=torch.uint8, device="cuda")
        ar = torch.arange(T, device="cuda")
        dstep = max(1, min(n, (1 << 26) // T))
        for f0 in range(0, n, dstep):
            k = min(dstep, n - f0)
            depth[f0:f0 + k] = buf[(offs[f0:f0 + k, None] + 24 + ar[None, :]).reshape(-1)].view(k, T)
        rb = {"a": frame_bytes, "b": frame_bytes + n * W * H * pix, "f": frame_bytes}
        wb = {"a": n * W * H * pix, "b": n * W * H * pix, "c": 0, "d": 0, "e": 0, "f": 0}
        share = {}
        for arm_key, mk in (("c", "dense"), ("d", "sparse"), ("e", "blocks")):
            labm = the_maps[mk][0]
            pad = np.zeros((h * 8, w * 8), np.int32)
            pad[:H, :W] = labm
            act = (pad.reshape(h, 8, w, 8) > 0).any(axis=(1, 3)).reshape(-1)
            act_t = torch.from_numpy(act).cuda()
            pay = 8 * int(depth[:, act_t].to(torch.int64).sum().item())
            rb[arm_key] = n * T + n * int(act.sum()) * pix + pay
            share[arm_key] = float(act.mean())
        del depth

        for _, fn in arms:   # warm-up
            fn()
        codec.sync()
        for rnd in range(a.rounds):
            order = arms if rnd % 2 == 0 else arms[::-1]
            for arm, fn in order:
                ms, reps = timed(fn, a.seconds)
                k = arm[0]
                ln = dict(dataset=name, content=content, W=W, H=H, frames=n, arm=arm, round=rnd, reps=reps, ms=ms,
                          read_bytes=rb[k], written_bytes=wb[k],
                          share_of_peak=(rb[k] + wb[k]) / (ms * 1e-3) / PEAK, measured=True)
                if k in share:
                    ln["active_tiles"] = share[k]
                print(json.dumps(ln), flush=True)
                lines.append(ln)
        del buf, images, outs, proj, ref
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    for tm in tmaps.values():
        tm.close()
    codec.close()


if __name__ == "__main__":
    main()
