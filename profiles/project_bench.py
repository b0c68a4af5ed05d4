"""Temporal projections (dbde_hip_project) against decoding the batch and reducing the images in torch.

    python profiles/project_bench.py [--rounds 3] [--seconds 0.6] [--out profiles/project_bench.jsonl]

Datasets (each encoded on the device into one slot per frame): 1,024 mixed and 1,024 noise8 4096x3072 frames, and
262,144 mixed 64x64 frames.  Arms, timed with device events over repeated calls (at least --seconds of work per figure,
after a warm-up), alternated round by round so that the spread shows:
  a  decode_frames alone
  b  decode_frames + torch reductions to max, min, sum and sum of squares (int64, 64 frames at a time)
  c  project, all four statistics
  d  project, max and min only
  e  project of a 512x512 window (4096x3072 only)
Prints one JSON line per (dataset, arm, round):
  ms             time of one call
  read_bytes     bytes the call must read at least, computed here from the streams: a, b, c, d the frames' bytes (b also
                 reads the images back once); e the depth arrays, the window tiles' minimum bytes, the depth bytes from
                 each window tile row's index chunk start to its first tile, and the window tiles' payload
  written_bytes  images (a, b); the outputs are negligible for c, d, e
  share_of_peak  (read_bytes + written_bytes) / time against 8 TB/s
The projections are checked once against the torch reductions (b) of the same frames before any timing.
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.6)
    ap.add_argument("--only", default=None, help="one dataset: mixed4k, noise4k or small")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    import torch
    import dbde_video_cpp_amd as dv

    codec = dv.Codec(0)
    datasets = [("mixed4k", "mixed", 4096, 3072, 1024), ("noise4k", "noise8", 4096, 3072, 1024),
                ("small", "mixed", 64, 64, 262144)]
    lines = []
    for name, content, W, H, n in datasets:
        if a.only and name != a.only:
            continue
        w, h = (W + 7) // 8, (H + 7) // 8
        T = w * h
        slot = (dv.max_frame_bytes(W, H) + 255) // 256 * 256
        buf = torch.empty(n * slot + 256, dtype=torch.uint8, device="cuda")
        offs = torch.empty(n, dtype=torch.int64, device="cuda")
        sizes = torch.empty(n, dtype=torch.int64, device="cuda")
        step = max(1, min(n, (1 << 28) // (W * H)))
        for f0 in range(0, n, step):   # synthesize and encode in groups
            k = min(step, n - f0)
            imgs = codec.synth_frames(content, 0xDBDE2016, f0, k, W, H)
            o, s = codec.encode_frames(imgs, W, H, k, buf, f0 * slot, (n - f0) * slot, first_index=f0,
                                       slot_stride=slot)
            offs[f0:f0 + k] = o + f0 * slot
            sizes[f0:f0 + k] = s
            del imgs
        codec.sync()
        stream_bytes = n * slot
        frame_bytes = int(sizes.sum().item())
        images = torch.empty((n, H, W), dtype=torch.uint8, device="cuda")
        res = torch.empty((n, 4), dtype=torch.int64, device="cuda")

        def decode():
            codec.decode_frames(buf, 0, stream_bytes, offs, W, H, n, images=images, results=res)

        ref = {s: None for s in ALL}
        chunk = max(1, min(n, (1 << 26) // (W * H)))

        def decode_reduce():
            decode()
            mx = mn = sm = sq = None
            for f0 in range(0, n, chunk):
                x = images[f0:f0 + chunk]
                x64 = x.to(torch.int64)
                a_, b_, c_, d_ = x.amax(0), x.amin(0), x64.sum(0), (x64 * x64).sum(0)
                mx = a_ if mx is None else torch.maximum(mx, a_)
                mn = b_ if mn is None else torch.minimum(mn, b_)
                sm = c_ if sm is None else sm + c_
                sq = d_ if sq is None else sq + d_
            ref.update(max=mx, min=mn, sum=sm, sumsq=sq)

        proj_all = dv.Projection.empty(H, W, ALL, "cuda")
        proj_mm = dv.Projection.empty(H, W, ("max", "min"), "cuda")
        arms = [("a decode_frames", decode), ("b decode_frames + torch reductions", decode_reduce),
                ("c project all four", lambda: codec.project(buf, 0, stream_bytes, offs, W, H, n, out=proj_all,
                                                             results=res)),
                ("d project max+min", lambda: codec.project(buf, 0, stream_bytes, offs, W, H, n, out=proj_mm,
                                                            results=res))]
        win = None
        if W >= 512 and H >= 512:
            win = (1000, 700, 512, 512) if W >= 1512 else (0, 0, 512, 512)
            proj_win = dv.Projection.empty(512, 512, ALL, "cuda")
            arms.append(("e project 512x512 window", lambda: codec.project(buf, 0, stream_bytes, offs, W, H, n, *win,
                                                                          out=proj_win, results=res)))

        # check the projections against the torch reductions once
        decode_reduce()
        for _, fn in arms[2:]:
            fn()
        codec.sync()
        assert int(proj_all.count.item()) == n
        for s in ALL:
            assert torch.equal(getattr(proj_all, s).to(torch.int64), ref[s].to(torch.int64)), (name, s)
        assert torch.equal(proj_mm.max, ref["max"]) and torch.equal(proj_mm.min, ref["min"])
        if win:
            x, y, rw, rh = win
            assert torch.equal(proj_win.sum, ref["sum"][y:y + rh, x:x + rw])

        # bytes each arm must read / write
        depth = torch.empty((n, T), dtype=torch.uint8, device="cuda")
        ar = torch.arange(T, device="cuda")
        dstep = max(1, min(n, (1 << 26) // T))
        for f0 in range(0, n, dstep):
            k = min(dstep, n - f0)
            depth[f0:f0 + k] = buf[(offs[f0:f0 + k, None] + 24 + ar[None, :]).reshape(-1)].view(k, T)
        rb = {"a": frame_bytes, "b": frame_bytes + n * W * H, "c": frame_bytes, "d": frame_bytes}
        wb = {"a": n * W * H, "b": n * W * H, "c": 0, "d": 0}
        if win:
            pl = dv.project_plan(W, H, n, *win)
            tx0, ty0, ntx, nty = pl["tile_x"], pl["tile_y"], pl["tiles_x"], pl["tiles_y"]
            pay = 8 * int(depth.view(n, h, w)[:, ty0:ty0 + nty, tx0:tx0 + ntx].to(torch.int64).sum().item())
            pre = n * nty * (tx0 % 512 if pl["chunk_pieces"] else 0)
            rb["e"], wb["e"] = n * T + n * ntx * nty + pre + pay, 0
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
                print(json.dumps(ln), flush=True)
                lines.append(ln)
        del buf, images, proj_all, proj_mm, ref
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    codec.close()


if __name__ == "__main__":
    main()
