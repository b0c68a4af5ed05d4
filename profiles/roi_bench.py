"""Window (region-of-interest) decode against the full-frame decode of the same batch.

    python profiles/roi_bench.py [--frames 1024] [--W 4096] [--H 3072] [--content mixed] [--steps 20] [--warmup 3]

Builds n synthetic frames on the device, encodes them into one slot per frame, then times (device events around `steps`
calls after `warmup` untimed ones) dbde_hip_decode_frames and dbde_hip_decode_roi for a set of windows, on the whole
batch and on one frame per call.  Prints one JSON line per case:
  ms            median time of one call
  touched_bytes what the call must move at least: decode_frames the frames' bytes + the images; a window the depth arrays
                (the validation reads all of them), the window tiles' depth / minimum bytes, the depth bytes from each
                window tile row's index chunk start to its first tile, the window tiles' payload and the window output
  share_of_peak touched_bytes / ms against 8 TB/s
  vs_full       ms / ms of decode_frames on the same frames
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12


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
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--W", type=int, default=4096)
    ap.add_argument("--H", type=int, default=3072)
    ap.add_argument("--content", default="mixed")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    import torch
    import dbde_video_cpp_amd as dv

    W, H, n = a.W, a.H, a.frames
    w, h = (W + 7) // 8, (H + 7) // 8
    T = w * h
    codec = dv.Codec(0)
    slot = (dv.max_frame_bytes(W, H) + 255) // 256 * 256
    buf = torch.empty(n * slot + 256, dtype=torch.uint8, device="cuda")
    offs = torch.empty(n, dtype=torch.int64, device="cuda")
    sizes = torch.empty(n, dtype=torch.int64, device="cuda")
    step = 64
    for f0 in range(0, n, step):   # synthesize and encode in groups (the images of the whole batch need not fit)
        k = min(step, n - f0)
        imgs = codec.synth_frames(a.content, 0xDBDE2016, f0, k, W, H)
        o, s = codec.encode_frames(imgs, W, H, k, buf, f0 * slot, (n - f0) * slot, first_index=f0, slot_stride=slot)
        offs[f0:f0 + k] = o + f0 * slot
        sizes[f0:f0 + k] = s
        del imgs
    codec.sync()
    stream_bytes = n * slot
    frame_bytes = sizes.double().sum().item()
    # depth arrays of every frame (device), for the bytes a window's tiles hold
    depth = torch.empty((n, T), dtype=torch.uint8, device="cuda")
    ar = torch.arange(T, device="cuda")
    for f0 in range(0, n, step):
        k = min(step, n - f0)
        depth[f0:f0 + k] = buf[(offs[f0:f0 + k, None] + 24 + ar[None, :]).reshape(-1)].view(k, T)
    depth3 = depth.view(n, h, w).to(torch.int64)

    def roi_bytes(nf, x, y, rw, rh):
        pl = dv.roi_plan(W, H, nf, x, y, rw, rh)
        tx0, ty0, ntx, nty = pl["tile_x"], pl["tile_y"], pl["tiles_x"], pl["tiles_y"]
        pay = 8 * depth3[:nf, ty0:ty0 + nty, tx0:tx0 + ntx].sum().item()
        # depth bytes from each window tile row's chunk start to its first tile (one tile row per chunk: tx0 bytes)
        pre = nf * nty * (tx0 % 512 if pl["chunk_pieces"] else 0)
        return nf * T + nf * ntx * nty * 2 + pre + pay + nf * rw * rh

    lines = []
    full_out = torch.empty((n, H, W), dtype=torch.uint8, device="cuda")
    res = torch.empty((n, 4), dtype=torch.int64, device="cuda")
    for nf in (n, 1):
        full_ms = timed(lambda: codec.decode_frames(buf, 0, stream_bytes, offs[:nf], W, H, nf, images=full_out[:nf],
                                                    results=res[:nf]), a.steps, a.warmup)
        if nf == n:
            fb = frame_bytes
        else:
            fb = sizes[:1].double().sum().item()
        full_touch = fb + nf * W * H
        base = dict(W=W, H=H, content=a.content, frames_per_call=nf)
        lines.append(dict(base, case="decode_frames", ms=full_ms, touched_bytes=int(full_touch),
                          share_of_peak=full_touch / (full_ms * 1e-3) / PEAK, vs_full=1.0))
        wins = [("256x256", 1000, 700, 256, 256), ("1024x1024", 1000, 700, 1024, 1024), ("512x512", 1000, 700, 512, 512),
                ("full", 0, 0, W, H)]
        for name, x, y, rw, rh in wins:
            out = torch.empty((nf, rh, rw), dtype=torch.uint8, device="cuda")
            ms = timed(lambda: codec.decode_roi(buf, 0, stream_bytes, offs[:nf], W, H, nf, x, y, rw, rh, out=out,
                                                results=res[:nf]), a.steps, a.warmup)
            tb = roi_bytes(nf, x, y, rw, rh)
            lines.append(dict(base, case=f"decode_roi {name} at ({x},{y})", ms=ms, touched_bytes=int(tb),
                              share_of_peak=tb / (ms * 1e-3) / PEAK, vs_full=ms / full_ms))
            del out
        # correctness spot check of the timed calls: the 256x256 window is a crop of the full decode
        out = torch.empty((nf, 256, 256), dtype=torch.uint8, device="cuda")
        codec.decode_roi(buf, 0, stream_bytes, offs[:nf], W, H, nf, 1000, 700, 256, 256, out=out)
        codec.sync()
        assert torch.equal(out, full_out[:nf, 700:956, 1000:1256]), "window differs from the full decode"
    for ln in lines:
        print(json.dumps(ln), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    codec.close()


if __name__ == "__main__":
    main()
