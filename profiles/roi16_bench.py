"""DBDE16 window (region-of-interest) decode against the full 16-bit decode of the same batch.

    python profiles/roi16_bench.py [--frames 128] [--steps 20] [--warmup 3] [--out FILE] [--lib PATH] [--tag NAME]

Builds n frames of 4096x3072 U16 on the device with a per-tile depth uniform in 0..16 (profiles/u16_bench.py's
content), encodes them (concatenated), then times (device events around `steps` calls after `warmup` untimed ones)
dbde16_hip_decode_frames and dbde16_hip_decode_roi for a set of windows, on the whole batch and on one frame per call.
--lib loads another build of libdbde_hip.so (an A/B variant of the window kernel's piece width).
Prints one JSON line per case:
  ms            median time of one call
  touched_bytes what the call must move at least: decode_frames16 the frames' bytes + the images; a window the depth
                arrays (the validation reads all of them), the window tiles' depth bytes and U16 minima, the depth bytes
                from each window tile row's index chunk start to its first tile, the window tiles' payload and the
                window output (2 bytes per pixel)
  share_of_peak touched_bytes / ms against 8 TB/s
  vs_full       ms / ms of decode_frames16 on the same frames
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 8.0e12
W, H = 4096, 3072


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
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--lib", default=None, help="libdbde_hip.so to load instead of the in-tree build")
    ap.add_argument("--tag", default="", help="label of the library in the JSON lines")
    a = ap.parse_args()

    import torch
    import dbde_video_cpp_amd as dv
    if a.lib:
        dv.LIB_PATH = os.path.abspath(a.lib)

    n = a.frames
    w, h = W // 8, H // 8
    T = w * h
    codec = dv.Codec(0)
    g = torch.Generator(device="cuda").manual_seed(1)
    d = torch.randint(0, 17, (n, h, w), device="cuda", generator=g)
    dd = d.repeat_interleave(8, 1).repeat_interleave(8, 2)
    mask = (torch.ones_like(dd) << dd) - 1
    noise = torch.randint(0, 65536, (n, H, W), device="cuda", generator=g) & mask
    base = torch.randint(0, 32768, (n, h, w), device="cuda", generator=g).repeat_interleave(8, 1).repeat_interleave(8, 2)
    imgs = torch.minimum(base, 65535 - mask).add_(noise).to(torch.int32).to(torch.int16).contiguous()
    del d, dd, mask, noise, base
    maxf = int(codec.L.dbde16_hip_max_frame_bytes(W, H))
    cap = n * maxf
    buf = torch.empty(32 + cap + 64, dtype=torch.uint8, device="cuda")
    offs, sizes = codec.encode_frames16(imgs, W, H, n, buf, 32, cap)
    codec.sync()
    stream_bytes = int((offs[-1] + sizes[-1]).item())
    frame_bytes = sizes.double().sum().item()
    depth = buf[(32 + offs[:, None] + 24 + torch.arange(T, device="cuda")[None, :]).reshape(-1)].view(n, h, w)
    depth3 = depth.to(torch.int64)

    def roi_bytes(nf, x, y, rw, rh):
        pl = dv.roi16_plan(W, H, nf, x, y, rw, rh)
        tx0, ty0, ntx, nty = pl["tile_x"], pl["tile_y"], pl["tiles_x"], pl["tiles_y"]
        pay = 8 * depth3[:nf, ty0:ty0 + nty, tx0:tx0 + ntx].sum().item()
        pre = nf * nty * (tx0 % 512 if pl["chunk_pieces"] else 0)
        return nf * T + nf * ntx * nty * 3 + pre + pay + 2 * nf * rw * rh

    lines = []
    full_out = torch.empty((n, H, W), dtype=torch.int16, device="cuda")
    for nf in (n, 1):
        full_ms = timed(lambda: codec.decode_frames16(buf, 32, stream_bytes, offs[:nf], W, H, nf, images=full_out[:nf]),
                        a.steps, a.warmup)
        codec.sync()
        assert torch.equal(full_out[:nf], imgs[:nf]), "full decode differs from the images"
        fb = frame_bytes if nf == n else sizes[:1].double().sum().item()
        full_touch = fb + 2 * nf * W * H
        base = dict(W=W, H=H, content="depth 0-16 per tile", frames_per_call=nf, lib=a.tag)
        lines.append(dict(base, case="decode_frames16", ms=full_ms, touched_bytes=int(full_touch),
                          share_of_peak=full_touch / (full_ms * 1e-3) / PEAK, vs_full=1.0))
        wins = [("256x256", 1000, 700, 256, 256), ("512x512", 1000, 700, 512, 512), ("1024x1024", 1000, 700, 1024, 1024),
                ("full", 0, 0, W, H)]
        for name, x, y, rw, rh in wins:
            out = torch.empty((nf, rh, rw), dtype=torch.int16, device="cuda")
            ms = timed(lambda: codec.decode_roi16(buf, 32, stream_bytes, offs[:nf], W, H, nf, x, y, rw, rh, out=out),
                       a.steps, a.warmup)
            codec.sync()
            assert torch.equal(out, imgs[:nf, y:y + rh, x:x + rw]), f"window {name} differs from the images"
            tb = roi_bytes(nf, x, y, rw, rh)
            lines.append(dict(base, case=f"decode_roi16 {name} at ({x},{y})", ms=ms, touched_bytes=int(tb),
                              share_of_peak=tb / (ms * 1e-3) / PEAK, vs_full=ms / full_ms))
            del out
    for ln in lines:
        print(json.dumps(ln), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    codec.close()


if __name__ == "__main__":
    main()
