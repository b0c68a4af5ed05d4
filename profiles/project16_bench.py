"""DBDE16 temporal projections (dbde16_hip_project) against decoding the batch and reducing the images in torch;
profiles/project_bench.py's method on 16-bit frames.

    python profiles/project16_bench.py [--rounds 3] [--seconds 0.6] [--out profiles/project16_bench.jsonl]

Datasets (generated and encoded on the device, one slot per frame): 128 4096x3072 frames with per-tile depths uniform
in 0..16 ("mixed16"), 128 4096x3072 frames of depth 16 everywhere ("depth16"), and 2,048 1024x768 mixed16 frames.
Arms, timed with device events over repeated calls (at least --seconds of work per figure, after a warm-up),
alternated round by round:
  a  decode_frames16 alone
  b  decode_frames16 + torch reductions to max, min, sum and sum of squares (int64, in chunks)
  c  project16, all four statistics
  d  project16, max and min only
  e  project16 of a 512x512 window
Prints one JSON line per (dataset, arm, round): ms, read_bytes (the frames' bytes; b also reads the images back once;
e the depth arrays, the window tiles' minima, the depth bytes in front of each window tile row within its index chunk
and the window tiles' payload), written_bytes (images for a, b) and share_of_peak against 8 TB/s.
The projections are checked once against the torch reductions (b) of the same frames before any timing.
"""
import argparse
import json
import math
import os
import sys

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


def frames16(kind, k, W, H, gen):
    """k (H, W) frames as an int16 device tensor of U16 bits.  mixed16: a depth uniform in 0..16 per 8x8 tile (a tile
    base plus d random bits); depth16: random values with 0 and 65535 in every tile."""
    import torch
    h, w = (H + 7) // 8, (W + 7) // 8
    up = lambda t: t.repeat_interleave(8, 1).repeat_interleave(8, 2)[:, :H, :W]   # noqa: E731
    noise = torch.randint(0, 65536, (k, H, W), dtype=torch.int32, device="cuda", generator=gen)
    if kind == "depth16":
        noise[:, 0::8, 0::8] = 0
        noise[:, 7::8, 7::8] = 65535
        img = noise
    else:
        mask = up((1 << torch.randint(0, 17, (k, h, w), dtype=torch.int32, device="cuda", generator=gen)) - 1)
        base = up(torch.randint(0, 65536, (k, h, w), dtype=torch.int32, device="cuda", generator=gen))
        img = torch.minimum(base >> 1, 65535 - mask) + (noise & mask)
    return img.to(torch.int16)   # (two's complement: the low 16 bits)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.6)
    ap.add_argument("--only", default=None, help="one dataset: mixed16_4k, depth16_4k or mixed16_1k")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    import torch
    import dbde_video_cpp_amd as dv

    codec = dv.Codec(0)
    gen = torch.Generator(device="cuda").manual_seed(0xDBDE16)
    datasets = [("mixed16_4k", "mixed16", 4096, 3072, 128), ("depth16_4k", "depth16", 4096, 3072, 128),
                ("mixed16_1k", "mixed16", 1024, 768, 2048)]
    lines = []
    for name, content, W, H, n in datasets:
        if a.only and name != a.only:
            continue
        w, h = (W + 7) // 8, (H + 7) // 8
        T = w * h
        slot = (int(codec.L.dbde16_hip_max_frame_bytes(W, H)) + 255) // 256 * 256
        buf = torch.empty(n * slot + 256, dtype=torch.uint8, device="cuda")
        offs = torch.empty(n, dtype=torch.int64, device="cuda")
        sizes = torch.empty(n, dtype=torch.int64, device="cuda")
        step = max(1, min(n, (1 << 26) // (W * H)))
        for f0 in range(0, n, step):   # generate and encode in groups
            k = min(step, n - f0)
            imgs = frames16(content, k, W, H, gen)
            o, s = codec.encode_frames16(imgs, W, H, k, buf, f0 * slot, (n - f0) * slot, first_index=f0,
                                         slot_stride=slot)
            offs[f0:f0 + k] = o + f0 * slot
            sizes[f0:f0 + k] = s
            del imgs
        codec.sync()
        stream_bytes = n * slot
        frame_bytes = int(sizes.sum().item())
        images = torch.empty((n, H, W), dtype=torch.int16, device="cuda")
        res = torch.empty((n, 4), dtype=torch.int64, device="cuda")

        def decode():
            codec.decode_frames16(buf, 0, stream_bytes, offs, W, H, n, images=images)

        ref = {s: None for s in ALL}
        chunk = max(1, min(n, (1 << 25) // (W * H)))

        def decode_reduce():
            decode()
            mx = mn = sm = sq = None
            for f0 in range(0, n, chunk):
                x64 = images[f0:f0 + chunk].to(torch.int64) & 0xFFFF
                a_, b_, c_, d_ = x64.amax(0), x64.amin(0), x64.sum(0), (x64 * x64).sum(0)
                mx = a_ if mx is None else torch.maximum(mx, a_)
                mn = b_ if mn is None else torch.minimum(mn, b_)
                sm = c_ if sm is None else sm + c_
                sq = d_ if sq is None else sq + d_
            ref.update(max=mx, min=mn, sum=sm, sumsq=sq)

        proj_all = dv.Projection.empty(H, W, ALL, "cuda", pix=2)
        proj_mm = dv.Projection.empty(H, W, ("max", "min"), "cuda", pix=2)
        win = (1000, 700, 512, 512) if W >= 1512 else (0, 0, 512, 512)
        proj_win = dv.Projection.empty(512, 512, ALL, "cuda", pix=2)
        arms = [("a decode_frames16", decode), ("b decode_frames16 + torch reductions", decode_reduce),
                ("c project16 all four", lambda: codec.project16(buf, 0, stream_bytes, offs, W, H, n, out=proj_all,
                                                                 results=res)),
                ("d project16 max+min", lambda: codec.project16(buf, 0, stream_bytes, offs, W, H, n, out=proj_mm,
                                                                results=res)),
                ("e project16 512x512 window", lambda: codec.project16(buf, 0, stream_bytes, offs, W, H, n, *win,
                                                                       out=proj_win, results=res))]

        # check the projections against the torch reductions once
        decode_reduce()
        for _, fn in arms[2:]:
            fn()
        codec.sync()
        u16 = lambda t: t.to(torch.int64) & 0xFFFF   # noqa: E731
        assert int(proj_all.count.item()) == n
        for s in ALL:
            got = getattr(proj_all, s)
            assert torch.equal(u16(got) if s in ("max", "min") else got, ref[s]), (name, s)
        assert torch.equal(u16(proj_mm.max), ref["max"]) and torch.equal(u16(proj_mm.min), ref["min"])
        x, y, rw, rh = win
        assert torch.equal(proj_win.sumsq, ref["sumsq"][y:y + rh, x:x + rw])

        # bytes each arm must read / write
        depth = torch.empty((n, T), dtype=torch.uint8, device="cuda")
        ar = torch.arange(T, device="cuda")
        dstep = max(1, min(n, (1 << 26) // T))
        for f0 in range(0, n, dstep):
            k = min(dstep, n - f0)
            depth[f0:f0 + k] = buf[(offs[f0:f0 + k, None] + 24 + ar[None, :]).reshape(-1)].view(k, T)
        img_bytes = 2 * n * W * H
        rb = {"a": frame_bytes, "b": frame_bytes + img_bytes, "c": frame_bytes, "d": frame_bytes}
        wb = {"a": img_bytes, "b": img_bytes, "c": 0, "d": 0}
        pl = dv.project16_plan(W, H, n, *win)
        tx0, ty0, ntx, nty = pl["tile_x"], pl["tile_y"], pl["tiles_x"], pl["tiles_y"]
        pay = 8 * int(depth.view(n, h, w)[:, ty0:ty0 + nty, tx0:tx0 + ntx].to(torch.int64).sum().item())
        pre = n * nty * (tx0 % 512 if pl["chunk_pieces"] else 0)
        rb["e"], wb["e"] = n * T + 2 * n * ntx * nty + pre + pay, 0
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
        del buf, images, proj_all, proj_mm, proj_win, ref
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    codec.close()


if __name__ == "__main__":
    main()
