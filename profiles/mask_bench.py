"""Threshold mask decode (dbde_hip_decode_mask) against decoding the window and comparing it in torch.

    python profiles/mask_bench.py [--rounds 3] [--seconds 0.3] [--only mixed4k] [--out profiles/mask_bench.jsonl]

Datasets (each encoded on the device into one slot per frame): 1,024 mixed and 1,024 noise8 4096x3072 DBDE frames, and
128 DBDE16 4096x3072 frames (16, 12, 8 and 4 significant bits, frame by frame).  For each dataset: the full frame,
1024x1024 and 256x256 windows at (1000, 696), and the full frame with one frame per call.  Thresholds:
  most   a scalar band at the top of the range (a saturation check): the tiles whose range lies below it are decided by
         their two header bytes
  none   a scalar band through the middle of the range
  maps   both thresholds from [H][W] maps (only depth-0 tiles skip their payload)
every line carries decided_share, the share of the window's tiles of depth > 0 that the decided-tile rule settles.
Arms, all in one process, timed with device events over repeated calls (at least --seconds of work per figure, after a
warm-up), alternated round by round so that the spread shows:
  a  decode_mask with counts (index, initialisation and mask kernel)
  b  the path it replaces: decode_roi, then (w >= lo) & (w <= hi) and .sum((1, 2)) in torch (DBDE16: the int16 tensor
     the decoder writes holds U16 bits; it is compared as uint16 where the installed torch can, else through
     int32 & 0xFFFF, which costs arm b two more passes; every u16 line says which in "widen")
  c  decode_roi alone: the floor of path b
(c is timed in the rounds of the "most" case only: it does not depend on the thresholds.)
Arm a's bits and counts are checked against arm b's (the first frames of the call) before any timing.
Prints one JSON line per (dataset, window, thresholds, arm, round), and with --out appends each line to that file as it
is measured.
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H = 4096, 3072
WINDOWS = [("full", (0, 0, W, H), None), ("1024", (1000, 696, 1024, 1024), None), ("256", (1000, 696, 256, 256), None),
           ("full x1", (0, 0, W, H), 1)]


def timed(fn, seconds):
    """ms per call over at least `seconds` of calls (device events around the whole run)."""
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):   # the call that sizes reps is a warmed one
        fn()
    a.record()
    fn()
    b.record()
    b.synchronize()
    one = max(a.elapsed_time(b), 1e-3)   # (includes the events' own cost: a short call is over-estimated)
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
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--only", default=None, help="one dataset: mixed4k, noise4k or u16")
    ap.add_argument("--frames", type=int, default=0, help="frames per dataset (default 1024; u16: 128)")
    ap.add_argument("--out", default=None, help="also append each JSON line to this file as it is measured")
    a = ap.parse_args()

    import torch
    import dbde_video_cpp_amd as dv

    codec = dv.Codec(0)
    w, h = W // 8, H // 8
    T = w * h
    g = torch.Generator(device="cuda").manual_seed(2016)
    sink = open(a.out, "a") if a.out else None
    try:   # does this torch compare uint16 on the device?  (not every build has the kernel)
        _ = torch.zeros(4, dtype=torch.int16, device="cuda").view(torch.uint16) >= 3
        widen = "uint16"
    except (RuntimeError, TypeError, AttributeError):
        widen = "int32"
    for name, content, pix, n_all in (("mixed4k", "mixed", 1, 1024), ("noise4k", "noise8", 1, 1024), ("u16", "u16", 2, 128)):
        if a.only and name != a.only:
            continue
        n_all = a.frames or n_all
        top = 255 if pix == 1 else 65535
        maxf = dv.max_frame_bytes(W, H) if pix == 1 else int(codec.L.dbde16_hip_max_frame_bytes(W, H))
        slot = (maxf + 255) // 256 * 256
        buf = torch.empty(n_all * slot + 256, dtype=torch.uint8, device="cuda")
        offs = torch.empty(n_all, dtype=torch.int64, device="cuda")
        step = 16
        for f0 in range(0, n_all, step):   # synthesize and encode in groups
            if pix == 1:
                imgs = codec.synth_frames(content, 0xDBDE2016, f0, step, W, H)
                o, _ = codec.encode_frames(imgs, W, H, step, buf, f0 * slot, (n_all - f0) * slot, first_index=f0,
                                           slot_stride=slot)
            else:
                imgs = torch.randint(-32768, 32768, (step, H, W), dtype=torch.int16, device="cuda", generator=g)
                for k in range(step):   # 16, 12, 8 and 4 significant bits, frame by frame
                    imgs[k] = ((imgs[k].to(torch.int32) & 0xFFFF) >> (4 * (k % 4))).to(torch.int16)
                o, _ = codec.encode_frames16(imgs, W, H, step, buf, f0 * slot, (n_all - f0) * slot, first_index=f0,
                                             slot_stride=slot)
            offs[f0:f0 + step] = o + f0 * slot
            del imgs
        codec.sync()
        stream_bytes = n_all * slot
        roi = codec.decode_roi if pix == 1 else codec.decode_roi16
        mask_fn = codec.decode_mask if pix == 1 else codec.decode_mask16
        plan = dv.mask_plan if pix == 1 else dv.mask16_plan
        ar = torch.arange(T, device="cuda")
        depth = torch.empty((n_all, T), dtype=torch.int32, device="cuda")
        mins = torch.empty((n_all, T), dtype=torch.int32, device="cuda")
        for f0 in range(0, n_all, 16):   # the depth and minimum of every tile, for decided_share
            at = offs[f0:f0 + 16, None]
            depth[f0:f0 + 16] = buf[(at + 24 + ar[None, :]).reshape(-1)].view(16, T).to(torch.int32)
            if pix == 1:
                mins[f0:f0 + 16] = buf[(at + 28 + T + ar[None, :]).reshape(-1)].view(16, T).to(torch.int32)
            else:
                lo8 = buf[(at + 28 + T + 2 * ar[None, :]).reshape(-1)].view(16, T).to(torch.int32)
                hi8 = buf[(at + 29 + T + 2 * ar[None, :]).reshape(-1)].view(16, T).to(torch.int32)
                mins[f0:f0 + 16] = lo8 | (hi8 << 8)
        depth, mins = depth.view(n_all, h, w), mins.view(n_all, h, w)
        lo_map = torch.randint(0, top // 2, (H, W), device="cuda", generator=g)
        hi_map = lo_map + torch.randint(0, top // 2, (H, W), device="cuda", generator=g)
        as_pix = (lambda t: t.to(torch.uint8)) if pix == 1 else (lambda t: torch.where(t > 32767, t - 65536, t).to(torch.int16))
        cases = [("most", top - top // 50, top, None, None), ("none", top * 2 // 5, top * 3 // 5, None, None),
                 ("maps", 0, top, as_pix(lo_map).contiguous(), as_pix(hi_map).contiguous())]

        for wname, (x, y, rw, rh), per_call in WINDOWS:
            n = per_call or n_all
            ofs = offs[:n].contiguous()
            pdt = torch.uint8 if pix == 1 else torch.int16
            pixels = torch.empty((n, rh, rw), dtype=pdt, device="cuda")
            res = torch.empty((n, 4), dtype=torch.int64, device="cuda")
            out = dv.Mask.empty(n, rh, rw, "cuda", counts=True)
            pl = plan(W, H, n, x, y, rw, rh)
            tx0, ty0, ntx, nty = pl["tile_x"], pl["tile_y"], pl["tiles_x"], pl["tiles_y"]
            dw = depth[:n, ty0:ty0 + nty, tx0:tx0 + ntx]
            mw = mins[:n, ty0:ty0 + nty, tx0:tx0 + ntx]

            def decode():
                roi(buf, 0, stream_bytes, ofs, W, H, n, x, y, rw, rh, out=pixels, results=res)

            for cname, lo0, hi0, lom, him in cases:
                lo = lo0 if lom is None else lom
                hi = hi0 if him is None else him
                if lom is None:
                    low, hiw = lo0, hi0
                elif pix == 1:
                    low, hiw = lom[y:y + rh, x:x + rw], him[y:y + rh, x:x + rw]
                elif widen == "uint16":
                    low, hiw = lom.view(torch.uint16)[y:y + rh, x:x + rw], him.view(torch.uint16)[y:y + rh, x:x + rw]
                else:
                    low, hiw = lo_map[y:y + rh, x:x + rw].to(torch.int32), hi_map[y:y + rh, x:x + rw].to(torch.int32)
                tp = mw + torch.bitwise_left_shift(torch.ones_like(dw), dw) - 1
                if lom is None:
                    dec = (dw > 0) & (tp <= top) & (((mw >= lo0) & (tp <= hi0)) | (tp < lo0) | (mw > hi0))
                    decided = float(dec.sum().item()) / max(1, int((dw > 0).sum().item()))
                else:
                    decided = 0.0
                holder = {}

                def arm_a():
                    mask_fn(buf, 0, stream_bytes, ofs, W, H, n, x, y, rw, rh, lo=lo, hi=hi, mask=out, results=res)

                def arm_b():
                    decode()
                    if pix == 1:
                        p = pixels
                    elif widen == "uint16":
                        p = pixels.view(torch.uint16)
                    else:
                        p = pixels.to(torch.int32) & 0xFFFF
                    m = (p >= low) & (p <= hiw)
                    holder["m"], holder["c"] = m, m.sum((1, 2))

                arms = [("a decode_mask", arm_a), ("b decode_roi + torch", arm_b)]
                if cname == "most":   # c does not depend on the thresholds: once per window
                    arms += [("c decode_roi alone", decode)]
                arm_a()
                arm_b()
                codec.sync()
                k = min(n, 4)
                assert torch.equal(dv.Mask(out.bits[:k], rw=rw).unpack(), holder["m"][:k]), (name, wname, cname)
                assert torch.equal(out.counts.long(), holder["c"]), (name, wname, cname)
                holder.clear()
                for _, fn in arms:   # warm-up
                    fn()
                codec.sync()
                for rnd in range(a.rounds):
                    order = arms if rnd % 2 == 0 else arms[::-1]
                    for arm, fn in order:
                        ms, reps = timed(fn, a.seconds)
                        ln = dict(dataset=name, window=wname, x=x, y=y, rw=rw, rh=rh, frames=n, thresholds=cname,
                                  decided_share=round(decided, 4), arm=arm, round=rnd, reps=reps, ms=ms, measured=True)
                        if pix == 2 and arm[0] == "b":
                            ln.update(widen=widen)
                        print(json.dumps(ln), flush=True)
                        if sink:
                            sink.write(json.dumps(ln) + "\n")
                            sink.flush()
                holder.clear()
            del pixels, out
            torch.cuda.empty_cache()
        del buf, depth, mins
        torch.cuda.empty_cache()
    if sink:
        sink.close()
    codec.close()


if __name__ == "__main__":
    main()
