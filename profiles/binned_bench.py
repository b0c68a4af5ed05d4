"""Binned decode (dbde_hip_decode_binned) against decoding the batch and pooling the images in torch;
profiles/hist_bench.py's method.

    python profiles/binned_bench.py [--rounds 3] [--seconds 0.4] [--out profiles/binned_bench.jsonl]

Datasets (encoded on the device, one slot per frame): 1,024 4096x3072 frames each of mixed, noise8 and smooth
content, and 128 4096x3072 DBDE16 frames with per-tile depths uniform in 0..16 (project16_bench.py's mixed16).
Arms, timed with device events over repeated calls (at least --seconds of work per figure, after a warm-up),
alternated round by round so that the spread shows:
  a         decode_frames alone
  b2 b4 b8  decode_frames + torch pooling to the sum plane: view(n, H/b, b, W/b, b).sum((2, 4)) in the plane's type,
            in sub-batches of 128 frames
  b4all     ... to all three planes (sum, amax, amin), b = 4
  c2 c4 c8  decode_binned, full frame, sum only
  c4all     decode_binned, full frame, all three planes, b = 4
  d         decode_binned, b = 4, sum only, of the 1024x1024 window at (1000, 700)
  e         decode_roi of that window
  f         decode_roi of the full frame
Prints one JSON line per (dataset, arm, round): ms per call and reps; the c arms also carry the bytes the kernel has to
move (the frames' encoded bytes + the plane bytes) and that over the time as a share of 8 TB/s.  Every plane is
checked once against the torch pooling of the decoded frames before any timing.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "profiles"))

from hist_bench import encode, timed   # noqa: E402

WIN = (1000, 700, 1024, 1024)
SUB = 128
PEAK = 8e12   # bytes per second


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--seconds", type=float, default=0.4)
    ap.add_argument("--only", default=None, help="one dataset: mixed4k, noise4k, smooth4k or mixed16_4k")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    import torch
    import dbde_video_cpp_amd as dv

    codec = dv.Codec(0)
    datasets = [("mixed4k", "mixed", 4096, 3072, 1024, 1), ("noise4k", "noise8", 4096, 3072, 1024, 1),
                ("smooth4k", "smooth", 4096, 3072, 1024, 1), ("mixed16_4k", "mixed16", 4096, 3072, 128, 2)]
    lines = []
    for name, content, W, H, n, pix in datasets:
        if a.only and name != a.only:
            continue
        buf, offs, stream_bytes = encode(codec, dv, content, W, H, n, pix)
        images = torch.empty((n, H, W), dtype=torch.uint8 if pix == 1 else torch.int16, device="cuda")
        res = torch.empty((n, 4), dtype=torch.int64, device="cuda")
        sum_t, mm_t = (torch.int16, torch.uint8) if pix == 1 else (torch.int32, torch.int16)
        dec_frames, dec_roi, dec_binned = (codec.decode_frames, codec.decode_roi, codec.decode_binned) if pix == 1 else \
                                          (codec.decode_frames16, codec.decode_roi16, codec.decode_binned16)

        def decode():
            if pix == 1:
                dec_frames(buf, 0, stream_bytes, offs, W, H, n, images=images, results=res)
            else:
                dec_frames(buf, 0, stream_bytes, offs, W, H, n, images=images)

        def pool(b, out, stats):
            """torch pooling of `images` into out's planes, SUB frames at a time."""
            for f0 in range(0, n, SUB):
                v = images[f0:f0 + SUB]
                if pix == 2:
                    v = v.to(torch.int32) & 0xFFFF   # the U16 values
                v = v.view(v.shape[0], H // b, b, W // b, b)
                if "sum" in stats:
                    out.sum[f0:f0 + SUB] = v.sum((2, 4), dtype=sum_t)
                if "max" in stats:
                    out.max[f0:f0 + SUB] = v.amax((2, 4)).to(mm_t)
                if "min" in stats:
                    out.min[f0:f0 + SUB] = v.amin((2, 4)).to(mm_t)

        ALL = ("sum", "max", "min")
        ref = {b: dv.Binned.empty(n, H, W, b, ALL if b == 4 else ("sum",), "cuda", pix=pix) for b in (2, 4, 8)}
        got = {b: dv.Binned.empty(n, H, W, b, ("sum",), "cuda", pix=pix) for b in (2, 4, 8)}
        got_all = dv.Binned.empty(n, H, W, 4, ALL, "cuda", pix=pix)
        x, y, rw, rh = WIN
        got_win = dv.Binned.empty(n, rh, rw, 4, ("sum",), "cuda", pix=pix)
        roi = torch.empty((n, rh, rw), dtype=images.dtype, device="cuda")

        def torch_arm(b, stats):
            def fn():
                decode()
                pool(b, ref[b], stats)
            return fn

        def binned_arm(b, out, win=(0, 0, W, H)):
            return lambda: dec_binned(buf, 0, stream_bytes, offs, W, H, n, b, *win, out=out, results=res)

        arms = [("a decode_frames", decode)]
        arms += [(f"b{b} decode_frames + torch sum pooling", torch_arm(b, ("sum",))) for b in (2, 4, 8)]
        arms += [("b4all decode_frames + torch sum/amax/amin pooling", torch_arm(4, ALL))]
        arms += [(f"c{b} decode_binned sum", binned_arm(b, got[b])) for b in (2, 4, 8)]
        arms += [("c4all decode_binned sum/max/min", binned_arm(4, got_all)),
                 ("d decode_binned b4 sum 1024x1024 window", binned_arm(4, got_win, WIN)),
                 ("e decode_roi 1024x1024 window", lambda: dec_roi(buf, 0, stream_bytes, offs, W, H, n, *WIN, out=roi,
                                                                   results=res)),
                 ("f decode_roi full frame", lambda: dec_roi(buf, 0, stream_bytes, offs, W, H, n, 0, 0, W, H,
                                                             out=images, results=res))]
        # check every plane once against the torch pooling of the decoded frames
        for _, fn in arms:
            fn()
        decode()
        for b in (2, 4, 8):
            pool(b, ref[b], ALL if b == 4 else ("sum",))
        codec.sync()
        for b in (2, 4, 8):
            assert torch.equal(got[b].sum, ref[b].sum), (name, b)
        assert all(torch.equal(getattr(got_all, s), getattr(ref[4], s)) for s in ALL), name
        wv = images[:, y:y + rh, x:x + rw]
        wv = wv if pix == 1 else wv.to(torch.int32) & 0xFFFF
        assert torch.equal(got_win.sum, wv.reshape(n, rh // 4, 4, rw // 4, 4).sum((2, 4), dtype=sum_t)), name
        assert torch.equal(roi, images[:, y:y + rh, x:x + rw]), name
        encoded = int(res[:, 3].sum().item())   # the bytes of the frames themselves (slots are larger)
        need = {f"c{b} decode_binned sum": encoded + n * (H // b) * (W // b) * 2 * pix for b in (2, 4, 8)}
        need["c4all decode_binned sum/max/min"] = encoded + n * (H // 4) * (W // 4) * 4 * pix
        for _, fn in arms:   # warm-up
            fn()
        codec.sync()
        for rnd in range(a.rounds):
            order = arms if rnd % 2 == 0 else arms[::-1]
            for arm, fn in order:
                ms, reps = timed(fn, a.seconds)
                ln = dict(dataset=name, content=content, W=W, H=H, frames=n, arm=arm, round=rnd, reps=reps, ms=ms,
                          measured=True)
                if arm in need:
                    ln.update(encoded_bytes=encoded, bytes_needed=need[arm],
                              share_of_8TBps=need[arm] / (ms * 1e-3) / PEAK)
                print(json.dumps(ln), flush=True)
                lines.append(ln)
        del buf, images, ref, got, got_all, got_win, roi
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    codec.close()


if __name__ == "__main__":
    main()
