"""Grouped projections (dbde_hip_project_groups) against one dbde_hip_project call per group and against decoding the
batch and reducing the images in torch.

    python profiles/gproject_bench.py [--rounds 3] [--seconds 0.6] [--only mixed4k] [--groups n,64,8,2]
                                      [--out profiles/gproject_bench.jsonl]

Datasets (each encoded on the device into one slot per frame): 1,024 mixed and 1,024 noise8 4096x3072 frames, 128
full-range DBDE16 4096x3072 frames, and 262,144 mixed 64x64 frames.
Settings: groups of g frames, g in {n, 64, 8, 2} (n: one group, or groups of 65,536, the most a group may hold, for
the 64x64 batch); all four statistics, the sum only (a U16 plane where the call allows
it -- DBDE, g <= 257 -- else U32) and max + min.
Arms, timed in the same run with device events over repeated calls (at least --seconds of work per figure, after a
warm-up) and alternated round by round so that the spread shows:
  a  project_groups
  b  one project call per group (every call writes the same set of planes, which spares (b) the planes' footprint but
     not their traffic)
  c  decode_frames + torch reductions over view(n / g, g, H, W), a chunk of groups at a time (the reduced planes of a
     chunk are dropped, not kept)
Prints one JSON line per (dataset, g, statistics, arm, round):
  ms             time of one pass over the whole batch
  read_bytes     the frames' bytes (c also reads the images back once)
  written_bytes  a: the planes and counts it writes; b: the planes project writes (U64 sums); c: the images
  share_of_peak  (read_bytes + written_bytes) / time against 8 TB/s
Before any timing, the first groups and the last one of (a) are compared with (b)'s projection of the same frames.
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
SETS = [("all four", ALL), ("sum", ("sum",)), ("max+min", ("max", "min"))]


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
    ap.add_argument("--only", default=None, help="one dataset: mixed4k, noise4k, u16 or small")
    ap.add_argument("--groups", default="n,64,8,2", help="group sizes, n = the whole batch")
    ap.add_argument("--arms", default="abc")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    import torch
    import dbde_video_cpp_amd as dv

    codec = dv.Codec(0)
    datasets = [("mixed4k", "mixed", 1, 4096, 3072, 1024), ("noise4k", "noise8", 1, 4096, 3072, 1024),
                ("u16", "full", 2, 4096, 3072, 128), ("small", "mixed", 1, 64, 64, 262144)]
    out_file = open(a.out, "a") if a.out else None
    for name, content, pix, W, H, n in datasets:
        if a.only and name != a.only:
            continue
        maxf = dv.max_frame_bytes(W, H) if pix == 1 else int(codec.L.dbde16_hip_max_frame_bytes(W, H))
        slot = (maxf + 255) // 256 * 256
        buf = torch.empty(n * slot + 256, dtype=torch.uint8, device="cuda")
        offs = torch.empty(n, dtype=torch.int64, device="cuda")
        sizes = torch.empty(n, dtype=torch.int64, device="cuda")
        step = max(1, min(n, (1 << 28) // (W * H)))
        gen = torch.Generator(device="cuda").manual_seed(16)
        for f0 in range(0, n, step):   # synthesize and encode a piece at a time
            k = min(step, n - f0)
            if pix == 1:
                imgs = codec.synth_frames(content, 0xDBDE2016, f0, k, W, H)
                o, s = codec.encode_frames(imgs, W, H, k, buf, f0 * slot, (n - f0) * slot, first_index=f0,
                                           slot_stride=slot)
            else:
                imgs = torch.randint(-32768, 32768, (k, H, W), dtype=torch.int16, device="cuda", generator=gen)
                o, s = codec.encode_frames16(imgs, W, H, k, buf, f0 * slot, (n - f0) * slot, first_index=f0,
                                             slot_stride=slot)
            offs[f0:f0 + k] = o + f0 * slot
            sizes[f0:f0 + k] = s
            del imgs
        codec.sync()
        stream_bytes = n * slot
        frame_bytes = int(sizes.sum().item())
        res = torch.empty((n, 4), dtype=torch.int64, device="cuda")
        img_dtype = torch.uint8 if pix == 1 else torch.int16
        groups_fn = codec.project_groups if pix == 1 else codec.project_groups16
        project_fn = codec.project if pix == 1 else codec.project16
        decode_fn = codec.decode_frames if pix == 1 else codec.decode_frames16
        images = None

        for gname in a.groups.split(","):
            g = min(n, 65536) if gname == "n" else int(gname)   # (a group holds at most 65,536 frames)
            ng = -(-n // g)
            for sname, stats in SETS:
                sum_dtype = torch.int16 if (pix == 1 and g <= 257 and stats == ("sum",)) else torch.int32
                gp = dv.GroupProjection.empty(ng, H, W, stats, "cuda", pix=pix, sum_dtype=sum_dtype)
                pr = dv.Projection.empty(H, W, stats, "cuda", pix=pix)
                P = ng * W * H
                wa = sum(P * sz for s, sz in (("max", pix), ("min", pix), ("sum", 2 if sum_dtype == torch.int16 else 4),
                                              ("sumsq", 8)) if s in stats) + 4 * ng
                wb = sum(P * sz for s, sz in (("max", pix), ("min", pix), ("sum", 8), ("sumsq", 8)) if s in stats)

                def arm_a():
                    groups_fn(buf, 0, stream_bytes, offs, W, H, n, group_frames=g, out=gp, results=res)

                def arm_b():
                    for k in range(ng):
                        lo, hi = k * g, min((k + 1) * g, n)
                        project_fn(buf, 0, stream_bytes, offs[lo:hi], W, H, hi - lo, out=pr, results=res[lo:hi])

                chunk = max(1, min(n, (1 << 26) // (W * H)))   # frames reduced at a time

                def reduce(x, dim):
                    v = x if pix == 1 else x.to(torch.int32) & 0xFFFF   # int16 tensors hold the U16 bits
                    x64 = v.to(torch.int64) if ("sum" in stats or "sumsq" in stats) else None
                    out = []
                    if "max" in stats:
                        out.append(v.amax(dim))
                    if "min" in stats:
                        out.append(v.amin(dim))
                    if "sum" in stats:
                        out.append(x64.sum(dim))
                    if "sumsq" in stats:
                        out.append((x64 * x64).sum(dim))
                    return out

                def arm_c():
                    nonlocal images
                    if images is None:
                        images = torch.empty((n, H, W), dtype=img_dtype, device="cuda")
                    decode_fn(buf, 0, stream_bytes, offs, W, H, n, images=images)
                    if g <= chunk:
                        cg = chunk // g
                        whole = n // g
                        for k0 in range(0, whole, cg):
                            k1 = min(k0 + cg, whole)
                            reduce(images[k0 * g:k1 * g].view(k1 - k0, g, H, W), 1)
                        if whole * g < n:
                            reduce(images[whole * g:], 0)
                    else:
                        for k in range(ng):
                            acc = None
                            for f0 in range(k * g, min((k + 1) * g, n), chunk):
                                part = reduce(images[f0:min(f0 + chunk, (k + 1) * g, n)], 0)
                                if acc is None:
                                    acc = part
                                else:
                                    for i, s in enumerate(stats):
                                        acc[i] = (torch.maximum(acc[i], part[i]) if s == "max" else
                                                  torch.minimum(acc[i], part[i]) if s == "min" else acc[i] + part[i])

                arms = [(k, fn) for k, fn in (("a project_groups", arm_a), ("b project per group", arm_b),
                                              ("c decode_frames + torch", arm_c)) if k[0] in a.arms]

                # (a) against (b): the first groups and the last one
                arm_a()
                for k in sorted({0, 1, ng // 2, ng - 1} & set(range(ng))):
                    lo, hi = k * g, min((k + 1) * g, n)
                    project_fn(buf, 0, stream_bytes, offs[lo:hi], W, H, hi - lo, out=pr)
                    codec.sync()
                    assert int(gp.counts[k].item()) == int(pr.count.item()) == hi - lo, (name, g, k)
                    for s in stats:
                        x, y = getattr(gp, s)[k], getattr(pr, s)
                        if s == "sum":
                            x = gp.sums()[k]
                        assert torch.equal(x.to(torch.int64), y.to(torch.int64)), (name, g, sname, s, k)

                rb = {"a": frame_bytes, "b": frame_bytes, "c": frame_bytes + n * W * H * pix}
                wr = {"a": wa, "b": wb, "c": n * W * H * pix}
                for _, fn in arms:   # warm-up
                    fn()
                codec.sync()
                for rnd in range(a.rounds):
                    order = arms if rnd % 2 == 0 else arms[::-1]
                    for arm, fn in order:
                        ms, reps = timed(fn, a.seconds)
                        k = arm[0]
                        ln = dict(dataset=name, content=content, W=W, H=H, frames=n, group_frames=g, groups=ng,
                                  stats=sname, sum_type="U16" if sum_dtype == torch.int16 else "U32", arm=arm,
                                  round=rnd, reps=reps, ms=ms, read_bytes=rb[k], written_bytes=wr[k],
                                  share_of_peak=(rb[k] + wr[k]) / (ms * 1e-3) / PEAK, measured=True)
                        print(json.dumps(ln), flush=True)
                        if out_file:
                            out_file.write(json.dumps(ln) + "\n")
                            out_file.flush()
                del gp, pr
                torch.cuda.empty_cache()
        del buf, images
        torch.cuda.empty_cache()
    if out_file:
        out_file.close()
    codec.close()


if __name__ == "__main__":
    main()
