"""Pair projection (per-pixel sums of neighbour products, in one pass over the compressed stream) and the local
correlation image built on it, against the floor (project's sum and sumsq) and the only route there was without it.

    python profiles/pairs_bench.py [--only mixed4k|small|u16|corr] [--frames N] [--steps 10] [--warmup 2] [--out FILE]

Datasets: 1,024 mixed 4096x3072 frames (synth), 65,536 mixed 64x64 frames, 128 DBDE16 4096x3072 frames (16, 12, 8 and 4
significant bits, frame by frame).  Cases: the full frame, a 1024x1024 and a 256x256 window, one frame per call, the
small frames and the DBDE16 frames, each with the masks 1, 3 and 15.  Every arm of a case runs in this process on the same
inputs, `warmup` untimed calls and then `steps` timed ones between device events on the context's stream, the arms
interleaved call by call; the median is reported.  Arms:
  k   project_pairs (the timed output);
  b   project(stats=("sum", "sumsq")), the floor: the same frames reduced pixel by pixel, no halo;
  a   the same planes through pixels: decode_frames (the full frame) or decode_roi (a window) in chunks of frames that
      keep the decoded pixels at 2^28 at most, and per offset the product of two shifted int32 views summed over the
      chunk into int64 planes in torch.  chunk_frames and the arm's peak device memory on top of the stream are recorded.
One JSON line per case with the medians, the ratios, the per-plane cost over the floor ((k - b) / planes), the plan (pieces,
segments, instance) and the halo's share of the decoded data that the plan implies: tiles decoded as partners only
(pieces_x * piece_tiles against tiles_x) and the rows below (one row in eight of every tile row but the last, behind a
second offset prefix).  The check: the timed planes equal arm a's, element for element.

The corr case times correlation.correlation_image (8 neighbours) end to end against arm a's planes plus the same sum and
sumsq in torch and the Pearson arithmetic on them.
"""
import argparse
import json
import os
import sys
from importlib import import_module

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, help="one part: mixed4k, small, u16 or corr")
    ap.add_argument("--frames", type=int, default=0, help="frames per dataset (default 1024; small: 65536; u16: 128)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()

    import torch
    import dbde_video_cpp_amd as dv
    cor = import_module("dbde_video_cpp_amd.correlation")

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
        step = min(16 if W > 64 else 4096, n_all)
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

    def spans(dx, dy, rw, rh):
        return ((slice(None), slice(0, rh - dy), slice(max(0, -dx), rw - max(0, dx))),
                (slice(None), slice(dy, rh), slice(max(0, dx), rw - max(0, -dx))))

    class Pixels:
        """Arm a: the planes of `offsets` (and optionally sum / sumsq) of nf frames through decoded pixels."""

        def __init__(self, pix, buf, stream_bytes, offs, W, H, nf, win, offsets, moments=False):
            self.pix, self.buf, self.sb, self.offs, self.W, self.H, self.nf = pix, buf, stream_bytes, offs, W, H, nf
            self.win, self.offsets, self.moments = win, offsets, moments
            x, y, rw, rh = win
            self.whole = (rw, rh) == (W, H)
            self.chunk = max(1, min(nf, (1 << 28) // (rw * rh)))
            pdt = torch.uint8 if pix == 1 else torch.int16
            self.pixels = torch.empty((self.chunk, rh, rw), dtype=pdt, device="cuda")
            self.acc = torch.empty((len(offsets), rh, rw), dtype=torch.int64, device="cuda")
            self.sum = torch.empty((rh, rw), dtype=torch.int64, device="cuda") if moments else None
            self.sumsq = torch.empty((rh, rw), dtype=torch.int64, device="cuda") if moments else None

        def __call__(self):
            x, y, rw, rh = self.win
            self.acc.zero_()
            if self.moments:
                self.sum.zero_()
                self.sumsq.zero_()
            for f0 in range(0, self.nf, self.chunk):
                k = min(self.chunk, self.nf - f0)
                o = self.offs[f0:f0 + k]
                if self.whole and self.pix == 1:
                    codec.decode_frames(self.buf, 0, self.sb, o, self.W, self.H, k, images=self.pixels[:k])
                elif self.whole:
                    codec.decode_frames16(self.buf, 0, self.sb, o, self.W, self.H, k, images=self.pixels[:k])
                else:
                    roi = codec.decode_roi if self.pix == 1 else codec.decode_roi16
                    roi(self.buf, 0, self.sb, o, self.W, self.H, k, x, y, rw, rh, out=self.pixels[:k])
                px = self.pixels[:k].to(torch.int32)
                if self.pix == 2:
                    px &= 0xFFFF
                    px = px.to(torch.int64)      # a U16 product needs more than int32
                for j, (dx, dy) in enumerate(self.offsets):
                    sa, sb = spans(dx, dy, rw, rh)
                    self.acc[j][sa[1:]] += (px[sa] * px[sb]).sum(0, dtype=torch.int64)
                if self.moments:
                    self.sum += px.sum(0, dtype=torch.int64)
                    self.sumsq += (px * px).sum(0, dtype=torch.int64)
                del px

    def peak_of(fn):
        fn()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return int(torch.cuda.max_memory_allocated() - base)

    for name, pix, W, H, n_all in (("mixed4k", 1, 4096, 3072, 1024), ("small", 1, 64, 64, 65536), ("u16", 2, 4096, 3072, 128),
                                   ("corr", 1, 4096, 3072, 1024)):
        if a.only and a.only != name:
            continue
        n_all = a.frames or n_all
        buf, offs, stream_bytes = dataset(pix, W, H, n_all)
        pairs = codec.project_pairs if pix == 1 else codec.project_pairs16
        proj = codec.project if pix == 1 else codec.project16
        plan_fn = dv.pairs_plan if pix == 1 else dv.pairs16_plan
        res = torch.empty((n_all, 4), dtype=torch.int64, device="cuda")

        if name == "corr":
            win = (0, 0, W, H)
            px_arm = Pixels(pix, buf, stream_bytes, offs, W, H, n_all, win, dv.PAIR_OFFSETS, moments=True)
            state = {}

            def arm_image():
                state["k"] = cor.correlation_image(codec, buf, 0, stream_bytes, offs, W, H, n_all, neighbours=8)[0]

            def arm_pixels():
                px_arm()
                pp = dv.PairProjection(px_arm.acc, torch.full((1,), n_all, dtype=torch.int64, device="cuda"), dv.PAIR_OFFSETS)
                pr = dv.Projection(sum=px_arm.sum, sumsq=px_arm.sumsq, count=pp.count)
                state["a"] = cor.local_correlation(pp, pr)

            ms = timed(dict(k=arm_image, a=arm_pixels), a.steps, a.warmup)
            peak_k, peak_a = peak_of(arm_image), peak_of(arm_pixels)
            assert torch.equal(state["k"], state["a"]), "the image differs from the one through pixels"
            emit(dict(dataset=name, W=W, H=H, frames=n_all, neighbours=8, ms_correlation_image=ms["k"],
                      ms_pixels_route=ms["a"], pixels_route_over_image=ms["a"] / ms["k"], ms_image_minmax=ms["k_minmax"],
                      ms_pixels_route_minmax=ms["a_minmax"], chunk_frames=px_arm.chunk,
                      peak_bytes_correlation_image=peak_k, peak_bytes_pixels_route=peak_a, stream_bytes=int(stream_bytes),
                      decoded_bytes=int(n_all) * W * H * pix, equal=True))
            del px_arm, state, buf, offs
            continue

        if name == "mixed4k":
            wins = [(n_all, (0, 0, W, H)), (n_all, (1536, 1024, 1024, 1024)), (n_all, (1920, 1408, 256, 256)),
                    (1, (0, 0, W, H))]
        else:
            wins = [(n_all, (0, 0, W, H))]
        for nf, (x, y, rw, rh) in wins:
            for mask in (1, 3, 15):
                offsets = dv.pair_offsets(mask)
                o_f, r_f = offs[:nf], res[:nf]
                out = dv.PairProjection.empty(offsets, rh, rw, codec.device)
                pr = dv.Projection.empty(rh, rw, ("sum", "sumsq"), codec.device, pix=pix)
                px_arm = Pixels(pix, buf, stream_bytes, o_f, W, H, nf, (x, y, rw, rh), offsets)

                def arm_k():
                    pairs(buf, 0, stream_bytes, o_f, W, H, nf, offsets, x, y, rw, rh, out=out, results=r_f)

                def arm_b():
                    proj(buf, 0, stream_bytes, o_f, W, H, nf, x, y, rw, rh, out=pr, results=r_f)

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
                assert torch.equal(out.out, px_arm.acc), "the timed planes differ from the ones through pixels"
                p = plan_fn(W, H, nf, x, y, rw, rh, pairs=mask, n_cu=cus)
                decoded = p["pieces_x"] * p["piece_tiles"] if p["pieces_x"] > 1 else p["tiles_x"]
                emit(dict(dataset=name, W=W, H=H, frames_per_call=nf, window=[x, y, rw, rh], mask=mask, planes=p["planes"],
                          instance=p["instance"], pieces_x=p["pieces_x"], segments=p["segments"], ms_pairs=ms["k"],
                          ms_project_sum_sumsq=ms["b"], ms_pixels_route=ms["a"], pairs_over_floor=ms["k"] / ms["b"],
                          ms_per_plane_over_floor=(ms["k"] - ms["b"]) / p["planes"],
                          pixels_route_over_pairs=ms["a"] / ms["k"], ms_pairs_minmax=ms["k_minmax"],
                          ms_pixels_route_minmax=ms["a_minmax"], chunk_frames=px_arm.chunk,
                          peak_bytes_pixels_route=peak_a, out_bytes=int(out.out.numel()) * 8,
                          halo_tiles_share=decoded / p["tiles_x"] - 1.0,
                          rows_below_share=p["rows_below"] / (8.0 * p["tiles_y"]),
                          ms_index=t["decode_index"][0] / a.steps, ms_kernels=t["decode"][0] / a.steps,
                          equal_to_pixels_route=True))
                del out, pr, px_arm
        del buf, offs, res
    codec.close()


if __name__ == "__main__":
    main()
