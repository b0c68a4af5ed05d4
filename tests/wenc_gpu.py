"""The GPU cases of the window encoder, written once for both pixel sizes (test infrastructure, not a test module):
tests/test_gpu_wenc.py runs them with bits = 8, tests/test_gpu_wenc16.py with bits = 16.  Expected bytes come from
tests/wenc_ref.py (the oracle's frames of the windows); shapes are the smallest that reach each way to go wrong.
"""
import os

import numpy as np

import crafted_images as ci
import wenc_ref as wr


def experiment_codec(dv, flags):
    """A context created under $DBDE_HIP_EXPERIMENT = flags (bit 0: tickets, bit 10: three workgroups)."""
    if flags:
        os.environ["DBDE_HIP_EXPERIMENT"] = str(flags)
    try:
        return dv.Codec(0)
    finally:
        os.environ.pop("DBDE_HIP_EXPERIMENT", None)


def noise(rng, n, H, W, bits, kind="mixed"):
    """Images with a different depth per 8 x 8 tile (mixed) or full-range noise."""
    top = 1 << bits
    if kind == "full":
        return rng.integers(0, top, (n, H, W)).astype(ci.dtype_of(bits))
    h, w = (H + 7) // 8, (W + 7) // 8
    d = np.repeat(np.repeat(rng.integers(0, bits + 1, (n, h, w)), 8, 1), 8, 2)[:, :H, :W]
    base = np.repeat(np.repeat(rng.integers(0, top, (n, h, w)), 8, 1), 8, 2)[:, :H, :W]
    img = np.minimum(base, top - (1 << d)) + (rng.integers(0, top, (n, H, W)) & ((1 << d) - 1))
    return img.astype(ci.dtype_of(bits))


def source(rng, W, H, n, bits, pitch=0, frame_stride=0, base=0, exact_window=None):
    """A source of full-range noise everywhere (pitch padding and lead included): every byte outside a window differs
    from what the window's padding rule would put there."""
    px = bits // 8
    p, s = wr.compact(W, H, bits, pitch, frame_stride)
    size = base + wr.min_image_bytes(W, H, n, bits, pitch, frame_stride) + wr.GUARD
    if exact_window is not None:
        x, y, rw, rh = exact_window
        size = base + (n - 1) * s + (y + rh - 1) * p + (x + rw) * px
    buf = rng.integers(0, 256, size).astype(np.uint8)
    return wr.Source(buf, base, W, H, n, bits, pitch, frame_stride,
                     image_bytes=None if exact_window is None else size - base)


def margins(codec, pack, bits):
    """Source 40 x 29 at pitch 43 pixels, base offset one pixel, window at (5, 3), 3 frames: every right and bottom margin
    1..8 (rw 17..24, rh 9..16), the narrow windows rw 1..16 at rh = 9, both layouts, d_out at offsets 0..7."""
    px = bits // 8
    rng = np.random.default_rng(40 + bits)
    src = source(rng, 40, 29, 3, bits, pitch=43 * px, base=px)
    sizes = [(rw, rh) for rw in range(17, 25) for rh in range(9, 17)] + [(rw, 9) for rw in range(1, 17)]
    for k, (rw, rh) in enumerate(sizes):
        frames, _, _ = wr.encode_window(pack, src.host, src.base, 40, 29, src.pitch, 0, 3, 5, 3, rw, rh, bits, first_index=9)
        for slot in (0, wr.max_frame_bytes(rw, rh, bits) + 3):
            for mis in range(8):
                r = wr.run(codec, src, 5, 3, rw, rh, first_index=9, slot_stride=slot, out_misalign=mis)
                offs = [f * slot for f in range(3)] if slot else np.cumsum([0] + [len(f) for f in frames[:-1]]).tolist()
                wr.check(r, frames, offs, [len(f) for f in frames], rw, rh, bits, what=f"{rw}x{rh} slot {slot} out+{mis}")


def alignment(codec, pack, bits):
    """Window 64 x 16 in a 100 x 20 source, x0 = 0..15 at pitches of 100, 101, 112, 113 bytes (DBDE16: pixels at the even
    ones, doubled): every alignment of a row's 16-byte fetches."""
    px = bits // 8
    rng = np.random.default_rng(100 + bits)
    pitches = (100, 101, 112, 113) if bits == 8 else (200, 202, 224, 226)
    for pitch in pitches:
        src = source(rng, 100, 20, 2, bits, pitch=pitch, base=0)
        for x0 in range(16):
            wr.run_and_check(codec, pack, src, x0, 2, 64, 16, what=f"pitch {pitch} x0 {x0}")


FAMILIES = [("padding_trap", ci.padding_trap), ("lone_high", ci.lone_extreme(True)), ("lone_low", ci.lone_extreme(False)),
            ("range_ladder", ci.range_ladder), ("depth_runs", ci.depth_runs(64, "runs")), ("bit_patterns", ci.bit_patterns())]


def surroundings(codec, pack, bits, rw, rh):
    """The crafted families as windows inside a larger source whose other bytes are all 0 in one run and all ones in the
    other: each tile's depth and minimum are the family's own, both runs give identical bytes, and the frames are the
    oracle's.  A row below rh or a column beyond rw that entered a tile would change a minimum (0) or a depth (top)."""
    W, H, x, y, n = rw + 29, rh + 13, 11, 5, 3
    px = bits // 8
    for name, fam in FAMILIES:
        made = [fam(rw, rh, f, bits) for f in range(n)]
        runs = []
        for fill in (0, ci.top_of(bits)):
            buf = wr.embed([m[0] for m in made], W, H, x, y, bits, pitch=(W + 3) * px, base=px, fill=fill)
            src = wr.Source(buf, px, W, H, n, bits, pitch=(W + 3) * px)
            r, frames = wr.run_and_check(codec, pack, src, x, y, rw, rh, what=f"{name} fill {fill}", first_index=5)
            for f in range(n):
                depth, mins, _, _ = ci.frame_arrays(wr.frame_of(r, f), rw, rh, bits)
                assert np.array_equal(depth, made[f][1]), (name, fill, f, "depth")
                assert np.array_equal(mins, made[f][2]), (name, fill, f, "minimum")
            runs.append(r.canvas)
        assert np.array_equal(runs[0], runs[1]), (name, "the output depends on bytes outside the window")


def buffer_edges(codec, pack, bits):
    """Windows at (0, 0) and at (W-rw, H-rh) of a source sized exactly: image_bytes is the least the call accepts, so it
    ends with the last pixel of the last frame's window at (W-rw, H-rh) (compact pitch, and pitch = W + 5 pixels); the
    base lies one pixel into its allocation.  The last rows' fetches would pass the end of the extent."""
    px = bits // 8
    rng = np.random.default_rng(7 + bits)
    W, H, n = 61, 23, 3
    for pitch in (0, (W + 5) * px):
        src = source(rng, W, H, n, bits, pitch=pitch, base=px, exact_window=(0, 0, W, H))
        assert src.image_bytes == wr.min_image_bytes(W, H, n, bits, pitch) == len(src.host) - px
        for rw, rh in ((61, 23), (37, 13), (9, 5), (16, 8), (33, 23)):
            for x, y in ((0, 0), (W - rw, H - rh)):
                wr.run_and_check(codec, pack, src, x, y, rw, rh, what=f"pitch {pitch} {rw}x{rh} at {x},{y}")


def origins(codec, pack, bits):
    """7 frames with per-frame origins, among them (-5, -5), (W, H) and a diagonal walk: the model's clamped origins."""
    px = bits // 8
    rng = np.random.default_rng(3 + bits)
    W, H, rw, rh = 90, 50, 33, 31
    org = [(-5, -5), (W, H), (0, 0), (7, 3), (14, 6), (21, 9), (W - rw, H - rh)]
    src = source(rng, W, H, 7, bits, pitch=(W + 1) * px, base=px)
    for slot in (0, wr.max_frame_bytes(rw, rh, bits) + 8):
        wr.run_and_check(codec, pack, src, 0, 0, rw, rh, what=f"origins slot {slot}", origins=org, slot_stride=slot)


def record_levels(codec, pack, dv, bits, batch):
    """More chunks per frame than one group of records (1456 x 1448 in 1500 x 1460, 3 frames) or more frames than one
    group (130 frames of 20 x 12), concatenated, taken from the plan's constants.  -> the Source and the expected frames,
    for the runs under the experiment flags."""
    px = bits // 8
    rng = np.random.default_rng(11 + bits + len(batch))
    plan = dv.window_encode_plan if bits == 8 else dv.window_encode16_plan
    if batch == "chunks":
        W, H, n, x, y, rw, rh = 1500, 1460, 3, 31, 7, 1456, 1448
        pl = plan(W, H, n, x, y, rw, rh)
        assert pl["chunks_per_frame"] > pl["record_group"]
        imgs = noise(rng, n, rh, rw, bits)
        buf = wr.embed(list(imgs), W, H, x, y, bits, fill=ci.top_of(bits) // 3)
    else:
        W, H, n, x, y, rw, rh = 47, 19, 130, 13, 5, 20, 12
        pl = plan(W, H, n, x, y, rw, rh)
        assert n > 2 * pl["record_group"]
        buf = rng.integers(0, 256, wr.min_image_bytes(W, H, n, bits) + wr.GUARD).astype(np.uint8)
    src = wr.Source(buf, 0, W, H, n, bits)
    frames, offs, sizes = wr.encode_window(pack, src.host, 0, W, H, 0, 0, n, x, y, rw, rh, bits, first_index=3)
    return src, (x, y, rw, rh), (frames, offs, sizes)


def check_record_levels(codec, case, bits):
    src, (x, y, rw, rh), (frames, offs, sizes) = case
    for rep in range(2):   # the second call finds the workspace as the first left it
        r = wr.run(codec, src, x, y, rw, rh, first_index=3)
        wr.check(r, frames, offs, sizes, rw, rh, bits, what=f"rep {rep}")


ERROR_CASES = ["pitch_below_row", "odd_pitch", "stride_small", "image_bytes_short", "origin_outside", "rw_above_W",
               "rh_below_1", "capacity_short", "slot_stride_small"]


def broken_call(case, bits):
    """(source kwargs, call kwargs, expected code) of one broken rule on a 40 x 29 source, window 17 x 9 at (5, 3), 3 frames."""
    px = bits // 8
    W, H, n, rw, rh = 40, 29, 3, 17, 9
    maxf = wr.max_frame_bytes(rw, rh, bits)
    s = dict(pitch=43 * px, frame_stride=0, image_bytes=None)
    c = dict(x=5, y=3, rw=rw, rh=rh, slot_stride=0, cap=None)
    code = -1
    if case == "pitch_below_row":
        s["pitch"] = W * px - 1 if bits == 8 else W * px - 2
    elif case == "odd_pitch":
        s["pitch"] = 43 * px + 1            # an odd pitch is DBDE16's error only
        code = -1 if bits == 16 else 0
    elif case == "stride_small":
        s["frame_stride"] = (H - 1) * 43 * px + W * px - px
    elif case == "image_bytes_short":
        s["image_bytes"] = wr.min_image_bytes(W, H, n, bits, 43 * px) - 1
    elif case == "origin_outside":
        c["x"] = W - rw + 1
    elif case == "rw_above_W":
        c["x"], c["rw"] = 0, W + 1
    elif case == "rh_below_1":
        c["rh"] = 0
    elif case == "capacity_short":
        c["cap"], code = n * maxf - 1, -3
    elif case == "slot_stride_small":
        c["slot_stride"], code = maxf - 1, (-1 if bits == 8 else -3)
    return s, c, code


def errors(codec, pack, bits, case):
    px = bits // 8
    rng = np.random.default_rng(5)
    s, c, code = broken_call(case, bits)
    buf = rng.integers(0, 256, px + 3 * 29 * 44 * px + 256).astype(np.uint8)
    src = wr.Source(buf, px, 40, 29, 3, bits, pitch=s["pitch"], frame_stride=s["frame_stride"], image_bytes=s["image_bytes"])
    r = wr.run(codec, src, c["x"], c["y"], c["rw"], c["rh"], slot_stride=c["slot_stride"], cap=c["cap"])
    if code == 0:
        frames, offs, sizes = wr.encode_window(pack, buf, px, 40, 29, s["pitch"], 0, 3, 5, 3, 17, 9, bits)
        wr.check(r, frames, offs, sizes, 17, 9, bits, what=case)
        return
    assert r.rc == code, (case, r.rc, r.error)
    assert r.error, "dbde_hip_last_error is empty"
    wr.untouched(r, spans=[])
    assert (r.offsets == -1).all() and (r.sizes == -1).all()
