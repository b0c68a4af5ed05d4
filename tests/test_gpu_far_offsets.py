"""GPU: every kernel at stream, image and output offsets past 2^31 and 2^32 bytes.

The rest of the suite keeps the high half of every offset at zero, and bit 31 too in all but two tests, so a kernel
that narrowed an offset to 32 bits would pass it.  Here every buffer a kernel is given sits in one allocation laid
out by tests/far.py: a sentinel lead of 2^31 + 2^26 bytes (2^33 for U16 image batches) in front, a tail of 2^26 bytes
behind, offsets below 2^33.  A truncated or sign-extended offset then lands inside the test's own allocation, on a
decoy frame or on sentinel bytes, and the test fails with wrong values rather than a fault.

Stream readers (decode_frames in every form test_gpu_crafted_decode.CASES pins, decode_frames16, the window decoders,
projections, traces and histograms) read the six far placements of far.SLOTS, repeated to the batch size their form
needs, once for each field that crosses 2^32 (depth array, minima array, payload).  Each case is compared with the
oracle's decode of every distinct frame (exact int64 NumPy reductions for the statistics), element for element with
the same call on a near copy of the stream, and the sentinel lead and tail of every buffer a kernel wrote.
Encoders write slots past 2^31 and 2^32 and concatenated streams that cross 2^32 (8-bit and DBDE16), compared byte
for byte with the oracle; the scanners walk the 8-bit one; image batches past 2^32 are decoded back and compared on
the device.

Out of scope: a launch-wide payload word count past 2^32 words (32 GiB of payload); histogram rows and trace outputs
past 2^31 elements (8.6 GB and more of outputs); file I/O past 4 GiB; multi-rank transfers.
"""
import time

import numpy as np
import pytest

import far
from test_gpu_crafted_decode import CASES as DECODE_CASES
from test_gpu_traces import map_discs, reduce_labels
from test_oracle_u16 import o16, pack16, unpack16   # noqa: F401  (fixture + helpers)

pytestmark = pytest.mark.gpu

G31, G32 = far.G31, far.G32
S8 = far.SENTINEL
S16 = (S8 << 8) | S8
PERSISTENT, SMALL, TINY, MID, FRAMES, GROUP = 0, 1, 2, 3, 4, 5
SEED = 0xFA2_0FF5


@pytest.fixture(scope="module")
def dv():
    import dbde_video_cpp_amd as m
    return m


@pytest.fixture(scope="module")
def codec(dv):
    c = dv.Codec(0)
    assert c.arch.startswith("gfx950")
    yield c
    c.close()


@pytest.fixture(autouse=True)
def device_memory(record_property):
    """Frees what the last test left, and records this test's peak device memory and wall time."""
    import torch
    far.free()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    yield
    torch.cuda.synchronize()
    record_property("peak_device_bytes", int(torch.cuda.max_memory_allocated()))
    record_property("wall_seconds", round(time.perf_counter() - t0, 2))
    far.free()


# ---- the frame sets and their reference decode ------------------------------------------------------------------

class Frames:
    """far.frame_set of one geometry, its three layouts (one per straddle kind) and the reference row and image of
    every distinct frame (the oracle; the DBDE16 oracle for bits 16)."""

    def __init__(self, oracle, o16, W, H, bits):   # noqa: F811
        self.W, self.H, self.bits = W, H, bits
        good, bad, decoys = far.frame_set(W, H, bits, oracle, lambda img, i: pack16(o16, img, i))
        self.layouts = {s: far.far_layout(good, bad, decoys, s) for s in far.STRADDLES}
        self._ref = {}
        for fr in good + bad:
            _, fh = oracle.unpack_frame_header(fr)
            if bits == 8:
                adv, _, img = oracle.unpack_frame(fr, W, H)
                used = adv - 20
            else:
                used, img = unpack16(o16, fr, W, H)
            self._ref[id(fr)] = ((fh[0] if used else 0xFFFFFFFF, fh[1], fh[2], 20 + used), img if used else None)

    def refs(self, lay, slots):
        """[(row, image or None)] of the frames the entries `slots` read."""
        return [self._ref[id(lay.frames[k])] for k in slots]


_frames = {}


def frames_of(oracle, o16, W, H, bits=8):   # noqa: F811
    key = (W, H, bits)
    if key not in _frames:
        if len(_frames) > 3:
            _frames.clear()
        _frames[key] = Frames(oracle, o16, W, H, bits)
    return _frames[key]


def far_and_near(lay, ents, call):
    """call(stream) on the far stream, then on its near copy; -> (far outputs, near outputs).  call returns a tuple
    of device tensors (results rows included)."""
    import torch
    fs = far.far_stream(lay, ents)
    got = call(fs)
    torch.cuda.synchronize()
    del fs
    ns = far.NearStream(lay, ents)
    near = call(ns)
    torch.cuda.synchronize()
    return got, near


def assert_same(got, near, what):
    import torch
    for k, (a, b) in enumerate(zip(got, near)):
        if a is None:
            assert b is None
            continue
        if not torch.equal(a, b):
            bad = (a != b).nonzero()[0].tolist()
            raise AssertionError(f"{what}: output {k} differs from the near copy at {bad}: {a[tuple(bad)]} != "
                                 f"{b[tuple(bad)]} (an addressing bug)")


def assert_rows(codec, res, refs, what):
    rows = codec.parse_results(res)
    for f, (r, (want, _)) in enumerate(zip(rows, refs)):
        assert r == want, f"{what}: entry {f} result {r} != {want}"


def chunks(n):
    """The entry lists of the calls that cover all six slots with batches of n (n < 6: several calls)."""
    ents = far.entries(max(n, len(far.SLOTS)))
    return [ents[i:i + n] for i in range(0, len(ents), n) if len(ents[i:i + n]) == n]


# ---- a. stream readers at far offsets ---------------------------------------------------------------------------

def expected_images(refs, H, W, dtype, fill):
    return np.stack([img.astype(dtype) if img is not None else np.full((H, W), fill, dtype) for _, img in refs])


@pytest.mark.parametrize("W,H,n,form", [c[:4] for c in DECODE_CASES], ids=[f"{c[0]}x{c[1]}x{c[2]}" for c in DECODE_CASES])
def test_decode_frames_far(dv, codec, oracle, o16, W, H, n, form):   # noqa: F811
    import torch
    fr = frames_of(oracle, o16, W, H)
    for straddle, lay in fr.layouts.items():
        for ents in chunks(n):
            outs = []

            def call(s):
                g = far.guarded((n, H, W), torch.uint8)
                _, res = codec.decode_frames(s.buf, s.lead, s.stream_bytes, s.offs, W, H, n, images=g.t)
                codec.sync()
                g.check(f"{W}x{H} x{n} {straddle}")
                plan = dv.decode_plan(W, H, n, g.t.data_ptr())
                assert {k: plan[k] for k in form} == form, f"{W}x{H} x{n}: decode_plan {plan} is not {form}"
                outs.append(g)
                return g.t, res

            got, near = far_and_near(lay, ents, call)
            what = f"{W}x{H} x{n} {straddle}"
            assert_same(got, near, what)
            refs = fr.refs(lay, ents)
            assert_rows(codec, got[1], refs, what)
            want = expected_images(refs, H, W, np.uint8, S8)
            img = got[0].cpu().numpy()
            if not np.array_equal(img, want):
                f = int(np.argwhere((img != want).reshape(n, -1).any(1))[0][0])
                raise AssertionError(f"{what}: entry {f} (slot {far.SLOTS[ents[f]]}) differs from the oracle")
            del outs, got, near


@pytest.mark.parametrize("W,H,n", [(200, 123, 13), (1024, 768, 16), (4096, 3072, 6)])
def test_decode_frames16_far(codec, oracle, o16, W, H, n):   # noqa: F811
    import torch
    fr = frames_of(oracle, o16, W, H, 16)
    for straddle, lay in fr.layouts.items():
        ents = far.entries(n)

        def call(s):
            g = far.guarded((n, H, W), torch.int16)
            _, res = codec.decode_frames16(s.buf, s.lead, s.stream_bytes, s.offs, W, H, n, images=g.t)
            codec.sync()
            g.check(f"16-bit {W}x{H} {straddle}")
            return g.t, res

        got, near = far_and_near(lay, ents, call)
        what = f"16-bit {W}x{H} x{n} {straddle}"
        assert_same(got, near, what)
        refs = fr.refs(lay, ents)
        assert_rows(codec, got[1], refs, what)
        assert np.array_equal(got[0].cpu().numpy().view(np.uint16), expected_images(refs, H, W, np.uint16, S16)), what
        del got, near


@pytest.mark.parametrize("bits,W,H,n", [(8, 200, 123, 13), (8, 1024, 768, 6), (16, 200, 123, 13),
                                        (16, 1024, 768, 6)])
def test_windows_far(dv, codec, oracle, o16, bits, W, H, n):   # noqa: F811
    import torch
    fr = frames_of(oracle, o16, W, H, bits)
    rng = np.random.default_rng(W + n + bits)
    dtype, npd, fill = (torch.uint8, np.uint8, S8) if bits == 8 else (torch.int16, np.uint16, S16)
    plan_fn = dv.roi_plan if bits == 8 else dv.roi16_plan
    for (x, y, rw, rh) in [(W // 3, H // 5, W // 2, H // 3), (0, 0, W, H), (W - 9, 1, 9, H - 2)]:
        plan = plan_fn(W, H, n, x, y, rw, rh)
        assert (plan["tile_x"], plan["tile_y"]) == (x // 8, y // 8), plan
        assert (plan["tiles_x"], plan["tiles_y"]) == ((x + rw + 7) // 8 - x // 8, (y + rh + 7) // 8 - y // 8), plan
        for per_frame in (False, True):
            org = None
            if per_frame:
                org = np.stack([rng.integers(-3, W + 3, n), rng.integers(-3, H + 3, n)], 1).astype(np.int32)
            for straddle, lay in fr.layouts.items():
                ents = far.entries(n)

                def call(s):
                    g = far.guarded((n, rh, rw), dtype)
                    fn = codec.decode_roi if bits == 8 else codec.decode_roi16
                    _, res = fn(s.buf, s.lead, s.stream_bytes, s.offs, W, H, n, x, y, rw, rh,
                                origins=None if org is None else torch.from_numpy(org).cuda(), out=g.t)
                    codec.sync()
                    g.check(f"window {bits}-bit {straddle}")
                    return g.t, res

                got, near = far_and_near(lay, ents, call)
                what = f"{bits}-bit {W}x{H} window {(x, y, rw, rh)} per-frame {per_frame} {straddle}"
                assert_same(got, near, what)
                refs = fr.refs(lay, ents)
                assert_rows(codec, got[1], refs, what)
                win = got[0].cpu().numpy().view(npd)
                for f, (_, img) in enumerate(refs):
                    ox, oy = (x, y) if org is None else (min(max(int(org[f, 0]), 0), W - rw),
                                                         min(max(int(org[f, 1]), 0), H - rh))
                    want = np.full((rh, rw), fill, npd) if img is None else img[oy:oy + rh, ox:ox + rw]
                    assert np.array_equal(win[f], want), f"{what}: entry {f}"
                del got, near


def reduce_refs(refs, x, y, rw, rh, top):
    """Exact int64 max / min / sum / sumsq of the window over the accepted frames: each distinct frame reduced once."""
    per = {}
    mult = {}
    for _, img in refs:
        if img is None:
            continue
        k = id(img)
        mult[k] = mult.get(k, 0) + 1
        if k not in per:
            w = img[y:y + rh, x:x + rw].astype(np.int64)
            per[k] = (w, w * w)
    z = np.zeros((rh, rw), np.int64)
    if not per:
        return dict(max=z, min=z + top, sum=z, sumsq=z, count=0)
    return dict(max=np.max([w for w, _ in per.values()], 0), min=np.min([w for w, _ in per.values()], 0),
                sum=sum(mult[k] * w for k, (w, _) in per.items()), sumsq=sum(mult[k] * q for k, (_, q) in per.items()),
                count=sum(mult.values()))


def projection_tensors(pr):
    import torch
    v = lambda t: t.to(torch.int32) & 0xFFFF if t.dtype == torch.int16 else t.to(torch.int64)   # noqa: E731
    return v(pr.max), v(pr.min), pr.sum, pr.sumsq, pr.count


def assert_projection(pr, want, what):
    for name, t in zip(("max", "min", "sum", "sumsq"), projection_tensors(pr)[:4]):
        got = t.cpu().numpy().astype(np.int64)
        if not np.array_equal(got, want[name]):
            bad = tuple(np.argwhere(got != want[name])[0])
            raise AssertionError(f"{what}: {name} differs at {bad}: {got[bad]} != {want[name][bad]}")
    assert int(pr.count.item()) == want["count"], what


@pytest.mark.parametrize("bits", [8, 16])
def test_projections_far(dv, codec, oracle, o16, bits):   # noqa: F811
    """600 entries of 200 x 123: several segments and the combine kernel; and one call that continues a projection
    of a near batch."""
    W, H, n = 200, 123, 600
    fr = frames_of(oracle, o16, W, H, bits)
    top = 255 if bits == 8 else 65535
    proj = codec.project if bits == 8 else codec.project16
    plan = (dv.project_plan if bits == 8 else dv.project16_plan)(W, H, n)
    assert plan["segments"] > 1 and plan["combine_grid"] > 0, plan
    for (x, y, rw, rh) in [(0, 0, W, H), (13, 7, 101, 60)]:
        for straddle, lay in fr.layouts.items():
            ents = far.entries(n)

            def call(s):
                pr, res = proj(s.buf, s.lead, s.stream_bytes, s.offs, W, H, n, x, y, rw, rh)
                codec.sync()
                return projection_tensors(pr) + (res,)

            got, near = far_and_near(lay, ents, call)
            what = f"{bits}-bit projection {(x, y, rw, rh)} {straddle}"
            assert_same(got, near, what)
            refs = fr.refs(lay, ents)
            assert_rows(codec, got[5], refs, what)
            want = reduce_refs(refs, x, y, rw, rh, top)
            for name, t in zip(("max", "min", "sum", "sumsq"), got[:4]):
                assert np.array_equal(t.cpu().numpy().astype(np.int64), want[name]), f"{what}: {name}"
            assert int(got[4].item()) == want["count"], what
    # a projection of a near batch, continued by a far call
    lay = fr.layouts["payload"]
    near_ents, far_ents = far.entries(40)[::-1].copy(), far.entries(n)
    ns = far.NearStream(lay, near_ents)
    base, _ = proj(ns.buf, ns.lead, ns.stream_bytes, ns.offs, W, H, len(near_ents), 5, 3, 150, 100)
    fs = far.far_stream(lay, far_ents)
    acc, _ = proj(fs.buf, fs.lead, fs.stream_bytes, fs.offs, W, H, n, 5, 3, 150, 100, out=base, accumulate=True)
    codec.sync()
    assert_projection(acc, reduce_refs(fr.refs(lay, near_ents) + fr.refs(lay, far_ents), 5, 3, 150, 100, top),
                      f"{bits}-bit accumulated")


def trace_labels(W, H):
    """Discs (whole and boundary tiles) with the left third of the frame unlabelled (untouched tiles)."""
    lab, L = map_discs(W, H, seed=5)
    lab[:, : W // 3] = 0
    return lab, L


@pytest.mark.parametrize("bits,W,H,n", [(8, 200, 123, 13), (8, 4096, 3072, 6), (16, 200, 123, 13),
                                        (16, 1024, 768, 6)])
def test_traces_far(dv, codec, oracle, o16, bits, W, H, n):   # noqa: F811
    import torch
    fr = frames_of(oracle, o16, W, H, bits)
    lab, L = trace_labels(W, H)
    tmap = codec.trace_map(lab, L)
    info = tmap.info
    assert info["tiles_whole"] > 0 and info["tiles_mixed"] > 0 and info["tiles_active"] < info["tiles"], info
    plan = (dv.trace_plan if bits == 8 else dv.trace16_plan)(W, H, n, info)
    assert plan["chunks_per_frame"] >= 1, plan
    fn = codec.traces if bits == 8 else codec.traces16
    pix = 1 if bits == 8 else 2
    for straddle, lay in fr.layouts.items():
        ents = far.entries(n)

        def call(s):
            out = dv.Traces.empty(n, L, ("max", "min", "sum", "sumsq"), "cuda", pix=pix, pixels=tmap.pixels)
            for t in (out.max, out.min, out.sum, out.sumsq):
                t.fill_(0x5A)
            tr, res = fn(s.buf, s.lead, s.stream_bytes, s.offs, W, H, n, tmap, out=out)
            codec.sync()
            return tr.max, tr.min, tr.sum, tr.sumsq, res

        got, near = far_and_near(lay, ents, call)
        what = f"{bits}-bit traces {W}x{H} {straddle}"
        assert_same(got, near, what)
        refs = fr.refs(lay, ents)
        assert_rows(codec, got[4], refs, what)
        ok = [img is not None for _, img in refs]
        imgs = torch.from_numpy(np.stack([img.astype(np.int32) if img is not None else np.zeros((H, W), np.int32)
                                          for _, img in refs])).cuda()
        want = reduce_labels(imgs, lab, L, pix_max=255 if bits == 8 else 65535)
        for name, t in zip(("max", "min", "sum", "sumsq"), got[:4]):
            g = (t.to(torch.int32) & 0xFFFF if t.dtype == torch.int16 else t.to(torch.int64)).to(torch.int64)
            for f in range(n):
                if ok[f]:
                    assert torch.equal(g[f], want[name][f]), f"{what}: {name} of entry {f}"
                else:
                    assert (t[f] == 0x5A).all(), f"{what}: rejected entry {f}'s {name} row was written"
    tmap.close()


@pytest.mark.parametrize("bits,W,H,n,shift,bins", [
    (8, 4096, 3072, 6, 0, 256), (8, 200, 123, 13, 4, 9),           # LDS bins; whole tiles as one add (shift 4)
    (16, 1024, 768, 6, 0, 4096), (16, 200, 123, 13, 4, 4096),      # 4,096 LDS bins
    (16, 200, 123, 13, 8, 256), (16, 4096, 3072, 6, 12, 16)])      # 256 LDS bins; one add per whole tile
def test_histograms_far(dv, codec, oracle, o16, bits, W, H, n, shift, bins):   # noqa: F811
    import torch
    fr = frames_of(oracle, o16, W, H, bits)
    x, y, rw, rh = 3, 5, W - 11, H - 6
    plan = (dv.histogram_plan if bits == 8 else dv.histogram16_plan)(W, H, n, x, y, rw, rh, shift=shift, bins=bins,
                                                                      total=True)
    assert plan["lds_bins"] == (4096 if bins > 256 else 256), plan
    fn = codec.histogram if bits == 8 else codec.histogram16
    for straddle, lay in fr.layouts.items():
        ents = far.entries(n)

        def call(s):
            out = dv.Histograms(torch.full((n, bins), -7, dtype=torch.int32, device="cuda"),
                                torch.full((bins,), 99, dtype=torch.int64, device="cuda"),
                                torch.full((1,), 99, dtype=torch.int64, device="cuda"))
            h, res = fn(s.buf, s.lead, s.stream_bytes, s.offs, W, H, n, x, y, rw, rh, shift=shift, bins=bins,
                        total=True, out=out)
            codec.sync()
            return h.counts, h.total, h.count, res

        got, near = far_and_near(lay, ents, call)
        what = f"{bits}-bit histogram {W}x{H} shift {shift} bins {bins} {straddle}"
        assert_same(got, near, what)
        refs = fr.refs(lay, ents)
        assert_rows(codec, got[3], refs, what)
        counts = got[0].cpu().numpy().astype(np.int64)
        per = {}
        total = np.zeros(bins, np.int64)
        for f, (_, img) in enumerate(refs):
            if img is None:
                assert (counts[f] == -7).all(), f"{what}: rejected entry {f}'s row was written"
                continue
            if id(img) not in per:
                b = np.minimum(img[y:y + rh, x:x + rw].astype(np.int64) >> shift, bins - 1)
                per[id(img)] = np.bincount(b.reshape(-1), minlength=bins)
            assert np.array_equal(counts[f], per[id(img)]), f"{what}: entry {f}"
            total += per[id(img)]
        assert np.array_equal(got[1].cpu().numpy(), total), what
        assert int(got[2].item()) == sum(img is not None for _, img in refs), what


# ---- b. encoder outputs in slots past 2^31 and 2^32 ---------------------------------------------------------------

def check_untouched(buf, lead, spans, what):
    """Every byte of the allocation outside the spans [(start, end)] (relative to lead) is still the sentinel."""
    at = 0
    for s0, s1 in sorted(spans) + [(buf.numel() - lead, buf.numel() - lead)]:
        assert far.all_equal(buf[lead + at: lead + s0], S8), f"{what}: bytes in [{at}, {s0}) were written"
        at = s1
    assert far.all_equal(buf[:lead], S8), f"{what}: wrote into the lead"


ENCODERS = [  # (W, H, n, mode, encode_plan form); n = 3: slots at 0, 2^31 + 2^20, 2^32 + 2^21
    (4096, 3072, 3, "noise8", dict(kernel=PERSISTENT, input_mode=0)),
    (4096, 3072, 2, "mixed", dict(kernel=SMALL, input_mode=0)),
    (1921, 1081, 3, "mixed", dict(kernel=SMALL, input_mode=4)),
    (8, 8, 3, "noise8", dict(kernel=TINY)),
    (75, 70, 3, "mixed", dict(kernel=MID, input_mode=3)),
    (96, 96, 3, "mixed", dict(kernel=FRAMES)),
    (64, 64, 3, "noise8", dict(kernel=GROUP)),
    (100, 100, 3, "mixed", dict(kernel=GROUP, input_mode=1)),
]


def slot_stride(n):
    return (G31 + (1 << 20)) if n >= 3 else (G32 + (1 << 20))


@pytest.mark.parametrize("W,H,n,mode,form", ENCODERS, ids=[f"{e[0]}x{e[1]}x{e[2]}" for e in ENCODERS])
def test_encoders_write_far_slots(dv, codec, oracle, W, H, n, mode, form):
    import torch
    stride = slot_stride(n)
    cap = (n - 1) * stride + dv.max_frame_bytes(W, H)
    imgs = far.guarded((n, H, W), torch.uint8)
    first = G32 - 1                        # indices cross 2^32
    codec.synth_frames(mode, SEED, 0, n, W, H, out=imgs.t)
    out = far.guarded((cap,), torch.uint8)
    plan = dv.encode_plan(W, H, n, imgs.t.data_ptr(), out.t.data_ptr(), stride)
    assert {k: plan[k] for k in form} == form, f"{W}x{H} x{n}: encode_plan {plan} is not {form}"
    offs, sizes = codec.encode_frames(imgs.t, W, H, n, out.buf, out.lead, cap, first_index=first, slot_stride=stride)
    codec.sync()
    imgs.check("images")
    o, s = offs.cpu().numpy(), sizes.cpu().numpy()
    assert [int(v) for v in o] == [f * stride for f in range(n)], o
    assert int(o[-1]) > G32
    if n >= 3:
        assert G31 < int(o[1]) < G32
    host_imgs = imgs.t.cpu().numpy()
    for f in range(n):
        assert np.array_equal(host_imgs[f], oracle.synth_frame(dv.MODES[mode], SEED, f, W, H)), f
        want = oracle.pack_frame(first + f, host_imgs[f], W, H)
        assert int(s[f]) == len(want), (f, int(s[f]), len(want))
        got = out.t[int(o[f]): int(o[f]) + len(want)].cpu().numpy()
        assert got.tobytes() == want.tobytes(), f"{W}x{H} frame {f} at {int(o[f])}: bytes differ from the oracle"
    check_untouched(out.buf, out.lead, [(int(a), int(a) + int(b)) for a, b in zip(o, s)], f"{W}x{H} x{n}")


@pytest.mark.parametrize("W,H", [(1024, 768), (33, 31)])
def test_encoder16_writes_far_slots(codec, o16, W, H):   # noqa: F811
    import torch
    n, stride = 3, slot_stride(3)
    maxf = int(codec.L.dbde16_hip_max_frame_bytes(W, H))
    cap = (n - 1) * stride + maxf
    rng = np.random.default_rng(W)
    host = rng.integers(0, 65536, (n, H, W)).astype(np.uint16)
    host[1] >>= 7
    imgs = far.guarded((n, H, W), torch.int16)
    imgs.t.copy_(torch.from_numpy(host.view(np.int16)))
    out = far.guarded((cap,), torch.uint8)
    first = G32 + 5
    offs, sizes = codec.encode_frames16(imgs.t, W, H, n, out.buf, out.lead, cap, first_index=first, slot_stride=stride)
    codec.sync()
    imgs.check("images")
    o, s = offs.cpu().numpy(), sizes.cpu().numpy()
    assert [int(v) for v in o] == [f * stride for f in range(n)], o
    for f in range(n):
        want = pack16(o16, host[f], first + f)
        assert int(s[f]) == len(want)
        assert out.t[int(o[f]): int(o[f]) + len(want)].cpu().numpy().tobytes() == want.tobytes(), f
    check_untouched(out.buf, out.lead, [(int(a), int(a) + int(b)) for a, b in zip(o, s)], f"16-bit {W}x{H}")


# ---- c. concatenated streams that cross 2^32 --------------------------------------------------------------------

def frames_around(o, s, boundary):
    """The frame that holds byte `boundary`, the two after it and the last frame."""
    f = int(np.searchsorted(o + s, boundary, side="right"))
    assert o[f] <= boundary < o[f] + s[f] and o[f] < boundary
    return sorted({f, f + 1, f + 2, len(o) - 1})


def test_concatenated_stream_past_4gib(dv, codec, oracle):
    """344 noise8 frames of 4096 x 3072 (4.33 GB of images, 4.46 GB of stream), persistent encoder, concatenated: the
    offsets, the frames around 2^32 byte for byte, the three scanners, and the decode back into a 4.33 GB batch."""
    import torch
    W, H, n = 4096, 3072, 344
    first = G32 - 200
    imgs = far.guarded((n, H, W), torch.uint8)
    codec.synth_frames("noise8", SEED, 0, n, W, H, out=imgs.t)
    cap = n * dv.max_frame_bytes(W, H)
    out = far.guarded((cap,), torch.uint8)
    plan = dv.encode_plan(W, H, n, imgs.t.data_ptr(), out.t.data_ptr(), 0)
    assert plan["kernel"] == PERSISTENT and plan["input_mode"] == 0, plan
    offs, sizes = codec.encode_frames(imgs.t, W, H, n, out.buf, out.lead, cap, first_index=first)
    codec.sync()
    imgs.check("images")
    o, s = offs.cpu().numpy(), sizes.cpu().numpy()
    assert o[0] == 0 and np.array_equal(o[1:], np.cumsum(s)[:-1]), "offsets are not the running sum of the sizes"
    total = int(o[-1] + s[-1])
    assert total > G32 + (1 << 27)
    check_untouched(out.buf, out.lead, [(0, total)], "concatenated stream")
    for f in frames_around(o, s, G32):
        img = imgs.t[f].cpu().numpy()
        assert np.array_equal(img, oracle.synth_frame(0, SEED, f, W, H)), f
        want = oracle.pack_frame(first + f, img, W, H)
        assert out.t[int(o[f]): int(o[f]) + int(s[f])].cpu().numpy().tobytes() == want.tobytes(), f
    # the scanners: sizes are only in-band
    found, count = codec.index_stream(out.buf, out.lead, total, W, H, n + 8)
    assert count == n and torch.equal(found, offs), "index_stream"
    found = torch.full((n + 8,), -3, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
    codec.index_stream_async(out.buf, out.lead, total, W, H, n + 8, found, cnt)
    codec.sync()
    assert int(cnt.item()) == n and torch.equal(found[:n], offs), "index_stream_async"
    per = 100
    nb = (n + per - 1) // per
    cursor = torch.zeros(1, dtype=torch.int64, device="cuda")
    found = torch.full((nb * per,), -3, dtype=torch.int64, device="cuda")
    counts = torch.zeros(nb, dtype=torch.int32, device="cuda")
    for b in range(nb):
        codec.scan_ahead(out.buf, out.lead, total, W, H, per, cursor, found[b * per:(b + 1) * per], counts[b:b + 1])
        codec.scan_join()
    codec.sync()
    assert int(counts.sum().item()) == n and torch.equal(found[:n], offs), "scan_ahead"
    assert int(cursor.item()) == total
    # decode back into a batch past 2^32
    back = far.guarded((n, H, W), torch.uint8)
    _, res = codec.decode_frames(out.buf, out.lead, total, offs, W, H, n, images=back.t)
    codec.sync()
    back.check("decoded images")
    assert torch.equal(back.t, imgs.t), "round trip past 2^32"
    r = res.cpu().numpy()
    assert np.array_equal(r[:, 0] & 0xFFFFFFFF, np.full(n, 2)) and np.array_equal(r[:, 1], first + np.arange(n))
    assert np.array_equal(r[:, 2], np.zeros(n)) and np.array_equal(r[:, 3], s)


def test_concatenated_stream16_past_4gib(codec, o16):   # noqa: F811
    """172 full-range U16 frames of 4096 x 3072 (4.33 GB of images, 4.43 GB of stream), concatenated: offsets, the
    frames around 2^32 byte for byte, the decode back into a 4.33 GB U16 batch."""
    import torch
    W, H, n = 4096, 3072, 172
    first = G32 - 100
    imgs = far.guarded((n, H, W), torch.int16)
    g = torch.Generator(device="cuda").manual_seed(172)
    for f0 in range(0, n, 8):
        k = min(8, n - f0)
        imgs.t[f0:f0 + k] = torch.randint(-32768, 32768, (k, H, W), dtype=torch.int16, device="cuda", generator=g)
    maxf = int(codec.L.dbde16_hip_max_frame_bytes(W, H))
    cap = n * maxf
    out = far.guarded((cap,), torch.uint8)
    offs, sizes = codec.encode_frames16(imgs.t, W, H, n, out.buf, out.lead, cap, first_index=first)
    codec.sync()
    imgs.check("images")
    o, s = offs.cpu().numpy(), sizes.cpu().numpy()
    assert o[0] == 0 and np.array_equal(o[1:], np.cumsum(s)[:-1])
    total = int(o[-1] + s[-1])
    assert total > G32 + (1 << 26)
    check_untouched(out.buf, out.lead, [(0, total)], "DBDE16 stream")
    for f in frames_around(o, s, G32):
        img = imgs.t[f].cpu().numpy().view(np.uint16)
        want = pack16(o16, img, first + f)
        assert out.t[int(o[f]): int(o[f]) + int(s[f])].cpu().numpy().tobytes() == want.tobytes(), f
    back = far.guarded((n, H, W), torch.int16)
    _, res = codec.decode_frames16(out.buf, out.lead, total, offs, W, H, n, images=back.t)
    codec.sync()
    back.check("decoded U16 images")
    assert torch.equal(back.t, imgs.t), "round trip past 2^32"
    r = res.cpu().numpy()
    assert np.array_equal(r[:, 1], first + np.arange(n)) and np.array_equal(r[:, 3], s)


# ---- d. image batches past 2^32 through the small-frame kernels ------------------------------------------------

def test_small_frames_past_4gib(dv, codec, oracle):
    """1,050,000 frames of 64 x 64 (4.30 GB of images, 4.57 GB of slots): the group encoder, spot checks around the
    2^32 boundaries of images and slots, the mid decoder back into a guarded batch."""
    import torch
    W, H, n = 64, 64, 1_050_000
    stride = (dv.max_frame_bytes(W, H) + 255) // 256 * 256
    first = 7
    imgs = far.guarded((n, H, W), torch.uint8)
    codec.synth_frames("mixed", SEED, first, n, W, H, out=imgs.t)
    cap = (n - 1) * stride + dv.max_frame_bytes(W, H)
    out = far.guarded((cap,), torch.uint8)
    plan = dv.encode_plan(W, H, n, imgs.t.data_ptr(), out.t.data_ptr(), stride)
    assert plan["kernel"] == GROUP, plan
    offs, sizes = codec.encode_frames(imgs.t, W, H, n, out.buf, out.lead, cap, first_index=first, slot_stride=stride)
    codec.sync()
    imgs.check("images")
    assert torch.equal(offs, torch.arange(n, dtype=torch.int64, device="cuda") * stride)
    s = sizes.cpu().numpy()
    img_f, slot_f = G32 // (W * H), G32 // stride
    for f in sorted({0, slot_f - 1, slot_f, slot_f + 1, img_f - 1, img_f, img_f + 1, n - 1}):
        want = oracle.pack_frame(first + f, oracle.synth_frame(1, SEED, first + f, W, H), W, H)
        assert np.array_equal(imgs.t[f].cpu().numpy(), oracle.synth_frame(1, SEED, first + f, W, H)), f
        assert int(s[f]) == len(want), f
        assert out.t[f * stride: f * stride + len(want)].cpu().numpy().tobytes() == want.tobytes(), f
    back = far.guarded((n, H, W), torch.uint8)
    dplan = dv.decode_plan(W, H, n, back.t.data_ptr())
    assert dplan["kernel"] == MID, dplan
    _, res = codec.decode_frames(out.buf, out.lead, cap, offs, W, H, n, images=back.t)
    codec.sync()
    back.check("decoded images")
    assert torch.equal(back.t, imgs.t), "round trip past 2^32"
    assert torch.equal(res[:, 1], torch.arange(first, first + n, dtype=torch.int64, device="cuda"))
    assert torch.equal(res[:, 3], sizes) and bool((res[:, 2] == 0).all()) and bool(((res[:, 0] & 0xFFFFFFFF) == 2).all())


def test_windows_past_4gib(dv, codec, oracle):
    """decode_roi writing 360 windows of 4000 x 3000 (4.32 GB) from repeated offsets of three 4096 x 3072 frames."""
    import torch
    W, H, k, n = 4096, 3072, 3, 360
    x, y, rw, rh = 40, 33, 4000, 3000
    src = far.guarded((k, H, W), torch.uint8)
    codec.synth_frames("mixed", SEED, 0, k, W, H, out=src.t)
    cap = k * dv.max_frame_bytes(W, H)
    stream = far.guarded((cap,), torch.uint8)
    offs, sizes = codec.encode_frames(src.t, W, H, k, stream.buf, stream.lead, cap)
    codec.sync()
    total = int((offs[-1] + sizes[-1]).item())
    rep = offs.repeat(n // k)
    win = far.guarded((n, rh, rw), torch.uint8)
    plan = dv.roi_plan(W, H, n, x, y, rw, rh)
    assert (plan["tile_x"], plan["tiles_x"], plan["tile_y"], plan["tiles_y"]) == (5, 500, 4, 376), plan
    _, res = codec.decode_roi(stream.buf, stream.lead, total, rep, W, H, n, x, y, rw, rh, out=win.t)
    codec.sync()
    win.check("windows")
    assert n * rw * rh > G32
    want = src.t[:, y:y + rh, x:x + rw]
    assert bool((win.t.view(n // k, k, rh, rw) == want.unsqueeze(0)).all()), "windows past 2^32 differ"
    assert torch.equal(res[:, 3], sizes.repeat(n // k))
