"""GPU: DBDE16 region traces -- dbde16_hip_traces (Codec.traces16).

Expected values are int64 torch reductions over the label map of the images dbde16_hip_decode_frames writes (checked
against the DBDE16 oracle's decode by Batch16), and for crafted frames (tests/crafted.py, bits=16: wrapping U16 minima,
broken rules) of the numpy decoder's images.  Rejected frames keep their rows; results rows are
dbde16_hip_decode_frames' own.
"""
import numpy as np
import pytest

from test_gpu_project16 import Crafted16
from test_gpu_roi16 import Batch16, images16
from test_gpu_traces import ALL, GUARD, MAPS, SENTINEL, assert_traces, map_blocks, map_discs, reduce_labels
from test_oracle_u16 import o16   # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


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


def gpu_images(b):
    import torch
    return torch.from_numpy(b.gpu_full.astype(np.int32)).cuda()


def traces16(codec, b, tm, **kw):
    tr, res = codec.traces16(b.buf, b.lead, b.total, b.offs, b.W, b.H, b.n, tm, **kw)
    codec.sync()
    return tr, res


_batches = {}


def batch16(codec, o16, kind, W, H, n, seed=1):
    key = (id(codec), kind, W, H, n, seed)
    if key not in _batches:
        _batches[key] = Batch16(codec, o16, images16(np.random.default_rng(seed), n, W, H, kind))
    return _batches[key]


SHAPES = [(64, 64, 5), (100, 75, 4), (1921, 1081, 2), (4096, 3072, 2)]
KINDS = ("mixed", "full", "depth0", "depth16")
CASES = [(W, H, n, kind) for (W, H, n) in SHAPES for kind in sorted(MAPS) if kind != "max_labels" or W * H <= 100 * 75]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("W,H,n,mp", CASES)
def test_traces16_match_decoded_images(dv, codec, o16, kind, W, H, n, mp):
    import torch
    b = batch16(codec, o16, kind, W, H, n)
    labels, L = MAPS[mp](W, H)
    tm = codec.trace_map(labels, L)
    tr, res = traces16(codec, b, tm)
    assert_traces(tr, reduce_labels(gpu_images(b), labels, L, pix_max=65535), what=f"{kind} {W}x{H} {mp}")
    assert codec.parse_results(res) == [(2, b.first + f, 0, len(b.packed[f])) for f in range(b.n)]
    tm.close()


@pytest.mark.parametrize("stats", [tuple(s for j, s in enumerate(ALL) if m >> j & 1) for m in range(1, 16)])
def test_statistic_subsets_touch_only_their_buffers(dv, codec, o16, stats):
    """U16 outputs at 2-byte (not 4-byte) aligned addresses inside guard canvases."""
    import torch
    W, H, n = 200, 123, 5
    b = batch16(codec, o16, "mixed", W, H, n)
    labels, L = map_discs(W, H, seed=4)
    tm = codec.trace_map(labels, L)
    P = n * L
    canv = {s: torch.full((2 * GUARD + 2 + 8 * P,), SENTINEL, dtype=torch.uint8, device="cuda") for s in ALL}
    views = {}
    for s in ALL:
        if s in ("max", "min"):
            views[s] = canv[s][GUARD + 2: GUARD + 2 + 2 * P].view(torch.int16).view(n, L)
        else:
            views[s] = canv[s][GUARD: GUARD + 8 * P].view(torch.int64).view(n, L)
    out = dv.Traces(*[views[s] if s in stats else None for s in ALL], pixels=tm.pixels)
    tr, _ = traces16(codec, b, tm, out=out)
    assert_traces(tr, reduce_labels(gpu_images(b), labels, L, pix_max=65535), stats, what=str(stats))
    for s in ALL:
        c = canv[s].cpu().numpy()
        if s not in stats:
            assert (c == SENTINEL).all(), f"{s} was not requested but written"
        else:
            lo = GUARD + (2 if s in ("max", "min") else 0)
            hi = lo + (2 if s in ("max", "min") else 8) * P
            assert (c[:lo] == SENTINEL).all() and (c[hi:] == SENTINEL).all(), f"{s}: wrote outside its rows"
    tm.close()


@pytest.mark.parametrize("slot,shift", [(0, 1), (0, 7), (0, 13), (131072 + 3, 0), (200000, 5)])
def test_layouts_and_stream_bases(dv, codec, o16, slot, shift):
    W, H, n = 333, 97, 5
    rng = np.random.default_rng(slot + shift)
    maxf = int(codec.L.dbde16_hip_max_frame_bytes(W, H))
    b = Batch16(codec, o16, images16(rng, n, W, H, "mixed"), slot_stride=slot and max(slot, maxf), shift=shift)
    labels, L = map_discs(W, H, seed=5)
    tm = codec.trace_map(labels, L)
    tr, _ = traces16(codec, b, tm)
    assert_traces(tr, reduce_labels(gpu_images(b), labels, L, pix_max=65535), what=f"slot {slot} shift {shift}")
    tm.close()


def test_stream_end_at_every_residue(dv, codec, o16):
    W, H, n = 37, 29, 2
    labels = np.ones((H, W), np.int32)
    labels[H // 2:, :] = 2
    imgs = images16(np.random.default_rng(9), n, W, H, "depth16")
    for shift in range(16):
        b = Batch16(codec, o16, imgs, shift=shift)
        tm = codec.trace_map(labels)
        tr, _ = traces16(codec, b, tm)
        assert_traces(tr, reduce_labels(gpu_images(b), labels, 2, pix_max=65535), what=f"shift {shift}")
        tm.close()


@pytest.mark.parametrize("W,H,n,how", [(64, 48, 30, "concat"), (200, 123, 23, "residues"), (1921, 17, 9, "slots"),
                                       (8, 8, 70, "offsets")])
def test_crafted_and_rejected_frames(dv, codec, W, H, n, how):
    import torch
    rng = np.random.default_rng(W * 7919 + H + 16)
    s = Crafted16(rng, W, H, n, how)
    assert any(im is None for im in s.images) and any(im is not None for im in s.images)
    _, want_res = codec.decode_frames16(s.buf, s.lead, s.total, s.offs, W, H, n)
    labels, L = map_discs(W, H, seed=6)
    tm = codec.trace_map(labels, L)
    out = dv.Traces(torch.full((n, L), 0x3C3C, dtype=torch.int16, device="cuda"),
                    torch.full((n, L), 0x3C3C, dtype=torch.int16, device="cuda"),
                    torch.full((n, L), -7, dtype=torch.int64, device="cuda"),
                    torch.full((n, L), -9, dtype=torch.int64, device="cuda"), tm.pixels)
    tr, res = codec.traces16(s.buf, s.lead, s.total, s.offs, W, H, n, tm, out=out)
    codec.sync()
    assert torch.equal(res, want_res)
    ok = [f for f in range(n) if s.images[f] is not None]
    bad = [f for f in range(n) if s.images[f] is None]
    imgs = torch.from_numpy(np.stack([s.images[f] if s.images[f] is not None else np.zeros((H, W), np.uint16)
                                      for f in range(n)]).astype(np.int32)).cuda()
    assert_traces(tr, reduce_labels(imgs, labels, L, pix_max=65535), rows=ok, what=f"crafted {W}x{H}")
    r = torch.as_tensor(bad, device="cuda")
    assert (tr.max[r] == 0x3C3C).all() and (tr.min[r] == 0x3C3C).all()
    assert (tr.sum[r] == -7).all() and (tr.sumsq[r] == -9).all()
    tm.close()


def test_wrapping_minima_reduce_as_decoded_values(dv, codec):
    import torch
    import crafted as cr
    rng = np.random.default_rng(6)
    W, H, n = 40, 24, 6
    frames = [cr.craft(rng, W, H, 16, "max", "max" if f % 2 else "boundary", "ones" if f % 3 else "random",
                       header=(2, f, 0)) for f in range(n)]
    images = [cr.decode_frame(fr, W, H, 16)[2] for fr in frames]
    assert all(im is not None for im in images)
    buf, lead, offs, total = cr.layout(frames, "concat", lead=32)
    b, o = torch.from_numpy(buf).cuda(), torch.from_numpy(offs).cuda()
    labels, L = map_discs(W, H, seed=7, count=6)
    tm = codec.trace_map(labels, L)
    tr, _ = codec.traces16(b, lead, total, o, W, H, n, tm)
    codec.sync()
    want = reduce_labels(torch.from_numpy(np.stack(images).astype(np.int32)).cuda(), labels, L, pix_max=65535)
    assert_traces(tr, want, what="wrapping minima")
    tm.close()


def test_flat_65535_frame_sums_beyond_u32(dv, codec, o16):
    """One label over a whole flat-65,535 4096 x 3072 frame: sum 824,621,137,920 and sum of squares
    54,041,546,273,587,200, both far above 2^32."""
    W, H, n = 4096, 3072, 1
    b = Batch16(codec, o16, np.full((n, H, W), 65535, np.uint16))
    tm = codec.trace_map(np.ones((H, W), np.int32))
    tr, _ = traces16(codec, b, tm)
    P = W * H
    assert int(tr.sum[0, 0]) == 65535 * P and 65535 * P > 2 ** 32
    assert int(tr.sumsq[0, 0]) == 65535 * 65535 * P
    assert int(tr.max[0, 0].item()) & 0xFFFF == 65535 and int(tr.min[0, 0].item()) & 0xFFFF == 65535
    tm.close()


def test_one_call_equals_row_slices(dv, codec, o16):
    import torch
    W, H, n = 250, 130, 19
    b = batch16(codec, o16, "mixed", W, H, n)
    labels, L = map_blocks(W, H, 24)
    tm = codec.trace_map(labels, L)
    one, _ = traces16(codec, b, tm)
    out = dv.Traces.empty(n, L, ALL, "cuda", pix=2, pixels=tm.pixels)
    for lo, hi in [(0, 2), (2, 11), (11, n)]:
        part = dv.Traces(out.max[lo:hi], out.min[lo:hi], out.sum[lo:hi], out.sumsq[lo:hi], tm.pixels)
        codec.traces16(b.buf, b.lead, b.total, b.offs[lo:hi], W, H, hi - lo, tm, out=part)
    codec.sync()
    for s in ALL:
        assert torch.equal(getattr(out, s), getattr(one, s)), s
    assert_traces(one, reduce_labels(gpu_images(b), labels, L, pix_max=65535), what="one call")
    tm.close()


def test_argument_errors(dv, codec, o16):
    import torch
    W, H = 64, 64
    b = batch16(codec, o16, "mixed", W, H, 5)
    tm = codec.trace_map(map_blocks(W, H)[0])
    L = tm.n_labels
    odd = torch.zeros(2 * 2 * L + 2, dtype=torch.uint8, device="cuda")[1:1 + 2 * 2 * L]
    with pytest.raises(dv.DbdeError):   # an unaligned U16 output
        codec.traces16(b.buf, b.lead, b.total, b.offs, W, H, 2, tm, out=dv.Traces(max=odd, pixels=tm.pixels))
    with pytest.raises(dv.DbdeError):   # W / H other than the map's
        codec.traces16(b.buf, b.lead, b.total, b.offs, 72, 64, 2, tm)
    assert codec.L.dbde16_hip_traces(codec.h, None, 0, None, W, H, 2, None, None, None, None, None, None) == dv.ERR_ARG
    tm.close()
