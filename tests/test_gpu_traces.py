"""GPU: region traces -- dbde_hip_traces (Codec.traces, Codec.trace_map).

Expected values are int64 torch reductions (scatter_reduce amax / amin, scatter_add) over the label map of the images
dbde_hip_decode_frames writes for the same frames; for crafted frames (tests/crafted.py: wrapping minima, broken rules)
over the numpy decoder's images.  They must be equal, not close.  Rejected frames' rows must keep their sentinel, and
the results rows must be dbde_hip_decode_frames' own.
"""
import numpy as np
import pytest

from family_refs import map_discs, reduce_labels   # noqa: F401  (used here and imported from here)
from test_gpu_project import Batch, Crafted

pytestmark = pytest.mark.gpu

ALL = ("max", "min", "sum", "sumsq")
MODES = ("noise8", "mixed", "flat", "smooth")
GUARD = 40
SENTINEL = 0x5A


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


# ---- label maps ----------------------------------------------------------------------------------------------------
def map_blocks(W, H, b=16):
    """8-aligned blocks of b x b, one label each: only whole tiles where the frame is a multiple of 8."""
    by, bx = np.mgrid[0:H, 0:W]
    nbx = (W + b - 1) // b
    lab = (by // b) * nbx + (bx // b) + 1
    lab[(by // b + bx // b) % 3 == 2] = 0
    return lab.astype(np.int32), int(lab.max())


def map_pixels(W, H, seed=2):
    """Single-pixel labels scattered over the frame."""
    rng = np.random.default_rng(seed)
    lab = np.zeros((H, W), np.int32)
    k = min(W * H, 500)
    idx = rng.choice(W * H, size=k, replace=False)
    lab.reshape(-1)[idx] = np.arange(1, k + 1)
    return lab, k


def map_edges(W, H):
    """Regions only in the last tile column and the last tile row."""
    lab = np.zeros((H, W), np.int32)
    lab[:, 8 * ((W - 1) // 8):] = 1
    lab[8 * ((H - 1) // 8):, :] = 2
    return lab, 3   # label 3 has no pixels


def map_empty(W, H):
    return np.zeros((H, W), np.int32), 5


def map_max_labels(W, H, seed=3):
    """n_labels = 65,535 with random labels, the largest among them."""
    rng = np.random.default_rng(seed)
    lab = rng.integers(0, 65536, size=(H, W)).astype(np.int32)
    lab[0, 0] = 65535
    return lab, 65535


MAPS = {"discs": map_discs, "blocks": map_blocks, "pixels": map_pixels, "edges": map_edges, "empty": map_empty,
        "max_labels": map_max_labels}


# ---- expected values -----------------------------------------------------------------------------------------------
def values(t):
    """A trace output as int64 (max / min int16 tensors hold U16 bits)."""
    import torch
    if t.dtype == torch.int16:
        return t.to(torch.int32) & 0xFFFF
    return t.to(torch.int64)


def assert_traces(tr, want, stats=ALL, rows=None, what=""):
    """rows: the frames whose rows are compared (default all)."""
    import torch
    for s in ALL:
        got = getattr(tr, s)
        if s not in stats:
            assert got is None, (what, s)
            continue
        g, e = values(got), want[s].to(got.device)
        if rows is not None:
            r = torch.as_tensor(rows, device=got.device)
            g, e = g[r], e[r]
        if not torch.equal(g.to(torch.int64), e.to(torch.int64)):
            bad = (g.to(torch.int64) != e).nonzero()[0].tolist()
            raise AssertionError(f"{what}: {s} differs at (frame, label - 1) {bad}: {int(g[tuple(bad)])} != "
                                 f"{int(e[tuple(bad)])}")


_batches = {}


def batch(codec, mode, W, H, n):
    key = (id(codec), mode, W, H, n)
    if key not in _batches:
        _batches[key] = Batch(codec, mode, W, H, n)
    return _batches[key]


SHAPES = [(64, 64, 9), (100, 75, 7), (1921, 1081, 3), (4096, 3072, 2)]


# n_labels = 65,535 on the small shapes only (its (n, 65,535) reference is the costly part)
CASES = [(W, H, n, kind) for (W, H, n) in SHAPES for kind in sorted(MAPS) if kind != "max_labels" or W * H <= 100 * 75]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W,H,n,kind", CASES)
def test_traces_match_decoded_images(dv, codec, mode, W, H, n, kind):
    import torch
    labels, L = MAPS[kind](W, H)
    b = batch(codec, mode, W, H, n)
    tm = codec.trace_map(labels, L)
    tr, res = codec.traces(b.buf, b.lead, b.total, b.offs, W, H, n, tm)
    codec.sync()
    assert_traces(tr, reduce_labels(b.images, labels, L), what=f"{mode} {W}x{H} {kind}")
    assert torch.equal(res, b.results)
    assert torch.equal(tr.pixels.cpu(), torch.from_numpy(np.bincount(labels.reshape(-1), minlength=L + 1)[1:]))
    tm.close()


@pytest.mark.parametrize("stats", [tuple(s for j, s in enumerate(ALL) if m >> j & 1) for m in range(1, 16)])
@pytest.mark.parametrize("odd", [0, 1, 3])
def test_statistic_subsets_touch_only_their_buffers(dv, codec, stats, odd):
    """Every output sits in a guard canvas; the requested ones are written inside their n x L rows only, the others
    are never touched.  U8 outputs at odd byte offsets."""
    import torch
    W, H, n = 200, 123, 7
    b = batch(codec, "mixed", W, H, n)
    labels, L = map_discs(W, H, seed=4)
    tm = codec.trace_map(labels, L)
    P = n * L
    canv = {s: torch.full((2 * GUARD + odd + (8 if s in ("sum", "sumsq") else 1) * P,), SENTINEL, dtype=torch.uint8,
                          device="cuda") for s in ALL}
    views = {}
    for s in ALL:
        if s in ("max", "min"):
            views[s] = canv[s][GUARD + odd: GUARD + odd + P].view(n, L)
        else:
            views[s] = canv[s][GUARD: GUARD + 8 * P].view(torch.int64).view(n, L)
    out = dv.Traces(*[views[s] if s in stats else None for s in ALL], pixels=tm.pixels)
    tr, _ = codec.traces(b.buf, b.lead, b.total, b.offs, W, H, n, tm, out=out)
    codec.sync()
    assert tr is out
    assert_traces(tr, reduce_labels(b.images, labels, L), stats, what=str(stats))
    for s in ALL:
        c = canv[s].cpu().numpy()
        if s not in stats:
            assert (c == SENTINEL).all(), f"{s} was not requested but written"
        else:
            lo = GUARD + (odd if s in ("max", "min") else 0)
            hi = lo + (8 if s in ("sum", "sumsq") else 1) * P
            assert (c[:lo] == SENTINEL).all() and (c[hi:] == SENTINEL).all(), f"{s}: wrote outside its rows"
    tm.close()


@pytest.mark.parametrize("slot,misalign", [(0, 1), (0, 3), (0, 6), (4096 * 3 + 5, 0), (20000, 2)])
def test_layouts(dv, codec, slot, misalign):
    """Concatenated streams at misaligned leads and slot layouts; stream_bytes ends exactly at the last frame."""
    import torch
    W, H, n = 100, 75, 11
    b = Batch(codec, "mixed", W, H, n, slot_stride=slot, misalign=misalign)
    labels, L = map_discs(W, H, seed=5)
    tm = codec.trace_map(labels, L)
    tr, res = codec.traces(b.buf, b.lead, b.total, b.offs, W, H, n, tm)
    codec.sync()
    assert_traces(tr, reduce_labels(b.images, labels, L), what=f"slot {slot} misalign {misalign}")
    assert torch.equal(res, b.results)
    tm.close()


def test_stream_end_at_every_residue(dv, codec):
    """stream_bytes ends exactly at the last frame's last byte, with that end at every residue mod 16."""
    W, H, n = 37, 29, 3
    labels = np.ones((H, W), np.int32)
    labels[:, W // 2:] = 2
    for misalign in range(16):
        b = Batch(codec, "noise8", W, H, n, misalign=misalign)
        tm = codec.trace_map(labels)
        tr, _ = codec.traces(b.buf, b.lead, b.total, b.offs, W, H, n, tm)
        codec.sync()
        assert_traces(tr, reduce_labels(b.images, labels, 2), what=f"end residue {(b.lead + b.total) % 16}")
        tm.close()


@pytest.mark.parametrize("W,H,n,how", [(64, 48, 40, "concat"), (200, 123, 23, "residues"), (1921, 17, 9, "slots"),
                                       (8, 8, 70, "offsets"), (4200, 9, 7, "concat")])
def test_crafted_and_rejected_frames(dv, codec, W, H, n, how):
    """Rejected frames keep their rows as they were (sentinels); accepted ones equal the numpy decoder's images."""
    import torch
    rng = np.random.default_rng(W * 7919 + H)
    s = Crafted(rng, W, H, n, how)
    assert any(im is None for im in s.images) and any(im is not None for im in s.images)
    _, want_res = codec.decode_frames(s.buf, s.lead, s.total, s.offs, W, H, n)
    labels, L = map_discs(W, H, seed=6)
    tm = codec.trace_map(labels, L)
    out = dv.Traces(torch.full((n, L), 0x3C, dtype=torch.uint8, device="cuda"),
                    torch.full((n, L), 0x3C, dtype=torch.uint8, device="cuda"),
                    torch.full((n, L), -7, dtype=torch.int64, device="cuda"),
                    torch.full((n, L), -9, dtype=torch.int64, device="cuda"), tm.pixels)
    tr, res = codec.traces(s.buf, s.lead, s.total, s.offs, W, H, n, tm, out=out)
    codec.sync()
    assert torch.equal(res, want_res)
    ok = [f for f in range(n) if s.images[f] is not None]
    bad = [f for f in range(n) if s.images[f] is None]
    imgs = torch.from_numpy(np.stack([s.images[f] if s.images[f] is not None else np.zeros((H, W), np.uint8)
                                      for f in range(n)])).cuda()
    assert_traces(tr, reduce_labels(imgs, labels, L), rows=ok, what=f"crafted {W}x{H}")
    r = torch.as_tensor(bad, device="cuda")
    assert (tr.max[r] == 0x3C).all() and (tr.min[r] == 0x3C).all()
    assert (tr.sum[r] == -7).all() and (tr.sumsq[r] == -9).all()
    tm.close()


def test_wrapping_minima_reduce_as_decoded_bytes(dv, codec):
    """Every tile at the maximum minimum with a full payload: min + value wraps modulo 256 in nearly every pixel."""
    import torch
    import crafted as cr
    rng = np.random.default_rng(5)
    W, H, n = 40, 24, 6
    frames = [cr.craft(rng, W, H, 8, "max", "max" if f % 2 else "boundary", "ones" if f % 3 else "random",
                       header=(2, f, 0)) for f in range(n)]
    images = [cr.decode_frame(fr, W, H)[2] for fr in frames]
    assert all(im is not None for im in images)
    buf, lead, offs, total = cr.layout(frames, "concat", lead=32)
    b, o = torch.from_numpy(buf).cuda(), torch.from_numpy(offs).cuda()
    labels, L = map_discs(W, H, seed=7, count=6)
    tm = codec.trace_map(labels, L)
    tr, _ = codec.traces(b, lead, total, o, W, H, n, tm)
    codec.sync()
    assert_traces(tr, reduce_labels(torch.from_numpy(np.stack(images)).cuda(), labels, L), what="wrapping minima")
    tm.close()


def test_sums_beyond_u32(dv, codec):
    """One label over a whole flat-255 4096 x 3072 frame: sum 3,208,642,560 (above 2^31), sum of squares
    818,203,852,800 (above 2^32)."""
    import torch
    W, H, n = 4096, 3072, 2
    imgs = torch.full((n, H, W), 255, dtype=torch.uint8, device="cuda")
    b = Batch(codec, None, W, H, n, images=imgs)
    tm = codec.trace_map(np.ones((H, W), np.int32))
    assert tm.info["tiles_whole"] == tm.info["tiles"]
    tr, _ = codec.traces(b.buf, b.lead, b.total, b.offs, W, H, n, tm)
    codec.sync()
    assert 3_208_642_560 > 2 ** 31 and 255 * 3_208_642_560 > 2 ** 32
    assert (tr.sum == 3_208_642_560).all() and (tr.sumsq == 255 * 3_208_642_560).all()
    assert (tr.max == 255).all() and (tr.min == 255).all()
    assert torch.allclose(tr.mean(), torch.full((n, 1), 255.0, dtype=torch.float64, device="cuda"))
    assert torch.allclose(tr.std(), torch.zeros((n, 1), dtype=torch.float64, device="cuda"))


def test_one_call_equals_row_slices(dv, codec):
    """One batch traced in one call equals the same frames traced in several calls into row slices of one output."""
    import torch
    W, H, n = 333, 222, 41
    b = batch(codec, "noise8", W, H, n)
    labels, L = map_discs(W, H, seed=8)
    tm = codec.trace_map(labels, L)
    one, _ = codec.traces(b.buf, b.lead, b.total, b.offs, W, H, n, tm)
    out = dv.Traces.empty(n, L, ALL, "cuda", pixels=tm.pixels)
    for lo, hi in [(0, 1), (1, 9), (9, 30), (30, n)]:
        part = dv.Traces(out.max[lo:hi], out.min[lo:hi], out.sum[lo:hi], out.sumsq[lo:hi], tm.pixels)
        codec.traces(b.buf, b.lead, b.total, b.offs[lo:hi], W, H, hi - lo, tm, out=part)
    codec.sync()
    for s in ALL:
        assert torch.equal(getattr(out, s), getattr(one, s)), s
    assert_traces(one, reduce_labels(b.images, labels, L), what="one call")
    m = one.mean()
    empty = tm.pixels == 0
    assert torch.isnan(m[:, empty]).all() and not torch.isnan(m[:, ~empty]).any()
    tm.close()


def test_zero_frames_does_nothing(dv, codec):
    import torch
    W, H = 64, 64
    b = batch(codec, "mixed", W, H, 9)
    tm = codec.trace_map(map_blocks(W, H)[0])
    out = dv.Traces(torch.full((1, tm.n_labels), 7, dtype=torch.uint8, device="cuda"), None, None, None, tm.pixels)
    codec.traces(b.buf, b.lead, b.total, b.offs, W, H, 0, tm, out=out)
    codec.sync()
    assert (out.max == 7).all()
    tm.close()


def test_two_codecs_at_once(dv):
    """Two contexts on their own streams, each with its own map, queued together."""
    import torch
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    c1, c2 = dv.Codec(0, stream=s1), dv.Codec(0, stream=s2)
    try:
        with torch.cuda.stream(s1):
            b1 = Batch(c1, "mixed", 640, 480, 32)
        with torch.cuda.stream(s2):
            b2 = Batch(c2, "noise8", 333, 222, 60)
        torch.cuda.synchronize()
        l1, L1 = map_discs(640, 480, seed=9)
        l2, L2 = map_blocks(333, 222, 24)
        m1, m2 = c1.trace_map(l1, L1), c2.trace_map(l2, L2)
        for _ in range(3):
            with torch.cuda.stream(s1):
                t1, _ = c1.traces(b1.buf, b1.lead, b1.total, b1.offs, 640, 480, 32, m1)
            with torch.cuda.stream(s2):
                t2, _ = c2.traces(b2.buf, b2.lead, b2.total, b2.offs, 333, 222, 60, m2)
            torch.cuda.synchronize()
            assert_traces(t1, reduce_labels(b1.images, l1, L1), what="codec 1")
            assert_traces(t2, reduce_labels(b2.images, l2, L2), what="codec 2")
        with pytest.raises(dv.DbdeError):   # a map of another codec
            c1.traces(b1.buf, b1.lead, b1.total, b1.offs, 333, 222, 1, m2)
        m1.close()
        m2.close()
    finally:
        c1.close()
        c2.close()


def test_argument_errors(dv, codec):
    import torch
    W, H = 64, 64
    b = batch(codec, "flat", W, H, 9)
    tm = codec.trace_map(map_blocks(W, H)[0])
    L = tm.n_labels
    with pytest.raises(dv.DbdeError):   # W / H other than the map's
        codec.traces(b.buf, b.lead, b.total, b.offs, 64, 56, 2, tm)
    with pytest.raises(dv.DbdeError):   # no statistic
        codec.traces(b.buf, b.lead, b.total, b.offs, W, H, 2, tm, out=dv.Traces(pixels=tm.pixels))
    buf = torch.zeros(8 * 2 * L + 8, dtype=torch.uint8, device="cuda")
    odd = buf[1:1 + 8 * 2 * L]
    with pytest.raises(dv.DbdeError):   # an unaligned U64 output
        codec.traces(b.buf, b.lead, b.total, b.offs, W, H, 2, tm, out=dv.Traces(sum=odd, pixels=tm.pixels))
    L_ = codec.L
    rc = L_.dbde_hip_traces(codec.h, None, 0, None, W, H, 2, None, None, None, None, None, None)
    assert rc == dv.ERR_ARG
    rc = L_.dbde_hip_traces(codec.h, b.buf.data_ptr(), b.total, b.offs.data_ptr(), W, H, 2, tm.h, None, None, None,
                            None, None)
    assert rc == dv.ERR_ARG
    with pytest.raises(ValueError):
        codec.trace_map(np.full((H, W), 3, np.int32), 2)
    tm.close()
