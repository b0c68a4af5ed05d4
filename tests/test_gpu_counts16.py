"""GPU: count projections of DBDE16 streams -- dbde16_hip_project_counts (Codec.project_counts16).

test_gpu_counts.py's checks with U16 pixels and thresholds: every plane equal to tests/counts_ref.py over the DBDE16
oracle's decode of encoded batches (Batch16 holds it equal to dbde16_hip_decode_frames').
"""
import numpy as np
import pytest

import counts_gpu as cg
import counts_ref as cref
import far
import wproject_gpu as wg
from test_gpu_roi16 import Batch16, images16
from test_oracle_u16 import o16   # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

# edge tiles in both directions, and a frame of five pieces of 16 tiles (520 > 128 pixels)
SHAPES = [(72, 40), (100, 50), (520, 16)]
COUNTS = (1, 3, 4, 5, 13)
LEVELS = (1, 2, 7, 8)
NMAX = 13
BITS = 16


def windows(W, H):
    out = [(0, 0, W, H), (3, 5, 41, min(27, H - 5)), (W // 2 + 1, H - 2, 1, 1)]
    if W > 256:
        out.append((251, 1, 13, H - 2))       # across the boundary of two pieces (pixel 256)
    return out


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


@pytest.fixture(scope="module")
def cus(codec):
    return wg.cus_of(codec)


def stream_of(codec, o16, imgs, shift=0):   # noqa: F811
    b = Batch16(codec, o16, imgs, shift=shift)
    assert all(np.array_equal(a, g) for a, g in zip(b.full, b.gpu_full))
    return wg.Stream(b.buf, b.lead, b.total, b.offs, b.W, b.H, b.full)


@pytest.fixture(scope="module")
def streams(codec, o16):   # noqa: F811
    cache = {}

    def get(W, H, n=NMAX, kind="mixed"):
        if (W, H, n, kind) not in cache:
            rng = np.random.default_rng(W * 7919 + H * 31 + n)
            cache[(W, H, n, kind)] = stream_of(codec, o16, images16(rng, n, W, H, kind), shift=len(cache) % 4)
        return cache[(W, H, n, kind)]
    return get


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("W,H", SHAPES)
def test_random_thresholds_match_the_reference(dv, codec, streams, W, H, n):
    s = streams(W, H).first(n)
    rng = np.random.default_rng(W * 31 + n + 16)
    for win in windows(W, H):
        for K in LEVELS:
            for maps in (False, True):
                thr = cg.draw(rng, s.images, win, K, BITS, maps)
                _, res = cg.check(codec.project_counts16, s, thr, win, what="random")
                assert [r[1] for r in codec.parse_results(res)] == list(range(n))
    assert dv.counts16_plan(W, H, n)["segments"] == 1
    assert dv.counts16_plan(W, H, n)["pieces_x"] == -(-((W + 7) // 8) // 16)


@pytest.mark.parametrize("kind", ["full", "small", "depth16"])
def test_other_frame_contents(codec, streams, kind):
    """Noise over the whole range, smooth 8-bit content in 16-bit pixels, and tiles of depth 16."""
    W, H, n = 100, 50, 5
    s = streams(W, H, n, kind)
    rng = np.random.default_rng(7)
    for win in windows(W, H)[:2]:
        for maps in (False, True):
            # "small" stays below 32: its thresholds are drawn over the data's range, or every count is 0 or n
            thr = cg.draw(rng, s.images, win, 7, BITS, maps, over_data=kind == "small")
            cg.check(codec.project_counts16, s, thr, win, what=kind)


def test_flat_frames(codec, o16):   # noqa: F811
    """Every pixel of every frame holds one value v: thresholds v - 1, v and v + 1 count 0, n and n."""
    W, H, n, v = 100, 50, 5, 0x1234
    s = stream_of(codec, o16, np.full((n, H, W), v, np.uint16))
    for win in windows(W, H)[:2]:
        thr = np.array([v - 1, v, v + 1], np.uint16)
        out, _ = cg.check(codec.project_counts16, s, thr, win, what="flat scalars")
        got = cg.planes(out)
        assert (got[0] == 0).all() and (got[1] == n).all() and (got[2] == n).all()
        m = np.broadcast_to(thr[:, None, None], (3, win[3], win[2])).copy()
        m[:, ::2, 1::2] += 1
        cg.check(codec.project_counts16, s, m, win, what="flat maps")


@pytest.mark.parametrize("W,H", SHAPES)
def test_threshold_families(codec, streams, W, H):
    s = streams(W, H)
    n = s.n
    for j, win in enumerate(windows(W, H)):
        x, y, rw, rh = win
        st = cg.window_stack(s.images, win)
        own = np.stack([st[(j + k) % n] for k in range(3)])
        assert (st[None] == own[:, None]).any(), "ties"
        le = (st[None] <= own[:, None]).sum(1)
        lt = (st[None] < own[:, None]).sum(1)
        assert not np.array_equal(le, lt)
        out, _ = cg.check(codec.project_counts16, s, own, win, what="a frame's own pixels")
        assert (cg.planes(out) >= 1).all()
        below = np.where(own > 0, own - 1, 0).astype(np.uint16)
        out, _ = cg.check(codec.project_counts16, s, below, win, what="own pixels minus one")
        assert np.array_equal(cg.planes(out), np.where(own > 0, lt, le))
        for K in (1, 8):
            for shape in ((K,), (K, rh, rw)):
                cg.check(codec.project_counts16, s, np.zeros(shape, np.uint16), win, what="all zero")
                out, _ = cg.check(codec.project_counts16, s, np.full(shape, 65535, np.uint16), win, what="all maximum")
                assert (cg.planes(out) == n).all()


def test_the_compare_is_unsigned(codec, o16):   # noqa: F811
    """Flat images of 40000 against 1000, 39999, 40000, 65535: a signed 16-bit compare (40000 = -25536) would count
    1000 and not 65535."""
    W, H, n = 72, 40, 3
    s = stream_of(codec, o16, np.full((n, H, W), 40000, np.uint16))
    thr = np.array([1000, 39999, 40000, 65535], np.uint16)
    for win in windows(W, H):
        for t in (thr, np.broadcast_to(thr[:, None, None], (4, win[3], win[2])).copy()):
            out, _ = cg.check(codec.project_counts16, s, t, win, what="unsigned")
            got = cg.planes(out)
            assert (got[0] == 0).all() and (got[1] == 0).all() and (got[2] == n).all() and (got[3] == n).all()


@pytest.mark.parametrize("n", [50, 70])
def test_segments(dv, codec, cus, streams, n):
    import torch
    W, H = 72, 40
    s = streams(W, H, 70, "full").first(n)
    rng = np.random.default_rng(n)
    for win in [(0, 0, W, H), (3, 5, 41, 27)]:
        for K in (1, 7, 8):
            for maps in (False, True):
                p = dv.counts16_plan(W, H, n, *win, levels=K, n_cu=cus, maps=maps)
                assert p["segments"] > 1 and p["workspace_bytes"] > 0
                thr = cg.draw(rng, s.images, win, K, BITS, maps)
                out, _ = cg.check(codec.project_counts16, s, thr, win, what="segments")
                cut = 37
                assert dv.counts16_plan(W, H, cut, *win, levels=K, n_cu=cus)["segments"] > 1
                two, _ = codec.project_counts16(s.buf, s.lead, s.total, s.offs, W, H, cut, cg.device(thr), *win)
                codec.project_counts16(s.buf, s.lead, s.total, s.offs[cut:], W, H, n - cut, cg.device(thr), *win, out=two,
                                       accumulate=True)
                codec.sync()
                assert torch.equal(two.out, out.out) and int(two.count.item()) == n


@pytest.mark.parametrize("cut", [1, 4, 6])
def test_accumulate_split_equals_one_call(codec, streams, cut):
    import torch
    W, H, n = 100, 50, 13
    full = streams(W, H)
    rng = np.random.default_rng(cut)
    win = (3, 5, 41, 27)
    for K, maps in ((2, False), (8, True)):
        thr = cg.draw(rng, full.images, win, K, BITS, maps)
        one, _ = cg.check(codec.project_counts16, full, thr, win, what="one call")
        out, _ = cg.check(codec.project_counts16, full.first(cut), thr, win, what="first part")
        codec.project_counts16(full.buf, full.lead, full.total, full.offs[cut:], W, H, n - cut, cg.device(thr), *win,
                               out=out, accumulate=True)
        codec.sync()
        assert torch.equal(out.out, one.out) and int(out.count.item()) == n
        codec.project_counts16(full.buf, full.lead, full.total, full.offs, W, H, 0, cg.device(thr), *win, out=out,
                               accumulate=True)
        codec.sync()
        assert torch.equal(out.out, one.out) and int(out.count.item()) == n
        codec.project_counts16(full.buf, full.lead, full.total, full.offs, W, H, 0, cg.device(thr), *win, out=out)
        codec.sync()
        assert (out.out == 0).all() and int(out.count.item()) == 0


def test_guarded_outputs_eleven_levels_and_level_slices(dv, codec, streams):
    import torch
    W, H, n = 100, 50, 13
    s = streams(W, H)
    win = (3, 5, 41, 27)
    x, y, rw, rh = win
    rng = np.random.default_rng(n)
    for maps in (False, True):
        K = 11
        thr = cg.draw(rng, s.images, win, K, BITS, maps)
        want, _ = cref.counts(s.images, thr, *win)
        g = far.guarded((K, rh, rw), torch.int32)
        count = torch.full((3,), -7, dtype=torch.int64, device="cuda")
        out = dv.CountProjection(g.t, count[1:2])
        codec.project_counts16(s.buf, s.lead, s.total, s.offs, W, H, n, cg.device(thr), *win, out=out)
        codec.sync()
        g.check(f"K = 11, maps={maps}")
        assert np.array_equal(cg.planes(out), want)
        assert count.tolist() == [-7, n, -7]
        del g
    far.free()
    thr = cg.draw(rng, s.images, win, 5, BITS, True)
    wide = torch.full((9, rh, rw), 777, dtype=torch.int16, device="cuda")
    wide[2:7] = cg.device(thr)
    out, _ = codec.project_counts16(s.buf, s.lead, s.total, s.offs, W, H, n, wide[2:7], *win)
    codec.sync()
    assert np.array_equal(cg.planes(out), cref.counts(s.images, thr, *win)[0])
    with pytest.raises(ValueError):
        codec.project_counts16(s.buf, s.lead, s.total, s.offs, W, H, n, [70000], *win)
    a, _ = codec.project_counts16(s.buf, s.lead, s.total, s.offs, W, H, n, [1000, 40000, 65535], *win)
    codec.sync()
    assert np.array_equal(cg.planes(a), cref.counts(s.images, np.array([1000, 40000, 65535], np.uint16), *win)[0])


def test_argument_errors(dv, codec, streams):
    import torch
    W, H = 72, 40
    s = streams(W, H)
    L, h = codec.L, codec.h
    thr = torch.zeros((9, H, W), dtype=torch.int16, device="cuda")
    out = torch.zeros((9, H, W), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")

    def rc(n=13, tp=None, K=2, stride=W * H, flags=1, op=None, cp=None):
        return L.dbde16_hip_project_counts(h, s.buf.data_ptr() + s.lead, s.total, s.offs.data_ptr(), W, H, n, 0, 0, W, H,
                                           thr.data_ptr() if tp is None else tp, K, stride, 0, flags,
                                           out.data_ptr() if op is None else op, cnt.data_ptr() if cp is None else cp, None)
    assert rc() == dv.OK
    assert rc(tp=thr.data_ptr() + 2) == dv.OK
    for kw in (dict(K=0), dict(K=9), dict(stride=W * H - 1), dict(flags=2), dict(tp=thr.data_ptr() + 1),
               dict(op=out.data_ptr() + 2), dict(cp=cnt.data_ptr() + 4), dict(n=-1)):
        assert rc(**kw) == dv.ERR_ARG, kw
    codec.sync()
