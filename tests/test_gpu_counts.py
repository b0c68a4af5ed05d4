"""GPU: count projections -- dbde_hip_project_counts (Codec.project_counts).

Every plane is compared for equality with tests/counts_ref.py -- (images[None] <= thr[:, None]).sum(1) over the accepted
frames in numpy -- on the images dbde_hip_decode_frames writes for encoded batches.  Nothing expected comes from the
call itself.  Random thresholds are drawn on the CPU until every level's expected plane has a pixel with
0 < count < N (one frame: both 0 and 1), so no case passes by counting nothing or everything (counts_gpu.draw).
"""
import numpy as np
import pytest

import counts_gpu as cg
import counts_ref as cref
import far
import wproject_gpu as wg
from test_gpu_project import Batch

pytestmark = pytest.mark.gpu

# edge tiles in both directions (72x40, 100x50) and a frame wider than one piece of 32 tiles (520 > 256 pixels)
SHAPES = [(72, 40), (100, 50), (520, 16)]
COUNTS = (1, 3, 4, 5, 13)       # the four-frame pipeline step's boundaries and tails
LEVELS = (1, 2, 7, 8)
NMAX = 13
BITS = 8


def windows(W, H):
    """The full frame, an unaligned window (x = 3, y = 5, 41 x 27 where the frame has the rows), one pixel; for the
    wide frame a window across the boundary of the two pieces."""
    out = [(0, 0, W, H), (3, 5, 41, min(27, H - 5)), (W // 2 + 1, H - 2, 1, 1)]
    if W > 256:
        out.append((251, 1, 13, H - 2))
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


def stream_of(codec, W, H, n, mode="mixed", images=None):
    b = Batch(codec, mode, W, H, n, images=images)
    return wg.Stream(b.buf, b.lead, b.total, b.offs, W, H, list(b.images.cpu().numpy())), b


@pytest.fixture(scope="module")
def streams(codec):
    cache = {}

    def get(W, H, n=NMAX, mode="mixed"):
        if (W, H, n, mode) not in cache:
            cache[(W, H, n, mode)] = stream_of(codec, W, H, n, mode)
        return cache[(W, H, n, mode)]
    return get


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("W,H", SHAPES)
def test_random_thresholds_match_the_reference(dv, codec, streams, W, H, n):
    """Every window x level count x threshold mode."""
    import torch
    full, b = streams(W, H)
    s = full.first(n)
    rng = np.random.default_rng(W * 31 + n)
    for win in windows(W, H):
        for K in LEVELS:
            for maps in (False, True):
                thr = cg.draw(rng, s.images, win, K, BITS, maps)
                _, res = cg.check(codec.project_counts, s, thr, win, what="random")
                assert torch.equal(res, b.results[:n])
    assert dv.counts_plan(W, H, n)["segments"] == 1
    if W > 256:
        assert dv.counts_plan(W, H, n)["pieces_x"] > 1


@pytest.mark.parametrize("mode", ["noise8", "smooth"])
def test_other_frame_contents(codec, streams, mode):
    W, H, n = 100, 50, 5
    s, _ = streams(W, H, n, mode)
    rng = np.random.default_rng(7)
    for win in windows(W, H)[:2]:
        for maps in (False, True):
            # smooth content stays below 32: its thresholds are drawn over the data's range
            thr = cg.draw(rng, s.images, win, 7, BITS, maps, over_data=mode == "smooth")
            cg.check(codec.project_counts, s, thr, win, what=mode)


def test_flat_frames(codec, streams):
    """Every pixel of every frame holds one value v: thresholds v - 1, v and v + 1 count 0, n and n."""
    W, H, n = 100, 50, 5
    s, _ = streams(W, H, n, "flat")
    v = int(s.images[0][0, 0])
    assert all((im == v).all() for im in s.images) and 0 < v < 255
    for win in windows(W, H)[:2]:
        thr = np.array([v - 1, v, v + 1], np.uint8)
        out, _ = cg.check(codec.project_counts, s, thr, win, what="flat scalars")
        got = cg.planes(out)
        assert (got[0] == 0).all() and (got[1] == n).all() and (got[2] == n).all()
        m = np.broadcast_to(thr[:, None, None], (3, win[3], win[2])).copy()
        m[:, ::2, 1::2] += 1      # v, v + 1, v + 2 on a checkerboard's odd columns of even rows
        cg.check(codec.project_counts, s, m, win, what="flat maps")


@pytest.mark.parametrize("W,H", SHAPES)
def test_threshold_families(codec, streams, W, H):
    """Maps equal to one frame's own window pixels (ties p == thr occur, so <= and < differ), that map minus one
    saturating at zero, all zero, and all maximum (every pixel then equals the count of accepted frames)."""
    s, _ = streams(W, H)
    n = s.n
    for j, win in enumerate(windows(W, H)):
        x, y, rw, rh = win
        st = cg.window_stack(s.images, win)
        own = np.stack([st[(j + k) % n] for k in range(3)])
        assert (st[None] == own[:, None]).any(), "ties"
        le = (st[None] <= own[:, None]).sum(1)
        lt = (st[None] < own[:, None]).sum(1)
        assert not np.array_equal(le, lt)
        out, _ = cg.check(codec.project_counts, s, own, win, what="a frame's own pixels")
        assert (cg.planes(out) >= 1).all()                       # the frame itself is at its threshold
        below = np.where(own > 0, own - 1, 0).astype(np.uint8)
        out, _ = cg.check(codec.project_counts, s, below, win, what="own pixels minus one")
        assert np.array_equal(cg.planes(out), np.where(own > 0, lt, le))
        for K in (1, 8):
            for shape in ((K,), (K, rh, rw)):
                cg.check(codec.project_counts, s, np.zeros(shape, np.uint8), win, what="all zero")
                out, _ = cg.check(codec.project_counts, s, np.full(shape, 255, np.uint8), win, what="all maximum")
                assert (cg.planes(out) == n).all()


def test_the_compare_is_unsigned(codec):
    """Flat images of 200 against 100, 199, 200, 255: a signed byte compare (200 = -56) would count 100 and not 255."""
    import torch
    W, H, n = 72, 40, 3
    s, _ = stream_of(codec, W, H, n, images=torch.full((n, H, W), 200, dtype=torch.uint8, device="cuda"))
    thr = np.array([100, 199, 200, 255], np.uint8)
    for win in windows(W, H):
        for t in (thr, np.broadcast_to(thr[:, None, None], (4, win[3], win[2])).copy()):
            out, _ = cg.check(codec.project_counts, s, t, win, what="unsigned")
            got = cg.planes(out)
            assert (got[0] == 0).all() and (got[1] == 0).all() and (got[2] == n).all() and (got[3] == n).all()


@pytest.mark.parametrize("n", [50, 70])
def test_segments(dv, codec, cus, streams, n):
    """A window of few workgroups and n >= 33 frames: the plan cuts S > 1 segments on this device (asserted, not
    assumed).  The result is the reference and equals two accumulating calls over the same n frames."""
    import torch
    W, H = 72, 40
    s, _ = streams(W, H, 70)
    s = s.first(n)
    rng = np.random.default_rng(n)
    for win in [(0, 0, W, H), (3, 5, 41, 27)]:
        for K in (1, 7, 8):
            for maps in (False, True):
                p = dv.counts_plan(W, H, n, *win, levels=K, n_cu=cus, maps=maps)
                assert p["segments"] > 1 and p["workspace_bytes"] > 0
                thr = cg.draw(rng, s.images, win, K, BITS, maps)
                out, _ = cg.check(codec.project_counts, s, thr, win, what="segments")
                cut = 37
                assert dv.counts_plan(W, H, cut, *win, levels=K, n_cu=cus)["segments"] > 1
                two, _ = codec.project_counts(s.buf, s.lead, s.total, s.offs, W, H, cut, cg.device(thr), *win)
                codec.project_counts(s.buf, s.lead, s.total, s.offs[cut:], W, H, n - cut, cg.device(thr), *win, out=two,
                                     accumulate=True)
                codec.sync()
                assert torch.equal(two.out, out.out) and int(two.count.item()) == n


@pytest.mark.parametrize("cut", [1, 4, 6])
def test_accumulate_split_equals_one_call(codec, streams, cut):
    """n = a + b over two calls equals one call, planes and count; n == 0 adds nothing, or zeroes without accumulate."""
    import torch
    W, H, n = 100, 50, 13
    full, _ = streams(W, H)
    rng = np.random.default_rng(cut)
    for win in ((3, 5, 41, 27), (0, 0, W, H)):
        for K, maps in ((2, False), (8, True)):
            thr = cg.draw(rng, full.images, win, K, BITS, maps)
            one, _ = cg.check(codec.project_counts, full, thr, win, what="one call")
            out, _ = cg.check(codec.project_counts, full.first(cut), thr, win, what="first part")
            codec.project_counts(full.buf, full.lead, full.total, full.offs[cut:], W, H, n - cut, cg.device(thr), *win,
                                 out=out, accumulate=True)
            codec.sync()
            assert torch.equal(out.out, one.out) and int(out.count.item()) == n
            codec.project_counts(full.buf, full.lead, full.total, full.offs, W, H, 0, cg.device(thr), *win, out=out,
                                 accumulate=True)
            codec.sync()
            assert torch.equal(out.out, one.out) and int(out.count.item()) == n
            codec.project_counts(full.buf, full.lead, full.total, full.offs, W, H, 0, cg.device(thr), *win, out=out)
            codec.sync()
            assert (out.out == 0).all() and int(out.count.item()) == 0


@pytest.mark.parametrize("n", [13, 70])
def test_guarded_outputs_eleven_levels_and_level_slices(dv, codec, streams, n):
    """The planes sit in a far.guarded canvas (one and several segments) and the guards stay intact.  K = 11 through the
    wrapper (two calls, the frames counted once).  A (K, rh, rw) map passed as a level slice of a wider tensor whose
    other levels hold a different value."""
    import torch
    W, H = 72, 40
    s, _ = streams(W, H, 70)
    s = s.first(n)
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
        got, _ = codec.project_counts(s.buf, s.lead, s.total, s.offs, W, H, n, cg.device(thr), *win, out=out)
        codec.sync()
        assert got is out
        g.check(f"K = 11, maps={maps}")
        assert np.array_equal(cg.planes(out), want)
        assert count.tolist() == [-7, n, -7]
        # 3 levels into the middle of the canvas leave the planes on either side alone
        g.t.fill_(-1)
        mid = dv.CountProjection(g.t[4:7], count[1:2])
        codec.project_counts(s.buf, s.lead, s.total, s.offs, W, H, n, cg.device(thr[4:7]), *win, out=mid)
        codec.sync()
        g.check("planes 4..6")
        assert np.array_equal(cg.planes(mid), want[4:7])
        assert (g.t[:4] == -1).all() and (g.t[7:] == -1).all()
        del g
    far.free()
    # level slices: levels 2..6 of a wider tensor, and every second level (a level stride of two maps)
    thr = cg.draw(rng, s.images, win, 5, BITS, True)
    wide = torch.full((9, rh, rw), 77, dtype=torch.uint8, device="cuda")
    wide[2:7] = cg.device(thr)
    out, _ = codec.project_counts(s.buf, s.lead, s.total, s.offs, W, H, n, wide[2:7], *win)
    codec.sync()
    assert np.array_equal(cg.planes(out), cref.counts(s.images, thr, *win)[0])
    wide[0:9:2] = cg.device(thr)
    out, _ = codec.project_counts(s.buf, s.lead, s.total, s.offs, W, H, n, wide[0:9:2], *win)
    codec.sync()
    assert np.array_equal(cg.planes(out), cref.counts(s.images, thr, *win)[0])


def test_python_threshold_forms_and_fraction(dv, codec, streams):
    """An int, a sequence of ints and a (K,) device tensor are the same scalars; fraction() is out / count."""
    import torch
    W, H = 100, 50
    s, _ = streams(W, H)
    win = (3, 5, 41, 27)
    a, _ = codec.project_counts(s.buf, s.lead, s.total, s.offs, W, H, s.n, [40, 200, 128], *win)
    b, _ = codec.project_counts(s.buf, s.lead, s.total, s.offs, W, H, s.n, cg.device(np.array([40, 200, 128], np.uint8)), *win)
    c, _ = codec.project_counts(s.buf, s.lead, s.total, s.offs, W, H, s.n, 200, *win)
    codec.sync()
    want, _ = cref.counts(s.images, np.array([40, 200, 128], np.uint8), *win)
    assert np.array_equal(cg.planes(a), want) and torch.equal(a.out, b.out) and torch.equal(c.out[0], a.out[1])
    f = a.fraction()
    assert f.dtype == torch.float64 and np.array_equal(f.cpu().numpy(), want.astype(np.float64) / s.n)
    for bad in (-1, 256, [3, 300], []):
        with pytest.raises(ValueError):
            codec.project_counts(s.buf, s.lead, s.total, s.offs, W, H, s.n, bad, *win)
    with pytest.raises(ValueError):
        codec.project_counts(s.buf, s.lead, s.total, s.offs, W, H, s.n, torch.zeros((2, 27, 40), dtype=torch.uint8, device="cuda"), *win)
    with pytest.raises(ValueError):
        codec.project_counts(s.buf, s.lead, s.total, s.offs, W, H, s.n, 5, *win, accumulate=True)   # nothing to continue


def test_argument_errors(dv, codec, streams):
    import torch
    W, H = 72, 40
    s, _ = streams(W, H)
    L, h = codec.L, codec.h
    thr = torch.zeros((9, H, W), dtype=torch.uint8, device="cuda")
    out = torch.zeros((9, H, W), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")

    def rc(n=13, x=0, y=0, rw=W, rh=H, tp=None, K=2, stride=W * H, acc=0, flags=1, op=None, cp=None):
        return L.dbde_hip_project_counts(h, s.buf.data_ptr() + s.lead, s.total, s.offs.data_ptr(), W, H, n, x, y, rw, rh,
                                         thr.data_ptr() if tp is None else tp, K, stride, acc, flags,
                                         out.data_ptr() if op is None else op, cnt.data_ptr() if cp is None else cp, None)
    assert rc() == dv.OK
    assert rc(flags=0, stride=0) == dv.OK                       # scalars: the stride is ignored
    assert rc(tp=thr.data_ptr() + 1) == dv.OK                   # U8 thresholds need no alignment
    for kw in (dict(K=0), dict(K=9), dict(stride=W * H - 1), dict(flags=2), dict(flags=3), dict(flags=-1),
               dict(op=out.data_ptr() + 2), dict(cp=cnt.data_ptr() + 4), dict(x=70, rw=8), dict(rh=0), dict(n=-1)):
        assert rc(**kw) == dv.ERR_ARG, kw
    for name in ("tp", "op", "cp"):
        args = [h, s.buf.data_ptr() + s.lead, s.total, s.offs.data_ptr(), W, H, 13, 0, 0, W, H, thr.data_ptr(), 2, W * H,
                0, 1, out.data_ptr(), cnt.data_ptr(), None]
        args[{"tp": 11, "op": 16, "cp": 17}[name]] = None
        assert L.dbde_hip_project_counts(*args) == dv.ERR_ARG, name
    codec.sync()
