"""GPU: neighbour-product projections -- dbde_hip_project_pairs (Codec.project_pairs).

Every plane is compared for equality with tests/pairs_ref.py -- integer products of shifted windows summed over the
accepted frames in numpy -- on the images dbde_hip_decode_frames writes for encoded batches.  Nothing expected comes
from the call itself.  Wherever the window is at least 3 x 3, pairs_gpu.distinct holds on the expected planes of all
four offsets: pairwise different, none zero, none equal to the sum of squares.
"""
import numpy as np
import pytest

import far
import pairs_gpu as pg
import pairs_ref as pref
import wproject_gpu as wg
from test_gpu_project import Batch

pytestmark = pytest.mark.gpu

# edge tiles both ways, several waves of tiles and several tile rows (72x40, 100x50); three overlapping pieces and one
# seam between tile rows (520x16); a tile row of two index chunks, so that the row below starts two chunks on (4104x16)
SHAPES = [(72, 40), (100, 50), (520, 16)]
WIDE = (4104, 16)
COUNTS = (1, 3, 4, 5, 13)       # the four-frame pipeline step's boundaries and tails
NMAX = 13


def windows(W, H):
    """The full frame, an unaligned window, one pixel, the one-pixel-wide and one-pixel-high strips, a 2 x 2 window
    whose four offsets all cross a tile corner; on the wide frame a 2 x 2 window across the corner at pixel 256 and a
    window across it."""
    out = [(0, 0, W, H), (3, 5, 41, min(27, H - 5)), (W // 2 + 1, H - 2, 1, 1), (9, 2, 1, H - 3), (2, 9, W - 5, 1),
           (7, 7, 2, 2)]
    if W > 256:
        out += [(255, 7, 2, 2), (251, 1, 13, H - 2)]
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
def test_every_mask_and_window_matches_the_reference(dv, codec, streams, W, H, n):
    import torch
    full, b = streams(W, H)
    s = full.first(n)
    for win in windows(W, H):
        for mask in pg.MASKS:
            out, res = pg.check(codec.project_pairs, s, mask, win, what="mixed")
            assert torch.equal(res, b.results[:n])
            x, y, rw, rh = win
            got = pg.planes(out)
            # edge elements hold 0: every plane of the one-pixel window, all but DOWN of the one-pixel-wide strip and
            # all but RIGHT of the one-pixel-high one (has_partner: tests/test_pairs_ref.py)
            assert not got[~pref.has_partner(mask, rw, rh)].any()
    p = dv.pairs_plan(W, H, n)
    assert p["segments"] == 1 and p["rows_below"] == (H + 7) // 8 - 1
    assert p["pieces_x"] == (3 if W > 256 else 1)


def test_tile_rows_in_different_index_chunks(dv, codec, streams):
    """4104 x 16: 513 tiles across, so a tile row is two index chunks and the row below a piece starts two chunks on.
    Pieces 17 and 18 (of 18) lie around tile 512, where the second chunk of each row begins."""
    W, H = WIDE
    n = 3
    p = dv.pairs_plan(W, H, n)
    assert p["chunk_pieces"] == 2 and p["chunks_per_frame"] == 4 and p["chunk_tiles"] == 512
    assert p["pieces_x"] == 1 + -(-(513 - 32) // 30) and p["rows_below"] == 1
    assert dv.roi_plan(W, H, n, 0, 0, W, H)["chunks_per_frame"] == 4
    s, _ = streams(W, H, n)
    for win in [(0, 0, W, H), (4090, 3, 14, 12)]:
        for mask in (15, 3, 1):
            pg.check(codec.project_pairs, s, mask, win, what="two chunks per tile row")
    # 100 x 50: every tile row is a chunk of its own
    q = dv.pairs_plan(100, 50, n)
    assert q["chunk_tiles"] == 13 and q["chunks_per_frame"] == 7


@pytest.mark.parametrize("mode", ["noise8", "smooth"])
def test_other_frame_contents(codec, streams, mode):
    for W, H in SHAPES:
        s, _ = streams(W, H, 5, mode)
        for win in windows(W, H)[:2]:
            for mask in (15, 10, 3, 1):
                pg.check(codec.project_pairs, s, mask, win, what=mode)


def test_flat_frames(codec, streams):
    """Every pixel of every frame holds one value v: every element with a partner equals n * v^2."""
    W, H, n = 100, 50, 5
    s, _ = streams(W, H, n, "flat")
    v = int(s.images[0][0, 0])
    assert all((im == v).all() for im in s.images) and v > 0
    for win in windows(W, H)[:2]:
        out, _ = pg.check(codec.project_pairs, s, 15, win, what="flat", cap=False)
        got = pg.planes(out)
        has = pref.has_partner(15, win[2], win[3])
        assert (got[has] == n * v * v).all() and (got[~has] == 0).all()


@pytest.mark.parametrize("cut", [1, 4, 6])
def test_accumulate_split_equals_one_call(codec, streams, cut):
    """n = a + b over two calls equals one call bit for bit, the edge elements (which the second call must leave alone:
    they are planted with a sentinel in a third run) and the count included; n == 0 adds nothing, or zeroes."""
    import torch
    W, H, n = 100, 50, 13
    full, _ = streams(W, H)
    for win in ((3, 5, 41, 27), (0, 0, W, H)):
        x, y, rw, rh = win
        for mask in (15, 10, 2):
            offs = pref.offsets_of(mask)
            one, _ = pg.check(codec.project_pairs, full, mask, win, what="one call")
            out, _ = pg.check(codec.project_pairs, full.first(cut), mask, win, what="first part")
            codec.project_pairs(full.buf, full.lead, full.total, full.offs[cut:], W, H, n - cut, offs, *win, out=out,
                                accumulate=True)
            codec.sync()
            assert torch.equal(out.out, one.out) and int(out.count.item()) == n
            codec.project_pairs(full.buf, full.lead, full.total, full.offs, W, H, 0, offs, *win, out=out, accumulate=True)
            codec.sync()
            assert torch.equal(out.out, one.out) and int(out.count.item()) == n
            # an accumulating call leaves the elements without a partner as they are
            edge = torch.from_numpy(~pref.has_partner(mask, rw, rh)).cuda()
            out.out[edge] = -77
            codec.project_pairs(full.buf, full.lead, full.total, full.offs, W, H, cut, offs, *win, out=out, accumulate=True)
            codec.sync()
            assert (out.out[edge] == -77).all() and int(out.count.item()) == n + cut
            want = pg.planes(one) + pref.pairs(full.images[:cut], mask, *win)[0]
            assert np.array_equal(pg.planes(out)[~edge.cpu().numpy()], want[~edge.cpu().numpy()])
            codec.project_pairs(full.buf, full.lead, full.total, full.offs, W, H, 0, offs, *win, out=out)
            codec.sync()
            assert (out.out == 0).all() and int(out.count.item()) == 0


def test_rejected_frames_add_nothing(codec):
    """Crafted frames with broken ones among them: the planes are those of the accepted frames and the results are
    project's on the same stream."""
    import torch
    rng = np.random.default_rng(77)
    W, H, n = 100, 50, 13
    s = wg.crafted_stream(rng, W, H, n, 8, bad=(1, 4, 5, 12))
    assert sum(im is None for im in s.images) == 4
    _, want_res = codec.project(s.buf, s.lead, s.total, s.offs, W, H, n, stats=("sum",))
    for win in windows(W, H)[:2]:
        for mask in (15, 3):
            out, res = pg.check(codec.project_pairs, s, mask, win, what="rejected frames", cap=False)
            assert torch.equal(res, want_res) and int(out.count.item()) == 9


@pytest.mark.parametrize("n", [50, 70])
def test_segments(dv, codec, cus, streams, n):
    """A window of few workgroups and n >= 33 frames: the plan cuts S > 1 segments on this device (asserted, not
    assumed).  The result is the reference (which has no segments) and equals two accumulating calls."""
    import torch
    W, H = 72, 40
    s, _ = streams(W, H, 70)
    s = s.first(n)
    for win in [(0, 0, W, H), (3, 5, 41, 27)]:
        for mask in (15, 10, 1):
            p = dv.pairs_plan(W, H, n, *win, pairs=mask, n_cu=cus)
            assert p["segments"] > 1 and p["workspace_bytes"] == -(-4 * p["segments"] * p["planes"] * win[2] * win[3] // 16) * 16
            out, _ = pg.check(codec.project_pairs, s, mask, win, what="segments")
            cut = 37
            assert dv.pairs_plan(W, H, cut, *win, pairs=mask, n_cu=cus)["segments"] > 1
            offs = pref.offsets_of(mask)
            two, _ = codec.project_pairs(s.buf, s.lead, s.total, s.offs, W, H, cut, offs, *win)
            codec.project_pairs(s.buf, s.lead, s.total, s.offs[cut:], W, H, n - cut, offs, *win, out=two, accumulate=True)
            codec.sync()
            assert torch.equal(two.out, out.out) and int(two.count.item()) == n


def test_sums_beyond_u32(dv, codec, cus):
    """66,052 frames of 8 x 16, all 255: more than a segment may hold (65,536), and the smallest count whose sum
    n * 65,025 = 4,294,981,300 exceeds 2^32 = 4,294,967,296 (65,537 frames give 4,261,543,425, still below it), through
    U32 partials of several segments and the combine.  On a device of many compute units the plan cuts far more than
    the two segments the bound asks for, so no partial comes near 2^32 here: tests/test_gpu_bounds.py fills the
    per-lane accumulators to the header's bound (65,536 frames in one segment, 65,536 * 255^2 < 2^32)."""
    import torch
    n, W, H = 66052, 8, 16
    assert (n - 1) * 65025 < 2 ** 32 < n * 65025
    p = dv.pairs_plan(W, H, n, n_cu=cus)
    assert p["segments"] >= 2 and p["frames_per_segment"] <= p["max_frames_per_segment"] == 65536
    assert dv.pairs_plan(W, H, n, n_cu=1)["segments"] == 2
    imgs = torch.full((n, H, W), 255, dtype=torch.uint8, device="cuda")
    b = Batch(codec, None, W, H, n, images=imgs)
    out, _ = codec.project_pairs(b.buf, b.lead, b.total, b.offs, W, H, n, 8)
    codec.sync()
    has = pref.has_partner(15, W, H)
    got = pg.planes(out)
    assert n * 65025 > 2 ** 32 and (got[has] == n * 65025).all() and (got[~has] == 0).all()
    assert int(out.count.item()) == n


def test_guarded_outputs(dv, codec, streams):
    """The planes sit in a far.guarded canvas (one and several segments) and the guards stay intact; the count sits
    between two sentinels."""
    import torch
    W, H = 72, 40
    full, _ = streams(W, H, 70)
    win = (3, 5, 41, 27)
    for n in (13, 70):
        s = full.first(n)
        for mask in (15, 2):
            want, _ = pref.pairs(s.images, mask, *win)
            g = far.guarded((len(want), win[3], win[2]), torch.int64)
            count = torch.full((3,), -7, dtype=torch.int64, device="cuda")
            out = dv.PairProjection(g.t, count[1:2], pref.offsets_of(mask))
            got, _ = codec.project_pairs(s.buf, s.lead, s.total, s.offs, W, H, n, pref.offsets_of(mask), *win, out=out)
            codec.sync()
            assert got is out
            g.check(f"n = {n}, mask = {mask}")
            assert np.array_equal(pg.planes(out), want) and count.tolist() == [-7, n, -7]
            del g
    far.free()


def test_python_pairs_forms(dv, codec, streams):
    """4 and 8 are the neighbourhoods, other ints masks, iterables offsets; the argument errors."""
    import torch
    W, H = 100, 50
    s, _ = streams(W, H)
    win = (3, 5, 41, 27)
    args = (s.buf, s.lead, s.total, s.offs, W, H, s.n)
    a, _ = codec.project_pairs(*args, 8, *win)
    b, _ = codec.project_pairs(*args, 15, *win)
    c, _ = codec.project_pairs(*args, 4, *win)
    d, _ = codec.project_pairs(*args, [(1, 0), (0, 1)], *win)
    e, _ = codec.project_pairs(*args, x=win[0], y=win[1], rw=win[2], rh=win[3])
    f, _ = codec.project_pairs(*args, [(-1, 1), (1, 1)], *win)      # plane order is bit order, not the argument's
    codec.sync()
    assert a.offsets == ((1, 0), (0, 1), (1, 1), (-1, 1)) and c.offsets == ((1, 0), (0, 1)) and f.offsets == ((1, 1), (-1, 1))
    assert a.mask == 15 and c.mask == 3 and f.mask == 12
    assert np.array_equal(pg.planes(a), pref.pairs(s.images, 15, *win)[0])
    assert torch.equal(a.out, b.out) and torch.equal(a.out, e.out) and torch.equal(c.out, d.out)
    assert torch.equal(c.out, a.out[:2]) and torch.equal(f.out, a.out[2:])
    for bad in (0, 16, -1, [(2, 0)], [(0, -1)], [], "8"):
        with pytest.raises(ValueError):
            codec.project_pairs(*args, bad, *win)
    with pytest.raises(ValueError):
        codec.project_pairs(*args, 8, *win, accumulate=True)                      # nothing to continue
    with pytest.raises(ValueError):
        codec.project_pairs(*args, 4, *win, out=a)                                # other offsets than out holds
    with pytest.raises(ValueError):
        codec.project_pairs(*args, 8, 0, 0, W, H, out=a)                          # another window
    with pytest.raises(ValueError):
        codec.project_pairs(*args, 8, *win, out=dv.PairProjection(a.out.to(torch.int32), a.count, a.offsets))
    e = dv.PairProjection.empty(4, 5, 6, "cuda")
    assert tuple(e.out.shape) == (2, 5, 6) and e.out.dtype == torch.int64 and int(e.count.item()) == 0


def test_argument_errors(dv, codec, streams):
    import torch
    W, H = 72, 40
    s, _ = streams(W, H)
    L, h = codec.L, codec.h
    out = torch.zeros((4, H, W), dtype=torch.int64, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")

    def rc(n=13, x=0, y=0, rw=W, rh=H, pairs=15, acc=0, op=None, cp=None):
        return L.dbde_hip_project_pairs(h, s.buf.data_ptr() + s.lead, s.total, s.offs.data_ptr(), W, H, n, x, y, rw, rh,
                                        pairs, acc, out.data_ptr() if op is None else op,
                                        cnt.data_ptr() if cp is None else cp, None)
    assert rc() == dv.OK
    for kw in (dict(pairs=0), dict(pairs=16), dict(pairs=-1), dict(op=out.data_ptr() + 4), dict(cp=cnt.data_ptr() + 4),
               dict(x=70, rw=8), dict(rh=0), dict(n=-1)):
        assert rc(**kw) == dv.ERR_ARG, kw
    for at in (1, 3, 13, 14):     # the stream, the offsets, d_out, d_count
        args = [h, s.buf.data_ptr() + s.lead, s.total, s.offs.data_ptr(), W, H, 13, 0, 0, W, H, 15, 0, out.data_ptr(),
                cnt.data_ptr(), None]
        args[at] = None
        assert L.dbde_hip_project_pairs(*args) == dv.ERR_ARG, at
    codec.sync()
