"""GPU: neighbour-product projections of DBDE16 streams -- dbde16_hip_project_pairs (Codec.project_pairs16).

test_gpu_pairs.py's checks with U16 pixels (values at and above 32,768 among them): every plane equal to
tests/pairs_ref.py over the DBDE16 oracle's decode of encoded batches (Batch16 holds it equal to
dbde16_hip_decode_frames').
"""
import numpy as np
import pytest

import pairs_gpu as pg
import pairs_ref as pref
import wproject_gpu as wg
from test_gpu_roi16 import Batch16, images16
from test_oracle_u16 import o16   # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

# edge tiles both ways and several tile rows; 264 x 16: 33 tiles, three overlapping pieces of 16, one seam
SHAPES = [(72, 40), (100, 50), (264, 16)]
COUNTS = (1, 3, 4, 5, 13)
NMAX = 13


def windows(W, H):
    out = [(0, 0, W, H), (3, 5, 41, min(27, H - 5)), (W // 2 + 1, H - 2, 1, 1), (9, 2, 1, H - 3), (2, 9, W - 5, 1),
           (7, 7, 2, 2)]
    if W > 128:
        out += [(127, 7, 2, 2), (123, 1, 13, H - 2)]      # across the corner at pixel 128, where a piece of 16 tiles ends
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
def test_every_mask_and_window_matches_the_reference(dv, codec, streams, W, H, n):
    s = streams(W, H).first(n)
    assert max(int(im.max()) for im in s.images) >= 32768
    for win in windows(W, H):
        for mask in pg.MASKS:
            out, res = pg.check(codec.project_pairs16, s, mask, win, what="mixed16")
            assert [r[1] for r in codec.parse_results(res)] == list(range(n))
            assert not pg.planes(out)[~pref.has_partner(mask, win[2], win[3])].any()
    p = dv.pairs16_plan(W, H, n)
    assert p["segments"] == 1 and p["rows_below"] == (H + 7) // 8 - 1
    assert p["pieces_x"] == (3 if W > 128 else 1)


@pytest.mark.parametrize("kind", ["full", "small", "depth16"])
def test_other_frame_contents(codec, streams, kind):
    """Noise over the whole range, smooth 8-bit content in 16-bit pixels, and tiles of depth 16."""
    for W, H in SHAPES[1:]:
        s = streams(W, H, 5, kind)
        for win in windows(W, H)[:2]:
            for mask in (15, 10, 3, 1):
                pg.check(codec.project_pairs16, s, mask, win, what=kind)


def test_two_frames_of_65535_need_u64_sums(codec, o16):   # noqa: F811
    """Every element with a partner is 2 * 65,535^2 = 8,589,672,450 > 2^32: the U64 accumulators."""
    W, H, n = 100, 50, 2
    s = stream_of(codec, o16, np.full((n, H, W), 65535, np.uint16))
    for win in windows(W, H)[:2]:
        out, _ = pg.check(codec.project_pairs16, s, 15, win, what="65535", cap=False)
        has = pref.has_partner(15, win[2], win[3])
        got = pg.planes(out)
        assert 2 * 65535 ** 2 > 2 ** 32 and (got[has] == 2 * 65535 ** 2).all() and (got[~has] == 0).all()


def test_flat_frames(codec, o16):   # noqa: F811
    W, H, n, v = 100, 50, 5, 0x9234
    s = stream_of(codec, o16, np.full((n, H, W), v, np.uint16))
    for win in windows(W, H)[:2]:
        out, _ = pg.check(codec.project_pairs16, s, 15, win, what="flat", cap=False)
        has = pref.has_partner(15, win[2], win[3])
        assert (pg.planes(out)[has] == n * v * v).all()


@pytest.mark.parametrize("cut", [1, 4, 6])
def test_accumulate_split_equals_one_call(codec, streams, cut):
    import torch
    W, H, n = 100, 50, 13
    full = streams(W, H)
    for win in ((3, 5, 41, 27), (0, 0, W, H)):
        x, y, rw, rh = win
        for mask in (15, 10, 2):
            offs = pref.offsets_of(mask)
            one, _ = pg.check(codec.project_pairs16, full, mask, win, what="one call")
            out, _ = pg.check(codec.project_pairs16, full.first(cut), mask, win, what="first part")
            edge = torch.from_numpy(~pref.has_partner(mask, rw, rh)).cuda()
            out.out[edge] = -77        # an accumulating call leaves the elements without a partner as they are
            codec.project_pairs16(full.buf, full.lead, full.total, full.offs[cut:], W, H, n - cut, offs, *win, out=out,
                                  accumulate=True)
            codec.sync()
            assert (out.out[edge] == -77).all() and int(out.count.item()) == n
            assert torch.equal(out.out[~edge], one.out[~edge])
            codec.project_pairs16(full.buf, full.lead, full.total, full.offs, W, H, 0, offs, *win, out=out, accumulate=True)
            codec.sync()
            assert torch.equal(out.out[~edge], one.out[~edge]) and int(out.count.item()) == n
            codec.project_pairs16(full.buf, full.lead, full.total, full.offs, W, H, 0, offs, *win, out=out)
            codec.sync()
            assert (out.out == 0).all() and int(out.count.item()) == 0


def test_rejected_frames_add_nothing(codec):
    import torch
    rng = np.random.default_rng(78)
    W, H, n = 100, 50, 13
    s = wg.crafted_stream(rng, W, H, n, 16, bad=(0, 4, 5, 11))
    _, want_res = codec.project16(s.buf, s.lead, s.total, s.offs, W, H, n, stats=("sum",))
    for win in windows(W, H)[:2]:
        for mask in (15, 3):
            out, res = pg.check(codec.project_pairs16, s, mask, win, what="rejected frames", cap=False)
            assert torch.equal(res, want_res) and int(out.count.item()) == 9


@pytest.mark.parametrize("n", [50, 70])
def test_segments(dv, codec, cus, streams, n):
    """S > 1 segments on this device (asserted): U64 partials and the combine equal the reference and two calls."""
    import torch
    W, H = 72, 40
    s = streams(W, H, 70).first(n)
    for win in [(0, 0, W, H), (3, 5, 41, 27)]:
        for mask in (15, 10, 1):
            p = dv.pairs16_plan(W, H, n, *win, pairs=mask, n_cu=cus)
            assert p["segments"] > 1 and p["workspace_bytes"] == -(-8 * p["segments"] * p["planes"] * win[2] * win[3] // 16) * 16
            out, _ = pg.check(codec.project_pairs16, s, mask, win, what="segments")
            cut = 37
            offs = pref.offsets_of(mask)
            two, _ = codec.project_pairs16(s.buf, s.lead, s.total, s.offs, W, H, cut, offs, *win)
            codec.project_pairs16(s.buf, s.lead, s.total, s.offs[cut:], W, H, n - cut, offs, *win, out=two, accumulate=True)
            codec.sync()
            assert torch.equal(two.out, out.out) and int(two.count.item()) == n


def test_argument_errors(dv, codec, streams):
    import torch
    W, H = 72, 40
    s = streams(W, H)
    L, h = codec.L, codec.h
    out = torch.zeros((4, H, W), dtype=torch.int64, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")

    def rc(n=13, x=0, y=0, rw=W, rh=H, pairs=15, acc=0, op=None, cp=None):
        return L.dbde16_hip_project_pairs(h, s.buf.data_ptr() + s.lead, s.total, s.offs.data_ptr(), W, H, n, x, y, rw,
                                          rh, pairs, acc, out.data_ptr() if op is None else op,
                                          cnt.data_ptr() if cp is None else cp, None)
    assert rc() == dv.OK
    for kw in (dict(pairs=0), dict(pairs=16), dict(op=out.data_ptr() + 4), dict(cp=cnt.data_ptr() + 2),
               dict(x=70, rw=8), dict(rh=0), dict(n=-1), dict(op=0), dict(cp=0)):
        assert rc(**kw) == dv.ERR_ARG, kw
    with pytest.raises(ValueError):
        codec.project_pairs16(s.buf, s.lead, s.total, s.offs, W, H, 13, 16)
    codec.sync()
