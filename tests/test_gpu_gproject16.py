"""GPU: grouped temporal projections of DBDE16 streams -- dbde16_hip_project_groups (Codec.project_groups16).

Expected values are int64 reductions, group by group (tests/gproject_ref.py), over the DBDE16 oracle's decode and
dbde16_hip_decode_frames' decode of the same frames (every depth 0..16 occurs in the kinds), and over the numpy
decoder's images for crafted frames (wrapping U16 minima, rejected frames).  Sums are U32, sums of squares U64.
"""
import numpy as np
import pytest

from gproject_ref import group_ranges, reduce_groups
from test_gpu_gproject import ALL, GUARD, SENTINEL, assert_groups, ragged_starts, uniform_sizes, values
from test_gpu_project16 import Crafted16, encoded, windows16
from test_gpu_roi16 import KINDS, Batch16, images16
from test_oracle_u16 import o16   # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

SHAPES = [(200, 123, 13), (9, 9, 13), (8, 8, 13), (1921, 1081, 5), (4200, 24, 5)]


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


def groups16(codec, b, win, **kw):
    gp, res = codec.project_groups16(b.buf, b.lead, b.total, b.offs, b.W, b.H, b.n, *win, **kw)
    codec.sync()
    return gp, res


@pytest.mark.parametrize("W,H,n", SHAPES)
def test_uniform_and_ragged_groups_match_both_decodes(codec, o16, W, H, n):
    rng = np.random.default_rng(W * 7919 + H * 31 + n)
    forms = [dict(group_frames=g) for g in uniform_sizes(n)] + [dict(group_starts=s) for s in ragged_starts(n)]
    wins = windows16(W, H)
    for i, kind in enumerate(KINDS if W * H < 100000 else KINDS[:2]):
        b = Batch16(codec, o16, images16(rng, n, W, H, kind), first=3 + i, shift=i)
        for j, form in enumerate(forms):
            ranges = group_ranges(n, form.get("group_frames"), form.get("group_starts"))
            for win in {wins[0], wins[(i + j) % len(wins)]}:
                gp, res = groups16(codec, b, win, **form)
                assert_groups(gp, reduce_groups(b.full, ranges, *win, pix=2), what=f"{kind} {W}x{H} {form} {win} vs oracle")
                assert_groups(gp, reduce_groups(list(b.gpu_full), ranges, *win, pix=2), what=f"{kind} {form} {win} vs GPU")
                assert codec.parse_results(res) == [(2, b.first + f, 0, len(b.packed[f])) for f in range(n)]


def test_many_runs(dv, codec):
    """2,000 random 64x64 frames: several runs of groups."""
    import torch
    W, H, n = 64, 64, 2000
    g = torch.Generator(device="cuda").manual_seed(21)
    imgs = torch.randint(-32768, 32768, (n, H, W), dtype=torch.int16, device="cuda", generator=g)
    b = encoded(codec, imgs)
    host = list(imgs.cpu().numpy().view(np.uint16))
    assert dv.project_groups16_plan(W, H, n, group_frames=3)["runs"] > 1
    for form in (dict(group_frames=3), dict(group_frames=7), dict(group_starts=list(range(0, 2100, 5)))):
        ranges = group_ranges(n, form.get("group_frames"), form.get("group_starts"))
        for win in [(0, 0, W, H), (5, 9, 40, 33)]:
            gp, _ = groups16(codec, b, win, **form)
            assert_groups(gp, reduce_groups(host, ranges, *win, pix=2), what=f"runs {list(form)} {win}")


@pytest.mark.parametrize("W,H,n,how", [(64, 48, 30, "concat"), (200, 123, 23, "residues"), (8, 8, 70, "offsets")])
def test_crafted_and_rejected_frames(codec, W, H, n, how):
    import torch
    rng = np.random.default_rng(W * 7919 + H + 16)
    s = Crafted16(rng, W, H, n, how)
    bad = [f for f, im in enumerate(s.images) if im is None]
    assert bad and len(bad) < n
    _, want_res = codec.decode_frames16(s.buf, s.lead, s.total, s.offs, W, H, n)
    forms = [dict(group_frames=g) for g in (1, 3, 4, n)] + [dict(group_starts=[0, bad[0], bad[0] + 1, bad[0], n + 1])]
    for form in forms:
        ranges = group_ranges(n, form.get("group_frames"), form.get("group_starts"))
        for win in windows16(W, H)[:1] + windows16(W, H)[-1:]:
            gp, res = groups16(codec, s, win, **form)
            want = reduce_groups(s.images, ranges, *win, pix=2)
            assert_groups(gp, want, what=f"crafted {W}x{H} {form} {win}")
            assert torch.equal(res, want_res)
        if form.get("group_frames") == 1 or "group_starts" in form:
            assert 0 in want["counts"].tolist()


def test_each_group_equals_project16_of_its_frames(codec, o16):
    import torch
    W, H, n = 200, 123, 13
    b = Batch16(codec, o16, images16(np.random.default_rng(5), n, W, H, "full"))
    win = (5, 3, 131, 77)
    for form in (dict(group_frames=4), dict(group_starts=[0, 10, 5, 20, 2, 2])):
        gp, _ = groups16(codec, b, win, **form)
        for k, (lo, hi) in enumerate(group_ranges(n, form.get("group_frames"), form.get("group_starts"))):
            pr, _ = codec.project16(b.buf, b.lead, b.total, b.offs[lo:hi] if hi > lo else b.offs, W, H, hi - lo, *win)
            codec.sync()
            assert int(values(gp.counts)[k]) == int(pr.count.item())
            for s in ALL:
                assert torch.equal(values(getattr(gp, s)[k]), values(getattr(pr, s))), (form, k, s)


@pytest.mark.parametrize("stats", [("max",), ("min",), ("sum",), ("sumsq",), ("max", "min"), ALL])
def test_statistic_subsets_touch_only_their_buffers(dv, codec, o16, stats):
    """U16 planes at 2 mod 4 byte addresses; requested planes are written inside their extent only, the others never."""
    import torch
    W, H, n, g = 200, 123, 7, 3
    b = Batch16(codec, o16, images16(np.random.default_rng(17), n, W, H, "mixed"), shift=5)
    x, y, rw, rh = 5, 3, 131, 77
    ng = -(-n // g)
    P = ng * rw * rh
    size = {"max": 2, "min": 2, "sum": 4, "sumsq": 8}
    dt = {"max": torch.int16, "min": torch.int16, "sum": torch.int32, "sumsq": torch.int64}
    canv = {s: torch.full((2 * GUARD + 2 + size[s] * P,), SENTINEL, dtype=torch.uint8, device="cuda") for s in ALL}
    lo = {s: GUARD + (2 if size[s] == 2 else 0) for s in ALL}
    views = {s: canv[s][lo[s]: lo[s] + size[s] * P].view(dt[s]).view(ng, rh, rw) for s in ALL}
    counts = torch.full((ng + 2,), -7, dtype=torch.int32, device="cuda")
    out = dv.GroupProjection(*[views[s] if s in stats else None for s in ALL], counts=counts[1:ng + 1])
    gp, _ = groups16(codec, b, (x, y, rw, rh), group_frames=g, out=out)
    assert gp is out and counts[0].item() == -7 and counts[-1].item() == -7
    assert_groups(gp, reduce_groups(b.full, group_ranges(n, group_frames=g), x, y, rw, rh, pix=2), stats, what=str(stats))
    for s in ALL:
        c = canv[s].cpu().numpy()
        if s not in stats:
            assert (c == SENTINEL).all(), f"{s} was not requested but written"
        else:
            hi = lo[s] + size[s] * P
            assert (c[:lo[s]] == SENTINEL).all() and (c[hi:] == SENTINEL).all(), f"{s}: wrote outside its planes"


def test_accumulate_and_full_scale_sums(codec):
    """Full-scale frames: U32 sums and U64 sums of squares beyond 2^32; a second, accumulated batch adds."""
    import torch
    W, H, n = 40, 24, 6
    imgs = torch.full((n, H, W), -1, dtype=torch.int16, device="cuda")   # 65535
    imgs[:, 0::8, 0::8] = 0
    b = encoded(codec, imgs)
    host = list(imgs.cpu().numpy().view(np.uint16))
    starts = [0, 4, 4, n]
    ranges = group_ranges(n, starts=starts)
    gp, _ = groups16(codec, b, (0, 0, W, H), group_starts=starts)
    want = reduce_groups(host, ranges, 0, 0, W, H, pix=2)
    assert_groups(gp, want, what="first batch")
    assert int(want["sumsq"].max()) == 4 * 65535 ** 2 > 2 ** 32
    before = {s: getattr(gp, s)[1].clone() for s in ALL}
    groups16(codec, b, (0, 0, W, H), group_starts=starts, out=gp, accumulate=True)
    twice = dict(max=want["max"], min=want["min"], sum=2 * want["sum"], sumsq=2 * want["sumsq"],
                 counts=2 * want["counts"])
    assert_groups(gp, twice, what="accumulated")
    for s in ALL:
        assert torch.equal(getattr(gp, s)[1], before[s]), s   # the empty group's planes stay


def test_argument_errors(dv, codec):
    import torch
    W, H, n = 40, 24, 4
    b = encoded(codec, torch.zeros((n, H, W), dtype=torch.int16, device="cuda"))
    with pytest.raises(dv.DbdeError):   # U16 sums are DBDE only
        groups16(codec, b, (0, 0, W, H), group_frames=2, sum_dtype=torch.int16)
    raw = torch.full((1 << 14,), SENTINEL, dtype=torch.uint8, device="cuda")
    r, L, h, ptr = raw.data_ptr(), codec.L, codec.h, b.buf.data_ptr() + b.lead
    for mx, mn in [(r + 1, None), (None, r + 1)]:   # U16 planes not 2-byte aligned
        assert L.dbde16_hip_project_groups(h, ptr, b.total, b.offs.data_ptr(), W, H, n, 0, 0, 8, 8, 2, None, 2, 0, 0,
                                           mx, mn, None, None, r + 1024, None) == dv.ERR_ARG
    codec.sync()
    assert (raw.cpu().numpy() == SENTINEL).all()
