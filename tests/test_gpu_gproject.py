"""GPU: grouped temporal projections -- dbde_hip_project_groups (Codec.project_groups).

Expected values are int64 reductions, group by group (tests/gproject_ref.py's rule), over the images
dbde_hip_decode_frames writes for the same frames, or over the numpy decoder's images of tests/crafted.py for crafted
frames (wrapping minima, rejected frames).  They never come from the call itself; one test also checks the defining
property against Codec.project called once per group.
"""
import numpy as np
import pytest

from gproject_ref import group_ranges, reduce_groups
from test_gpu_project import Batch, Crafted, reduce_images, windows

pytestmark = pytest.mark.gpu

MODES = ("noise8", "mixed", "flat", "smooth")
ALL = ("max", "min", "sum", "sumsq")
GUARD = 40
SENTINEL = 0x5A
SHAPES = [(200, 123, 13), (9, 9, 13), (8, 8, 13), (1921, 1081, 5), (4200, 24, 5), (64, 64, 2000)]


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


def uniform_sizes(n):
    return [1, 2, 3, 4, 5, 7, n, n + 3]


def ragged_starts(n):
    rng = np.random.default_rng(n)
    trials = rng.permutation(max(n - 3, 1))[:6]   # stimulus-triggered: 3-frame epochs at permuted offsets
    return [[0, n], [0, 0, 5, 5, n], [3, 9], [0, 10, 5, n + 7],
            [int(v) for t in trials for v in (t, t + 3)]]


def values(t):
    """A plane as int64 on its device: int16 / int32 tensors hold U16 / U32 bits."""
    import torch
    bits = {torch.int16: 0xFFFF, torch.int32: 0xFFFFFFFF}.get(t.dtype)
    return t.to(torch.int64) & bits if bits else t.to(torch.int64)


def expect_groups(images, ranges, x, y, rw, rh):
    """Per-group reductions (torch, on the images' device) -> stacked planes and counts."""
    import torch
    per = [reduce_images(images[b:e], x, y, rw, rh) for b, e in ranges]
    out = {s: torch.stack([p[s] for p in per]) for s in ALL}
    out["counts"] = [p["count"] for p in per]
    return out


def assert_groups(gp, want, stats=ALL, what=""):
    import torch
    assert values(gp.counts).cpu().tolist() == [int(c) for c in want["counts"]], (what, "counts")
    for s in ALL:
        got = getattr(gp, s)
        if s not in stats:
            assert got is None, (what, s)
            continue
        exp = want[s]
        exp = exp if isinstance(exp, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(exp))
        g = values(got)
        exp = exp.to(g.device).to(torch.int64)
        assert g.shape == exp.shape, (what, s, g.shape, exp.shape)
        if not torch.equal(g, exp):
            bad = (g != exp).nonzero()[0].tolist()
            raise AssertionError(f"{what}: {s} differs at {bad}: {int(g[tuple(bad)])} != {int(exp[tuple(bad)])}")


def groups(codec, b, win, **kw):
    gp, res = codec.project_groups(b.buf, b.lead, b.total, b.offs, b.W, b.H, b.n, *win, **kw)
    codec.sync()
    return gp, res


@pytest.fixture(scope="module")
def batches(codec):
    cache = {}

    def get(mode, W, H, n):
        if (mode, W, H, n) not in cache:
            cache[(mode, W, H, n)] = Batch(codec, mode, W, H, n)
        return cache[(mode, W, H, n)]
    return get


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W,H,n", SHAPES)
def test_uniform_groups_match_decoded_images(dv, codec, batches, mode, W, H, n):
    """Every boundary position relative to the four-frame pipeline step, a ragged last group, one group (g = n, n + 3);
    64x64 x 2,000 frames has several runs."""
    import torch
    b = batches(mode, W, H, n)
    wins = windows(W, H)
    if n == 2000:
        assert dv.project_groups_plan(W, H, n, group_frames=3)["runs"] > 1
    for i, g in enumerate(uniform_sizes(n)):
        for win in {wins[0], wins[(i + 1) % len(wins)], wins[-1]}:
            gp, res = groups(codec, b, win, group_frames=g)
            assert_groups(gp, expect_groups(b.images, group_ranges(n, group_frames=g), *win),
                          what=f"{mode} {W}x{H} g={g} {win}")
            assert torch.equal(res, b.results)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("W,H,n", SHAPES[:5])
def test_ragged_groups_match_decoded_images(codec, batches, mode, W, H, n):
    import torch
    b = batches(mode, W, H, n)
    wins = windows(W, H)
    for i, starts in enumerate(ragged_starts(n)):
        for win in {wins[0], wins[(i + 2) % len(wins)]}:
            gp, res = groups(codec, b, win, group_starts=starts)
            assert_groups(gp, expect_groups(b.images, group_ranges(n, starts=starts), *win),
                          what=f"{mode} {W}x{H} starts={starts} {win}")
            assert torch.equal(res, b.results)


def test_ragged_groups_over_many_runs(dv, codec, batches):
    """2,000 frames of 64x64 in ragged groups of 0..6 frames: several runs, boundaries anywhere in a pipeline step."""
    W, H, n = 64, 64, 2000
    b = batches("mixed", W, H, n)
    rng = np.random.default_rng(3)
    starts = np.concatenate([[0], np.cumsum(rng.integers(0, 7, 700))]).tolist()
    assert dv.project_groups_plan(W, H, n, has_group_starts=True, n_groups=len(starts) - 1)["runs"] > 1
    for win in [(0, 0, W, H), (5, 9, 40, 33)]:
        gp, _ = groups(codec, b, win, group_starts=starts)
        assert_groups(gp, expect_groups(b.images, group_ranges(n, starts=starts), *win), what=f"ragged runs {win}")


def test_starts_as_a_device_tensor_with_values_above_2_31(codec, batches):
    import torch
    W, H, n = 200, 123, 13
    b = batches("mixed", W, H, n)
    starts = [2, 6, 0xFFFFFFFF, 1, 0x80000000]
    dev = torch.as_tensor(np.array(starts, np.uint32).view(np.int32), device="cuda")
    gp, _ = groups(codec, b, (0, 0, W, H), group_starts=dev)
    assert_groups(gp, expect_groups(b.images, group_ranges(n, starts=starts), 0, 0, W, H), what="U32 starts")


@pytest.mark.parametrize("W,H,n,how", [(64, 48, 40, "concat"), (200, 123, 23, "residues"), (8, 8, 70, "offsets")])
def test_crafted_and_rejected_frames(codec, W, H, n, how):
    """Crafted streams (wrapping minima) with every third frame rejected: groups partly rejected, and -- at g = 1 and in
    the ragged list -- wholly rejected (the empty projection, count 0).  d_results equals decode_frames'."""
    import torch
    rng = np.random.default_rng(W * 7919 + H)
    s = Crafted(rng, W, H, n, how)
    bad = [f for f, im in enumerate(s.images) if im is None]
    assert bad and len(bad) < n
    _, want_res = codec.decode_frames(s.buf, s.lead, s.total, s.offs, W, H, n)
    forms = [dict(group_frames=g) for g in (1, 3, 4, n)] + [dict(group_starts=[0, bad[0], bad[0] + 1, bad[0], n + 1])]
    for form in forms:
        ranges = group_ranges(n, form.get("group_frames"), form.get("group_starts"))
        for win in windows(W, H)[:1] + windows(W, H)[-1:]:
            gp, res = groups(codec, s, win, **form)
            want = reduce_groups(s.images, ranges, *win)
            assert_groups(gp, want, what=f"crafted {W}x{H} {form} {win}")
            assert torch.equal(res, want_res)
        if form.get("group_frames") == 1 or "group_starts" in form:
            assert 0 in want["counts"].tolist()
        if form.get("group_frames") in (3, 4):
            assert any(0 < c < e - b for c, (b, e) in zip(want["counts"].tolist(), ranges))


@pytest.mark.parametrize("form", [dict(group_frames=4), dict(group_frames=5), dict(group_starts=[0, 10, 5, 20, 2, 2])])
def test_each_group_equals_project_of_its_frames(codec, batches, form):
    """The defining property: group k's planes and count are bit-equal to Codec.project over frames [b, e) alone."""
    import torch
    W, H, n = 200, 123, 13
    b = batches("noise8", W, H, n)
    win = (5, 3, 131, 77)
    gp, _ = groups(codec, b, win, **form)
    for k, (lo, hi) in enumerate(group_ranges(n, form.get("group_frames"), form.get("group_starts"))):
        pr, _ = codec.project(b.buf, b.lead, b.total, b.offs[lo:hi] if hi > lo else b.offs, W, H, hi - lo, *win)
        codec.sync()
        assert int(values(gp.counts)[k]) == int(pr.count.item())
        for s in ALL:
            assert torch.equal(values(getattr(gp, s)[k]), getattr(pr, s).to(torch.int64)), (form, k, s)


@pytest.mark.parametrize("stats", [("max",), ("min",), ("sum",), ("sumsq",), ("max", "min"), ALL])
@pytest.mark.parametrize("odd", [0, 1, 3])
def test_statistic_subsets_touch_only_their_buffers(dv, codec, batches, stats, odd):
    """Every plane set and d_counts sit in guard canvases; the requested ones are written inside their extent only, the
    others are never touched.  U8 planes at odd byte offsets."""
    import torch
    W, H, n, g = 200, 123, 13, 3
    b = batches("mixed", W, H, n)
    x, y, rw, rh = 5, 3, 131, 77
    ng = -(-n // g)
    P = ng * rw * rh
    size = {"max": 1, "min": 1, "sum": 4, "sumsq": 8}
    dt = {"max": torch.uint8, "min": torch.uint8, "sum": torch.int32, "sumsq": torch.int64}
    canv = {s: torch.full((2 * GUARD + odd + size[s] * P,), SENTINEL, dtype=torch.uint8, device="cuda") for s in ALL}
    lo = {s: GUARD + (odd if size[s] == 1 else 0) for s in ALL}
    views = {s: canv[s][lo[s]: lo[s] + size[s] * P].view(dt[s]).view(ng, rh, rw) for s in ALL}
    counts = torch.full((ng + 2,), -7, dtype=torch.int32, device="cuda")
    out = dv.GroupProjection(*[views[s] if s in stats else None for s in ALL], counts=counts[1:ng + 1])
    gp, _ = groups(codec, b, (x, y, rw, rh), group_frames=g, out=out)
    assert gp is out
    assert counts[0].item() == -7 and counts[-1].item() == -7
    assert_groups(gp, expect_groups(b.images, group_ranges(n, group_frames=g), x, y, rw, rh), stats, what=str(stats))
    for s in ALL:
        c = canv[s].cpu().numpy()
        if s not in stats:
            assert (c == SENTINEL).all(), f"{s} was not requested but written"
        else:
            hi = lo[s] + size[s] * P
            assert (c[:lo[s]] == SENTINEL).all() and (c[hi:] == SENTINEL).all(), f"{s}: wrote outside its planes"


def test_u16_sums(dv, codec, batches):
    import torch
    W, H, n = 8, 8, 257
    imgs = torch.full((n, H, W), 255, dtype=torch.uint8, device="cuda")
    b = Batch(codec, None, W, H, n, images=imgs)
    gp, _ = groups(codec, b, (0, 0, W, H), group_frames=257, stats=("sum",), sum_dtype=torch.int16)
    assert gp.sum.dtype == torch.int16 and (values(gp.sum) == 65535).all() and values(gp.counts).tolist() == [257]
    b2 = Batch(codec, None, W, H, 258, images=torch.full((258, H, W), 255, dtype=torch.uint8, device="cuda"))
    with pytest.raises(dv.DbdeError):
        groups(codec, b2, (0, 0, W, H), group_frames=258, stats=("sum",), sum_dtype=torch.int16)
    with pytest.raises(dv.DbdeError):   # ragged with more than 257 frames
        groups(codec, b2, (0, 0, W, H), group_starts=[0, 2], stats=("sum",), sum_dtype=torch.int16)
    m = batches("mixed", 200, 123, 13)
    for form in (dict(group_frames=3), dict(group_starts=[0, 10, 5, 20])):
        a, _ = groups(codec, m, (3, 5, 190, 110), sum_dtype=torch.int16, **form)
        c, _ = groups(codec, m, (3, 5, 190, 110), sum_dtype=torch.int32, **form)
        assert a.sum.dtype == torch.int16 and c.sum.dtype == torch.int32
        assert torch.equal(values(a.sum), values(c.sum))
        for s in ("max", "min", "sumsq", "counts"):
            assert torch.equal(getattr(a, s), getattr(c, s)), s
        ranges = group_ranges(13, form.get("group_frames"), form.get("group_starts"))
        assert_groups(a, expect_groups(m.images, ranges, 3, 5, 190, 110), what=f"U16 sums {form}")
    with pytest.raises(dv.DbdeError):   # a U16 sum cannot accumulate
        groups(codec, m, (3, 5, 190, 110), group_frames=3, out=a, accumulate=True)


def test_accumulate_two_batches(codec, batches):
    """Two batches with the same groups, the second accumulated: the reductions over both; counts add; the planes of an
    empty group stay as they were."""
    import torch
    W, H, n = 200, 123, 13
    b1, b2 = batches("mixed", W, H, n), batches("noise8", W, H, n)
    win = (3, 5, 190, 110)
    for form in (dict(group_frames=4), dict(group_starts=[0, 5, 5, 3, n])):
        ranges = group_ranges(n, form.get("group_frames"), form.get("group_starts"))
        gp, _ = groups(codec, b1, win, **form)
        first = {s: getattr(gp, s).clone() for s in ALL + ("counts",)}
        groups(codec, b2, win, out=gp, accumulate=True, **form)
        e1, e2 = expect_groups(b1.images, ranges, *win), expect_groups(b2.images, ranges, *win)
        want = dict(max=torch.maximum(e1["max"], e2["max"]), min=torch.minimum(e1["min"], e2["min"]),
                    sum=e1["sum"] + e2["sum"], sumsq=e1["sumsq"] + e2["sumsq"],
                    counts=[a + c for a, c in zip(e1["counts"], e2["counts"])])
        assert_groups(gp, want, what=f"accumulated {form}")
        for k, (lo, hi) in enumerate(ranges):
            if lo == hi:
                for s in ALL + ("counts",):
                    assert torch.equal(getattr(gp, s)[k], first[s][k]), (k, s)
        groups(codec, b2, win, out=gp, **form)   # accumulate=False starts again
        assert_groups(gp, e2, what="reset")


def test_interleaved_with_other_calls_on_one_context(dv, codec, batches):
    """project_groups between decode_roi, encode_frames, project and histogram calls of other geometries: the index
    workspace is shared, the results are unchanged either way round."""
    import torch
    W, H, n = 200, 123, 13
    b, o = batches("mixed", W, H, n), batches("noise8", 64, 64, 2000)
    win, g = (5, 3, 131, 77), 3
    want = expect_groups(b.images, group_ranges(n, group_frames=g), *win)
    alone, _ = groups(codec, b, win, group_frames=g)
    assert_groups(alone, want, what="alone")

    def others():
        roi, _ = codec.decode_roi(o.buf, o.lead, o.total, o.offs, 64, 64, 2000, 3, 5, 40, 30)
        pr, _ = codec.project(o.buf, o.lead, o.total, o.offs, 64, 64, 2000)
        hs = codec.histogram(o.buf, o.lead, o.total, o.offs, 64, 64, 2000)
        buf, lead, cap = codec.alloc_stream(1921, 17, 3)
        codec.encode_frames(codec.synth_frames("smooth", 1, 0, 3, 1921, 17), 1921, 17, 3, buf, lead, cap)
        return roi, pr, hs

    ref = others()
    codec.sync()
    for _ in range(2):
        gp, res = codec.project_groups(b.buf, b.lead, b.total, b.offs, W, H, n, *win, group_frames=g)
        got = others()
        gq, _ = codec.project_groups(o.buf, o.lead, o.total, o.offs, 64, 64, 2000, group_frames=7, stats=("max", "sum"))
        gp2, _ = codec.project_groups(b.buf, b.lead, b.total, b.offs, W, H, n, *win, group_starts=[0, 4, 2, n])
        codec.sync()
        assert_groups(gp, want, what="before the others")
        assert_groups(gp2, expect_groups(b.images, group_ranges(n, starts=[0, 4, 2, n]), *win), what="after the others")
        assert_groups(gq, expect_groups(o.images, group_ranges(2000, group_frames=7), 0, 0, 64, 64), ("max", "sum"),
                      what="other geometry")
        assert torch.equal(res, b.results)
        assert torch.equal(got[0], ref[0])
        for s in ALL + ("count",):
            assert torch.equal(getattr(got[1], s), getattr(ref[1], s)), s
        h_got, h_ref = got[2][0], ref[2][0]
        assert torch.equal(h_got.counts, h_ref.counts)


def test_zero_frames_and_empty_ragged_batch(dv, codec, batches):
    import torch
    W, H = 200, 123
    b = batches("mixed", W, H, 13)
    gp, res = codec.project_groups(b.buf, b.lead, b.total, b.offs, W, H, 0, group_frames=4)   # does nothing
    codec.sync()
    assert gp.max.shape == (0, H, W) and res.shape == (0, 4)
    gp, _ = codec.project_groups(b.buf, b.lead, b.total, b.offs, W, H, 0, 7, 9, 50, 60, group_starts=[0, 3, 9])
    codec.sync()
    assert_groups(gp, reduce_groups([], [(0, 0), (0, 0)], 7, 9, 50, 60), what="ragged, no frames")


def test_mean_and_std_per_group(codec, batches):
    import torch
    W, H, n = 200, 123, 13
    b = batches("noise8", W, H, n)
    gp, _ = groups(codec, b, (0, 0, W, H), group_starts=[0, 5, 5, n], stats=("sum", "sumsq"))
    f = b.images.to(torch.float64)
    mean, std = gp.mean(), gp.std()
    assert torch.allclose(mean[0], f[:5].mean(0)) and torch.allclose(mean[2], f[5:].mean(0))
    assert torch.allclose(std[0], f[:5].std(0, unbiased=False)) and torch.allclose(std[2], f[5:].std(0, unbiased=False))
    assert torch.isnan(mean[1]).all() and torch.isnan(std[1]).all()


def test_argument_errors(dv, codec, batches):
    import torch
    W, H, n = 64, 64, 2000
    b = batches("noise8", W, H, n)
    with pytest.raises(ValueError):      # both forms / neither
        codec.project_groups(b.buf, b.lead, b.total, b.offs, W, H, n, group_frames=2, group_starts=[0, 2])
    with pytest.raises(ValueError):
        codec.project_groups(b.buf, b.lead, b.total, b.offs, W, H, n)
    with pytest.raises(ValueError):      # accumulate without planes to continue
        codec.project_groups(b.buf, b.lead, b.total, b.offs, W, H, n, group_frames=2, accumulate=True)
    L, h, ptr = codec.L, codec.h, b.buf.data_ptr() + b.lead
    raw = torch.full((1 << 16,), SENTINEL, dtype=torch.uint8, device="cuda")
    r, st = raw.data_ptr(), torch.zeros(4, dtype=torch.int32, device="cuda").data_ptr()

    def call(g, starts, ng, sum_type=0, acc=0, mx=None, mn=None, sm=None, sq=None, cnt=r + 1024, frames=4):
        return L.dbde_hip_project_groups(h, ptr, b.total, b.offs.data_ptr(), W, H, frames, 0, 0, 8, 8, g, starts, ng,
                                         sum_type, acc, mx, mn, sm, sq, cnt, None)
    assert call(2, None, 2, mx=r) == dv.OK
    assert call(2, st, 2, mx=r) == dv.ERR_ARG            # both forms
    assert call(0, None, 2, mx=r) == dv.ERR_ARG          # neither
    assert call(2, None, 3, mx=r) == dv.ERR_ARG          # n_groups != ceil(n / g)
    assert call(65537, None, 1, mx=r) == dv.ERR_ARG      # g > 65,536
    assert call(0, st, 0, mx=r) == dv.ERR_ARG            # ragged without a group
    assert call(2, None, 2) == dv.ERR_ARG                # no plane
    assert call(2, None, 2, mx=r, cnt=None) == dv.ERR_ARG
    assert call(2, None, 2, mx=r, cnt=r + 1026) == dv.ERR_ARG
    assert call(2, None, 2, sm=r + 2) == dv.ERR_ARG      # U32 sums at 2 mod 4
    assert call(2, None, 2, sm=r + 1, sum_type=1) == dv.ERR_ARG
    assert call(2, None, 2, sm=r + 2, sum_type=1) == dv.OK
    assert call(2, None, 2, sm=r + 4, sum_type=1, acc=1) == dv.ERR_ARG
    assert call(2, None, 2, sm=r, sum_type=2) == dv.ERR_ARG
    assert call(2, None, 2, sq=r + 4) == dv.ERR_ARG
    codec.sync()
    c = raw.cpu().numpy()
    c[:2 + 2 * 2 * 64] = SENTINEL  # the two accepted calls' planes
    c[1024:1032] = SENTINEL        # ... and counts
    assert (c == SENTINEL).all()
