"""GPU: patch match -- dbde_hip_match_patches (Codec.match_patches): the correlation surfaces of templates over a shift
search, straight from the compressed stream.

Every comparison is exact integer equality with tests/match_ref.py (the patch decoder's patch, then the three sums) over
the frames that were encoded; for crafted frames over crafted.decode_frame's images.  The surfaces and used origins are
written into 0xEE canvases with guard bands in front of and behind them, so "untouched" and "nothing outside" are
checked.  The cases are tests/match_cases.py's, each capped on the CPU by tests/test_match_ref.py: radii 0, 1, 2, 8, 16;
templates from 1 x 1 to 128 x 128; all 64 origin residues; FILL over every edge and corner and wholly outside; CLAMP
clamped on every side; one shared and per-patch templates for K = 1, 3, 70; counts; every stats mask.
"""
import numpy as np
import pytest

import match_cases as mc
import match_gpu as mg
import match_ref as mr
import patch_ref as pr

pytestmark = pytest.mark.gpu

BITS = 8


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


@pytest.mark.parametrize("c", mc.CASES, ids=mc.IDS)
def test_cases_match_match_ref(codec, c):
    mg.run_case(codec, c, BITS)


def test_rejected_and_truncated_frames_stay_untouched(codec):
    mg.run_rejected(codec, BITS)


def test_overflow_witness_all_255(codec):
    mg.run_overflow_witness(codec, BITS)


def test_decode_patches_plus_torch_agree(codec):
    mg.run_cross_check(codec, BITS)


def test_best_and_refine_against_the_reference(codec):
    """best's tie rule and NaN handling on the device equal tests/match_ref.best entry by entry; refine's offset is the
    parabola's, 0 on the border."""
    import torch
    c = next(c for c in mc.CASES if c["name"] == "t8x8_S2")
    frames, T, org, _ = mc.content(c, BITS)
    frames[0][:] = 77                                   # a flat frame: every zncc entry NaN, every ssd entry tied in runs
    e = mg.Encoded(codec, frames, BITS)
    d_org = torch.from_numpy(org.astype(np.int32)).cuda()
    pm, _ = codec.match_patches(*e.stream, c["W"], c["H"], c["n"], mg.dev_templates(T, BITS), c["S"], d_org,
                                edge="clamp" if c["mode"] == pr.CLAMP else "fill", fill=mc.fill_of(c, BITS))
    z, ssd = pm.zncc().cpu().numpy(), pm.ssd().cpu().numpy()
    for score, surf, up in (("zncc", z, True), ("ssd", ssd, False)):
        shifts, val = pm.best(score)
        sub = pm.refine(score).cpu().numpy()
        shifts, val = shifts.cpu().numpy(), val.cpu().numpy()
        for f in range(c["n"]):
            for k in range(org.shape[1]):
                want, wv = mr.best(surf[f, k].astype(np.float64) if up else surf[f, k], c["S"], maximize=up)
                assert tuple(shifts[f, k]) == want, (score, f, k)
                assert (np.isnan(val[f, k]) and np.isnan(wv)) or val[f, k] == wv
                s, S = surf[f, k].astype(np.float64), c["S"]
                r, col = want[1] + S, want[0] + S
                for axis, (a, b, pos) in enumerate((((r, col - 1), (r, col + 1), col), ((r - 1, col), (r + 1, col), r))):
                    off = 0.0
                    if 0 < pos < 2 * S:
                        lo, mid, hi = s[a], s[r, col], s[b]
                        with np.errstate(all="ignore"):
                            o = 0.5 * (lo - hi) / (lo - 2 * mid + hi)
                        off = o if np.isfinite(o) else 0.0
                    assert sub[f, k, axis] == want[axis] + off, (score, f, k, axis)
    assert np.isnan(z[0]).all() and (pm.best()[0][0] == 0).all()


def test_timing_hook_zero_frames_and_argument_errors(codec, dv):
    import torch
    W, H, n = 139, 99, 2
    rng = np.random.default_rng(4)
    e = mg.Encoded(codec, rng.integers(0, 256, size=(n, H, W)).astype(np.uint8))
    buf, lead, total, offs = e.stream
    org = torch.zeros((n, 3, 2), dtype=torch.int32, device="cuda")
    T = torch.full((3, 8, 8), 9, dtype=torch.uint8, device="cuda")
    codec.timing(True)
    codec.timing_read(reset=True)
    codec.match_patches(buf, lead, total, offs, W, H, n, T, 2, org)
    t = codec.timing_read(reset=True)
    codec.timing(False)
    assert t["decode_index"][1] == 1 and t["decode"][1] == 1 and t["encode"][1] == 0
    surf = [torch.full((n * 3 * 25 + 1,), mr.UNTOUCHED, dtype=torch.int64, device="cuda") for _ in range(3)]
    usd = torch.full((n * 3 * 2 + 1,), pr.UNTOUCHED_ORIGIN, dtype=torch.int32, device="cuda")

    def call(n_frames=n, tw=8, th=8, S=2, K=3, origins=org, edge=0, fill=0, templates=T, Kt=3, stats=7, prod=surf[0],
             sm=surf[1], sq=surf[2], used=usd):
        ptr = lambda v: v.data_ptr() if torch.is_tensor(v) else v   # noqa: E731
        return codec.L.dbde_hip_match_patches(codec.h, buf.data_ptr() + lead, total, offs.data_ptr(), W, H, n_frames, tw, th, S,
                                              K, ptr(origins), None, edge, fill, ptr(templates), Kt, stats, ptr(prod), ptr(sm),
                                              ptr(sq), ptr(used), None)

    assert call(n_frames=0) == dv.OK
    bad = [dict(tw=0), dict(th=0), dict(tw=129), dict(th=129), dict(S=-1), dict(S=17), dict(tw=128, S=8), dict(th=90, S=5),
           dict(edge=2), dict(fill=256), dict(K=0), dict(Kt=2), dict(Kt=0), dict(stats=0), dict(stats=8), dict(origins=None),
           dict(templates=None), dict(prod=None), dict(sm=None), dict(sq=None), dict(prod=surf[0].data_ptr() + 4),
           dict(sq=surf[2].data_ptr() + 2), dict(used=usd.data_ptr() + 2), dict(n_frames=-1)]
    for kw in bad:
        assert call(**kw) == dv.ERR_ARG, kw
    codec.sync()
    assert all((s == mr.UNTOUCHED).all() for s in surf) and (usd == pr.UNTOUCHED_ORIGIN).all()
    # a surface outside the mask may be NULL or misaligned; the used origins are optional; one template serves all
    assert call(stats=1, sm=None, sq=surf[2].data_ptr() + 4) == dv.OK and call(stats=6, prod=None) == dv.OK
    assert call(used=None) == dv.OK and call(Kt=1) == dv.OK and call(S=0) == dv.OK and call(edge=1, S=1) == dv.OK
    codec.sync()
    for kw in (dict(S=17), dict(S=-1), dict(fill=256), dict(fill=-1), dict(fill=2 ** 32), dict(stats=0), dict(stats=8),
               dict(stats=2 ** 32 + 1), dict(edge=2)):
        a = dict(S=2, fill=0, stats=7, edge="clamp")
        a.update(kw)
        for nn in (n, 0):   # refused for any n (also n = 0, where the C call is not made); nothing wraps modulo 2^32
            with pytest.raises(dv.DbdeError, match="match_patches"):
                codec.match_patches(buf, lead, total, offs, W, H, nn, T, a["S"], org[:nn], edge=a["edge"], fill=a["fill"],
                                    stats=a["stats"])
    with pytest.raises(dv.DbdeError, match="dbde16_hip_match_patches"):
        codec.match_patches16(buf, lead, total, offs, W, H, 0, T.to(torch.int16), 2, org[:0], fill=65536)
    pm, _ = codec.match_patches(buf, lead, total, offs, W, H, 0, T, 2, org[:0], stats=("prod",))
    assert tuple(pm.prod.shape) == (0, 3, 5, 5) and pm.sum is None and pm.sq is None
    with pytest.raises(ValueError, match="not requested"):
        pm.zncc()
    for wrong in (org.to(torch.int64), org[:, :, :1], org.permute(1, 0, 2), org[:1]):
        with pytest.raises(ValueError, match="origins"):
            codec.match_patches(buf, lead, total, offs, W, H, n, T, 2, wrong)
    for wrong in (T.to(torch.int16), T[:2], T[0], T.permute(0, 2, 1)[:, :, :4]):
        with pytest.raises(ValueError, match="templates"):
            codec.match_patches(buf, lead, total, offs, W, H, n, wrong, 2, org)
    with pytest.raises(ValueError, match="stats"):
        codec.match_patches(buf, lead, total, offs, W, H, n, T, 2, org, stats=("prod", "mean"))
