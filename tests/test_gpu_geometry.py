"""GPU: every stream-reading family x {8, 16} bits at the four geometries of tests/geometry_cases.py -- regime A at its
widest row (prefixes of up to 511 depth bytes), regime B at its smallest and with three pieces (the split index), and
regime C with tile rows that straddle chunk boundaries.

Every kernel that reads a window of a compressed frame carries its own copy of the front half (the chunk of its first
tile and the sum of the depth bytes in front of it); a wrong prefix sum, a wrong chunk for a straddled row or a wrong
piece seam in one copy shows only where that copy runs at such a frame.  tests/test_geometry_cases.py proves on the CPU
that the windows, origins and patches sit on those spots and that a wrong tile changes every expected value; here each
family makes one call per window (origin set, patch set) and is compared with the numpy reference it already has:

  * twelve families through tests/sequences.py's run / expect pairs into guarded canvases (the window, origins, patch
    origins and label map come in the step parameters): equality of every output element, of the result rows with the
    crafted frames' verdicts, the guard bands, and the canvas fill where the rejected frame must leave its output alone;
    project_weighted by its bit-exact chain of fused multiply-adds over the plan's segments;
  * count projections (and one quantiles call on top), neighbour-product, lag (lags 1 and 2: pairs that span the
    rejected frame) and registered projections and match_patches through counts_gpu, pairs_gpu, lag_gpu.check,
    registered_gpu and match_gpu: equality with their references, the rejected frame counted for nothing.

One context and one upload of each stream per (geometry, pixel size) serve the whole module.
"""
import time
from importlib import import_module

import numpy as np
import pytest

import counts_gpu as cg
import counts_ref as cref
import geometry_cases as gc
import lag_gpu as lg
import match_gpu as mg
import pairs_gpu as pg
import registered_gpu as rg
import registered_ref as rr
import sequences as sq

pytestmark = pytest.mark.gpu

SEQUENCED = ("decode_roi", "project", "traces", "histogram", "decode_binned", "decode_scaled", "crop_frames",
             "decode_mask", "decode_patches", "project_groups", "project_weighted", "patch_moments")
NEWER = ("project_counts", "project_pairs", "project_lag", "project_registered", "match_patches")
FAMILIES = SEQUENCED + NEWER
CASES = [(family, bits, name) for family in FAMILIES for bits in gc.BITS for name in gc.NAMES]
T0 = [None]


@pytest.fixture(scope="module")
def dv():
    import dbde_video_cpp_amd as m
    return m


@pytest.fixture(scope="module")
def codec(dv):
    T0[0] = time.time()
    c = dv.Codec(0)
    assert c.arch.startswith("gfx950")
    yield c
    c.close()
    print(f"\ntest_gpu_geometry: {len(CASES)} cases in {time.time() - T0[0]:.1f} s")


def steps_of(family, name):
    """The step parameters (tests/sequences.py) of one family at one geometry: one call per window, and one per set of
    moving origins where the family takes per-frame origins."""
    wins = gc.WINDOWS[name]
    (rw, rh), org = gc.MOVING[name]
    moving = dict(win=(0, 0, rw, rh), origins=org)
    if family == "decode_roi":
        return [dict(win=w) for w in wins] + [moving]
    if family == "project":
        return [dict(win=w) for w in wins]
    if family == "traces":                       # the windows are the regions (later ones over earlier ones)
        return [dict(label_windows=wins[::-1])]
    if family == "histogram":
        return [dict(win=w) for w in wins]
    if family == "decode_binned":
        return [dict(win=gc.aligned(w), bin=(2, 4, 8)[k % 3]) for k, w in enumerate(wins)]
    if family == "decode_scaled":
        return [dict(win=w, type=("f32", "f16", "bf16")[k % 3]) for k, w in enumerate(wins)] + [dict(moving, type="f32")]
    if family == "crop_frames":
        return [dict(win=gc.aligned(w)) for w in wins] + [moving]            # (the origins are rounded down to multiples of 8)
    if family == "decode_mask":
        return [dict(win=w, maps=k % 2 == 0, boxes=True) for k, w in enumerate(wins)] + [dict(moving, boxes=True)]
    if family == "decode_patches":
        return [dict(porg=gc.patch_origins(name), edge="clamp"), dict(porg=gc.patch_origins(name), edge="fill", fill=0x5A5A)]
    if family == "project_groups":
        return [dict(win=w, g=2) for w in wins]
    if family == "project_weighted":
        return [dict(win=w, R=2) for w in wins]
    if family == "patch_moments":
        return [dict(porg=gc.patch_origins(name), edge="clamp", bbox=True),
                dict(porg=gc.patch_origins(name), edge="fill", bbox=True, weight="value")]
    raise KeyError(family)


def rows_match(res, pool, what):
    """The call's result rows against the crafted frames' (u64s is a U32 in a U64 slot: its low half is specified)."""
    got = res.cpu().numpy().copy()
    want = sq.rows_array(pool.rows)
    got[:, 0] &= 0xFFFFFFFF
    want[:, 0] &= 0xFFFFFFFF
    assert np.array_equal(got, want), (what, got.tolist(), want.tolist())
    assert [int(r[3]) == 20 for r in got] == [not ok for ok in pool.ok]


def run_counts(codec, name, bits):
    s, pool = gc.stream(name, bits), gc.pool(name, bits)
    call = codec.project_counts if bits == 8 else codec.project_counts16
    rng = np.random.default_rng(gc.seed_of(name, bits) + 1)
    for k, win in enumerate(gc.WINDOWS[name]):
        maps = k == 1
        thr = cg.draw(rng, s.images, win, 3, bits, maps)
        out, res = cg.check(call, s, thr, win, what=f"{name} {bits}-bit")
        assert int(out.count.item()) == gc.N - 1
        rows_match(res, pool, ("project_counts", name, win))
    # one exact quantile on top: the median of the accepted frames at the first window
    qt = import_module("dbde_video_cpp_amd.quantiles")
    win = gc.WINDOWS[name][0]
    med, count, res = qt.temporal_quantile(codec, s.buf, s.lead, s.total, s.offs, s.W, s.H, s.n, 0.5, *win, bits=bits)
    codec.sync()
    want, _ = cref.order_statistic(s.images, 0.5, *win)
    got = med.cpu().numpy()
    assert np.array_equal(got if bits == 8 else got.view(np.uint16), want), (name, bits, "temporal_quantile")
    assert int(count.item()) == gc.N - 1
    rows_match(res, pool, ("temporal_quantile", name))


def run_pairs(codec, name, bits):
    s, pool = gc.stream(name, bits), gc.pool(name, bits)
    call = codec.project_pairs if bits == 8 else codec.project_pairs16
    for win in gc.WINDOWS[name]:
        out, res = pg.check(call, s, 15, win, what=f"{name} {bits}-bit")
        assert int(out.count.item()) == gc.N - 1
        rows_match(res, pool, ("project_pairs", name, win))


def run_lag(codec, name, bits):
    """Lags 1 and 2: frame BAD = 2 voids the pairs (1, 2), (2, 3) and (0, 2), (2, 4)."""
    s, pool = gc.stream(name, bits), gc.pool(name, bits)
    for win in gc.WINDOWS[name]:
        for lag, pairs in ((1, 2), (2, 1)):
            out, res = lg.check(codec, s, lag, win, bits=bits, what=name)
            assert int(out.pairs.item()) == pairs and int(out.count.item()) == gc.N - 1
            rows_match(res, pool, ("project_lag", name, win, lag))


def run_registered(codec, name, bits):
    import torch
    s, pool = gc.stream(name, bits), gc.pool(name, bits)
    (rw, rh), org = gc.MOVING[name]
    origins = np.array(org, np.int64)
    spec = ("crafted", gc.seed_of(name, bits), s.W, s.H, s.n, bits, (gc.BAD,))
    want = rg.cap(s.images, spec, rw, rh, origins, 15)
    names = rr.names_of(15)
    used = torch.full((s.n, 2), rg.SENT, dtype=torch.int32, device="cuda")
    out, res = rg.call_of(codec, bits)(s.buf, s.lead, s.total, s.offs, s.W, s.H, s.n, rw, rh, rg.device_origins(origins),
                                       stats=names, origins_used=used)
    codec.sync()
    rg.compare(out, want, names, f"{name} {rw}x{rh} {bits}-bit")
    u = used.cpu().numpy()
    for f in range(s.n):      # the rejected frame's row keeps the sentinel
        assert tuple(u[f]) == (want["used"].get(f, (rg.SENT, rg.SENT))), (name, f, "origins_used")
        assert (f in want["used"]) == (f != gc.BAD)
    assert int(out.count.item()) == gc.N - 1
    rows_match(res, pool, ("project_registered", name))


def run_match(codec, name, bits):
    pool = gc.pool(name, bits)
    buf, offs = pool.dev()
    for tw, th, S in gc.MATCH:
        res = mg.check_match(codec, (buf, pool.lead, pool.total, offs), list(pool.images), pool.W, pool.H,
                             gc.templates(name, bits, tw, th), S, gc.search_origins(name, S), None,
                             gc.match_mode(name, tw, th, S), 0x5A, 7, bits, what=name)
        rows_match(res, pool, ("match_patches", name, S))


RUN = dict(project_counts=run_counts, project_pairs=run_pairs, project_lag=run_lag, project_registered=run_registered,
           match_patches=run_match)


@pytest.mark.parametrize("family,bits,name", CASES, ids=[f"{f}{sq.suffix(b)}-{g}" for f, b, g in CASES])
def test_family_at_geometry(codec, family, bits, name):
    pool = gc.pool(name, bits)
    assert pool.ok == [f != gc.BAD for f in range(gc.N)]
    if family in RUN:
        RUN[family](codec, name, bits)
        return
    op = family + sq.suffix(bits)
    steps = [(op, pool.name, prm) for prm in steps_of(family, name)]
    outputs, elements = sq.run_chain(codec, {pool.name: pool}, f"{op} at {name}", steps, "stepwise")
    assert outputs >= 2 * len(steps) and elements > 0, (outputs, elements)
    for step in steps:        # every step compared its result rows (with the rejected frame's) and something else
        spec = sq.OPS[op].outputs(pool, step[2])
        assert "results" in spec and len(spec) >= 2
