"""GPU: the patch match on the state other calls leave in ONE context.

tests/sequences.py runs chains of calls of different families on one context and checks every step against its
reference; its helpers are used as they are, and the match is added here as one more consumer op (match_patches /
match_patches16: 12 x 8 templates at radius 3 on sequences.PATCH-sized search neighbourhoods of the pools' frames,
rejected frames among them).  The chain: a project, a decode_patches, a patch_moments and a persistent encode run before
and after the match, on pools whose decode index is split (A, 13 frames of 200 x 123), not split (D) and over 300 frames
(C), at both pixel sizes, stepwise and queued.  Every step equals its reference, which is what the same call gives on a
fresh context (the runner repeats a mismatching step on one and says which it was).
"""
import numpy as np
import pytest

import match_ref as mr
import patch_ref as pr
import sequences as sq
from test_gpu_crafted_decode import _codec
from test_oracle_u16 import o16   # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

TW, TH, S = 12, 8, 3
K = sq.PATCHES_PER_FRAME


def _templates(pool, prm):
    rng = np.random.default_rng(pool.W + pool.bits)
    return rng.integers(0, 1 << pool.bits, size=(1 if prm.get("shared") else K, TH, TW)).astype(np.uint8 if pool.bits == 8 else np.uint16)


def _templates_dev(pool, prm):
    import torch
    T = _templates(pool, prm)
    return sq.const(("match_T", pool.name, bool(prm.get("shared"))),
                    lambda: torch.from_numpy(T if pool.bits == 8 else T.view(np.int16)).cuda())


def _mask(prm):
    return prm.get("stats", 7)


def _outputs(pool, prm):
    f0, n = sq.frames_of(pool, prm)
    D = 2 * S + 1
    spec = {nm: ((n, K, D, D), "int64") for i, nm in enumerate(mr.NAMES) if _mask(prm) >> i & 1}
    return dict(spec, used=((n, K, 2), "int32"), **sq.results_spec(n))


def _run(codec, pool, prm, out):
    buf, lead, total, offs, W, H, n = sq.stream_args(pool, prm)
    org, cnt = sq._patch_inputs(pool, prm)
    fn = codec.match_patches if pool.bits == 8 else codec.match_patches16
    fn(buf, lead, total, offs, W, H, n, _templates_dev(pool, prm), S, org, counts=cnt, edge=prm.get("edge", "clamp"),
       fill=sq._patch_fill(pool, prm), stats=_mask(prm), out={nm: out[nm].t for nm in mr.NAMES if nm in out},
       used=out["used"].t, results=out["results"].t)


def _expect(pool, prm):
    f0, n = sq.frames_of(pool, prm)
    mode = pr.CLAMP if prm.get("edge", "clamp") == "clamp" else pr.FILL
    prod, sm, sq_, used, live = mr.expected(sq.images_or_none(pool, f0, n), pool.W, pool.H, _templates(pool, prm), S,
                                            sq.patch_origins_of(pool, prm), sq.patch_counts_of(pool, prm), mode,
                                            sq._patch_fill(pool, prm))
    want = {}
    for i, (nm, a) in enumerate(zip(mr.NAMES, (prod, sm, sq_))):
        if _mask(prm) >> i & 1:
            a[~live] = sq.FILLS["int64"]
            want[nm] = a
    used[~live] = sq.FILLS["int32"]
    return dict(want, used=used, results=sq.rows_array(pool.rows[f0:f0 + n]))


def _plan(pool, prm):
    dv = sq.dvm()
    f0, n = sq.frames_of(pool, prm)
    fn = dv.match_plan if pool.bits == 8 else dv.match16_plan
    pl = fn(pool.W, pool.H, n, TW, TH, S, K, 1 if prm.get("shared") else K, prm.get("edge", "clamp"), sq._patch_fill(pool, prm),
            _mask(prm))
    pl["index"] = sq.index_of_roi_plan(pool.bits, n, pl)
    return pl


for _b in (8, 16):
    _name = "match_patches" + sq.suffix(_b)
    sq.OPS[_name] = sq.Op(_name, _b, "consumer", _run, _expect, _plan, _outputs,
                          prepare=lambda codec, pool, prm: (sq._patch_inputs(pool, prm), _templates_dev(pool, prm)))


def chain(b):
    s = sq.suffix(b)
    A, C, D = f"A{b}", f"C{b}", f"D{b}"
    enc = ("encode:persistent", "persistent_big", {}) if b == 8 else ("encode:persistent16", "persistent16", {})
    m1 = ("match_patches" + s, A, dict(edge="fill", fill=0x1A5, counts=True))
    m2 = ("match_patches" + s, D, dict(edge="clamp", shared=True, stats=5))
    m3 = ("match_patches" + s, C, dict(edge="fill", fill=3, n=13, f0=250))
    before = [("project" + s, A, dict(w=1, stats=("max", "sum"))),
              ("decode_patches" + s, A, dict(edge="fill", fill=0x1A5, counts=True)),
              ("patch_moments" + s, D, dict(edge="clamp", weight="above", band="tile", bbox=True)),
              enc]
    return before + [m1] + before + [m2, m1, enc, m3, ("project" + s, A, {}), m2, m3]


CASES = [(b, mode) for b in (8, 16) for mode in ("stepwise", "queued")]


@pytest.fixture(scope="module")
def dv():
    import dbde_video_cpp_amd as m
    return m


@pytest.fixture(scope="module")
def things(oracle, o16):   # noqa: F811
    return sq.everything(oracle, o16)


@pytest.mark.parametrize("bits,mode", CASES, ids=[f"{b}-{m}" for b, m in CASES])
def test_match_between_other_families(dv, things, tmp_path, bits, mode):
    steps = chain(bits)
    pools = {things[p].name: things[p] for _, p, _ in steps if p[0] in "ACD"}
    A = pools[f"A{bits}"]
    assert _plan(A, dict(edge="fill"))["index"]["split"] > 1 and _plan(pools[f"D{bits}"], {})["index"]["split"] == 1
    assert not all(A.ok) and not all(pools[f"C{bits}"].ok[250:263])   # rejected frames inside the matched ranges
    codec = _codec(dv)
    try:
        outputs, elements = sq.run_chain(codec, things, f"match {bits}-bit", steps, mode, tmp=tmp_path)
    finally:
        codec.close()
    assert outputs >= len(steps) and elements > 0, (outputs, elements)
