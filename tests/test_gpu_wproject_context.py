"""GPU: the weighted projection on the state other calls leave in ONE context.

A short chain on a single context, two streams of different geometry: project_weighted, decode_roi, project_weighted
(several segments: the partials share the projections' workspace), project (all four statistics, several segments: it
re-lays-out that workspace), decode_patches, project_weighted16 on a DBDE16 stream, and the first calls again.  Every
weighted result is compared bit for bit with tests/wproject_ref.py's chain, and every call's outputs with what the same
call gave on a context of its own.  The geometries, windows and images are tests/sequences.py's (import only).
"""
import numpy as np
import pytest

import sequences as sq
import wproject_gpu as wg
import wproject_ref as wr
from test_gpu_project import Batch
from test_gpu_roi16 import Batch16
from test_oracle_u16 import o16   # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dv():
    return sq.dvm()


def test_weighted_projection_between_other_families(dv, o16):   # noqa: F811
    import torch
    rng = np.random.default_rng(17)
    (Wa, Ha), (Wb, Hb) = (200, 123), (72, 72)
    wins_a, wins_b = sq.WINDOWS[(Wa, Ha)], sq.WINDOWS[(Wb, Hb)]
    na, nb = 13, 70
    maker = dv.Codec(0)
    a = Batch(maker, None, Wa, Ha, na, images=torch.from_numpy(sq.mixed_images(rng, na, Ha, Wa, 8)).cuda())
    b = Batch(maker, None, Wb, Hb, nb, images=torch.from_numpy(sq.mixed_images(rng, nb, Hb, Wb, 8)).cuda())
    c = Batch16(maker, o16, sq.mixed_images(rng, na, Hb, Wb, 16))
    maker.close()
    wa, wb = wg.family(rng, "normal", 3, na), wg.family(rng, "normal", 8, nb)
    wa_d, wb_d, wc_d = wg.strided(wa), wg.strided(wb), wg.strided(wa[:2])
    origins = torch.from_numpy(rng.integers(0, 60, (na, 4, 2)).astype(np.int32)).cuda()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert dv.wproject_plan(Wb, Hb, nb, *wins_b[1], regressors=8, n_cu=cus)["segments"] > 1
    assert dv.project_plan(Wb, Hb, nb, *wins_b[1], n_cu=cus)["segments"] > 1

    steps = [
        ("wproject a", lambda k: k.project_weighted(a.buf, a.lead, a.total, a.offs, Wa, Ha, na, wa_d, *wins_a[1])),
        ("decode_roi a", lambda k: k.decode_roi(a.buf, a.lead, a.total, a.offs, Wa, Ha, na, *wins_a[1])),
        ("wproject b", lambda k: k.project_weighted(b.buf, b.lead, b.total, b.offs, Wb, Hb, nb, wb_d, *wins_b[1])),
        ("project b", lambda k: k.project(b.buf, b.lead, b.total, b.offs, Wb, Hb, nb, *wins_b[1])),
        ("wproject b, one segment", lambda k: k.project_weighted(b.buf, b.lead, b.total, b.offs, Wb, Hb, nb, wb_d,
                                                                 *wins_b[0], one_segment=True)),
        ("decode_patches a", lambda k: k.decode_patches(a.buf, a.lead, a.total, a.offs, Wa, Ha, na, 24, 16, origins)),
        ("wproject16 c", lambda k: k.project_weighted16(c.buf, c.lead, c.total, c.offs, Wb, Hb, na, wc_d, *wins_b[1])),
        ("wproject a", None), ("wproject b", None), ("project b", None),
    ]
    calls = dict((name, fn) for name, fn in steps if fn)

    def tensors(ret):
        out = []
        for r in ret:
            if torch.is_tensor(r):
                out.append(r)
            elif r is not None:
                out += [t for t in vars(r).values() if torch.is_tensor(t)]
        return [t.view(torch.int32) if t.dtype == torch.float32 else t for t in out]

    alone = {}
    for name, fn in calls.items():      # every call on a context of its own
        k = dv.Codec(0)
        try:
            alone[name] = [t.clone() for t in tensors(fn(k))]
            k.sync()
        finally:
            k.close()
    shared = dv.Codec(0)
    try:
        for mode in ("stepwise", "queued"):
            got = []
            for name, _ in steps:
                got.append((name, tensors(calls[name](shared))))
                if mode == "stepwise":
                    shared.sync()
            shared.sync()
            for i, (name, ts) in enumerate(got):
                assert len(ts) == len(alone[name]) > 0
                for t, want in zip(ts, alone[name]):
                    assert torch.equal(t, want), f"{mode}: step {i} ({name}) differs from the call on a fresh context"
    finally:
        shared.close()

    # and the weighted planes are the defined value
    for name, s, w, win, one in [("wproject a", a, wa, wins_a[1], False), ("wproject b", b, wb, wins_b[1], False),
                                 ("wproject b, one segment", b, wb, wins_b[0], True)]:
        plan = dv.wproject_plan(s.W, s.H, s.n, *win, regressors=w.shape[0], n_cu=cus, one_segment=one)
        want, count = wr.wproject(list(s.images.cpu().numpy()), w, *win, segments=plan["segments"],
                                  fps=plan["frames_per_segment"])
        wg.assert_bits(alone[name][0].view(torch.float32), want, name)
        assert int(alone[name][1].item()) == count
    plan = dv.wproject16_plan(Wb, Hb, na, *wins_b[1], regressors=2, n_cu=cus)
    want, _ = wr.wproject(c.full, wa[:2], *wins_b[1], segments=plan["segments"], fps=plan["frames_per_segment"])
    wg.assert_bits(alone["wproject16 c"][0].view(torch.float32), want, "wproject16 c")
