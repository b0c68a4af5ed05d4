"""GPU: the pair projection on the state other calls leave in ONE context.

A short chain on a single context, two streams of different geometry: project_pairs, decode_roi, project_pairs (several
segments: the partials share the projections' workspace), project (all four statistics, several segments: it
re-lays-out that workspace), project_counts, project_weighted, decode_patches, project_pairs16 on a DBDE16 stream
(several segments: U64 partials in the same workspace), and the first calls again.  Every pair result equals
tests/pairs_ref.py, and every call's outputs equal what the same call gave on a context of its own.  The geometries,
windows and images are tests/sequences.py's (import only).
"""
import numpy as np
import pytest

import counts_gpu as cg
import pairs_ref as pref
import sequences as sq
import wproject_gpu as wg
from test_gpu_project import Batch
from test_gpu_roi16 import Batch16
from test_oracle_u16 import o16   # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dv():
    return sq.dvm()


def test_pair_projection_between_other_families(dv, o16):   # noqa: F811
    import torch
    rng = np.random.default_rng(23)
    (Wa, Ha), (Wb, Hb) = (200, 123), (72, 72)
    wins_a, wins_b = sq.WINDOWS[(Wa, Ha)], sq.WINDOWS[(Wb, Hb)]
    na, nb = 13, 70
    maker = dv.Codec(0)
    a = Batch(maker, None, Wa, Ha, na, images=torch.from_numpy(sq.mixed_images(rng, na, Ha, Wa, 8)).cuda())
    b = Batch(maker, None, Wb, Hb, nb, images=torch.from_numpy(sq.mixed_images(rng, nb, Hb, Wb, 8)).cuda())
    c = Batch16(maker, o16, sq.mixed_images(rng, nb, Hb, Wb, 16))
    maker.close()
    ia, ib = list(a.images.cpu().numpy()), list(b.images.cpu().numpy())
    tb_d = cg.device(cg.draw(rng, ib, wins_b[1], 8, 8, True))
    wb_d = wg.strided(wg.family(rng, "normal", 8, nb))
    origins = torch.from_numpy(rng.integers(0, 60, (na, 4, 2)).astype(np.int32)).cuda()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert dv.pairs_plan(Wb, Hb, nb, *wins_b[1], pairs=15, n_cu=cus)["segments"] > 1
    assert dv.pairs16_plan(Wb, Hb, nb, *wins_b[1], pairs=3, n_cu=cus)["segments"] > 1
    assert dv.project_plan(Wb, Hb, nb, *wins_b[1], n_cu=cus)["segments"] > 1
    o10 = pref.offsets_of(10)

    steps = [
        ("pairs a", lambda k: k.project_pairs(a.buf, a.lead, a.total, a.offs, Wa, Ha, na, 8, *wins_a[1])),
        ("decode_roi a", lambda k: k.decode_roi(a.buf, a.lead, a.total, a.offs, Wa, Ha, na, *wins_a[1])),
        ("pairs b", lambda k: k.project_pairs(b.buf, b.lead, b.total, b.offs, Wb, Hb, nb, 8, *wins_b[1])),
        ("project b", lambda k: k.project(b.buf, b.lead, b.total, b.offs, Wb, Hb, nb, *wins_b[1])),
        ("pairs b, mask 10", lambda k: k.project_pairs(b.buf, b.lead, b.total, b.offs, Wb, Hb, nb, o10, *wins_b[0])),
        ("counts b", lambda k: k.project_counts(b.buf, b.lead, b.total, b.offs, Wb, Hb, nb, tb_d, *wins_b[1])),
        ("pairs b, right", lambda k: k.project_pairs(b.buf, b.lead, b.total, b.offs, Wb, Hb, nb, 1, *wins_b[1])),
        ("wproject b", lambda k: k.project_weighted(b.buf, b.lead, b.total, b.offs, Wb, Hb, nb, wb_d, *wins_b[1])),
        ("decode_patches a", lambda k: k.decode_patches(a.buf, a.lead, a.total, a.offs, Wa, Ha, na, 24, 16, origins)),
        ("pairs16 c", lambda k: k.project_pairs16(c.buf, c.lead, c.total, c.offs, Wb, Hb, nb, 4, *wins_b[1])),
        ("pairs a", None), ("pairs b", None), ("project b", None), ("counts b", None),
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

    # and the pair planes are the reference's
    for name, images, mask, win in [("pairs a", ia, 15, wins_a[1]), ("pairs b", ib, 15, wins_b[1]),
                                    ("pairs b, mask 10", ib, 10, wins_b[0]), ("pairs b, right", ib, 1, wins_b[1]),
                                    ("pairs16 c", c.full, 3, wins_b[1])]:
        want, count = pref.pairs(images, mask, *win)
        assert np.array_equal(alone[name][0].cpu().numpy().view(np.uint64), want), name
        assert int(alone[name][1].item()) == count
