"""GPU: the registered projection on the state other calls leave in ONE context.

A chain on a single context, three streams (200 x 123 and 77 x 45 at 8 bits, 200 x 123 at 16): project_registered is
interleaved with project, project_pairs, project_lag and decode_roi, with windows and frame counts that take the
projections' shared workspace up and down (no partials at n = 13, partials of one to four statistics at n = 70, U64
partials at 16 bits, project's, project_pairs' and project_lag's own layouts in between), and the first calls come again
at the end.  Every registered result equals tests/registered_ref.py, and every call's outputs equal what the same call
gave on a context of its own.
"""
import numpy as np
import pytest

import lag_gpu as lg
import registered_cases as rc
import registered_gpu as rg
import registered_ref as rr

pytestmark = pytest.mark.gpu


def test_registered_projection_between_other_families():
    import torch
    import dbde_video_cpp_amd as dv
    W, H = rc.BIG
    a = lg.stream(*rc.noise(W, H, 70, 8, 5))
    b = lg.stream(*rc.crafted(*rc.FRAME, rc.N_ALL, 8, rc.BAD))
    c = lg.stream(*rc.noise(W, H, 70, 16, 5))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    big = dv.registered_plan(W, H, 70, 150, 100, n_cu=cus)
    small = dv.registered_plan(W, H, 70, 41, 27, stats=4, n_cu=cus)
    assert big["segments"] > 1 and small["segments"] > 1 and big["workspace_bytes"] > small["workspace_bytes"] > 0
    assert dv.registered_plan(W, H, 13, 150, 100, n_cu=cus)["workspace_bytes"] == 0
    assert dv.registered16_plan(W, H, 70, 150, 100, n_cu=cus)["segments"] > 1

    def args(s, n):
        return (s.buf, s.lead, s.total, s.offs, s.W, s.H, n)

    o_big = rc.segment_origins(70, W, H, 150, 100, 5)
    o_small = rc.segment_origins(70, W, H, 41, 27, 9)
    o_b = rc.rejected(8)[0][4]
    reg_steps = {      # name: (stream, n, rw, rh, origins, stats mask, bits)
        "reg a big": (a, 70, 150, 100, o_big, 15, 8),
        "reg a 13": (a, 13, 150, 100, o_big[:13], 3, 8),
        "reg a small": (a, 70, 41, 27, o_small, 4, 8),
        "reg b": (b, rc.N_ALL, *rc.WINDOW, o_b, 10, 8),
        "reg16 c": (c, 70, 150, 100, o_big, 15, 16),
    }
    dev = {name: rg.device_origins(st[4]) for name, st in reg_steps.items()}

    def reg_call(name):
        s, n, rw, rh, _, mask, bits = reg_steps[name]
        return lambda k: rg.call_of(k, bits)(*args(s, n), rw, rh, dev[name], stats=rr.names_of(mask))

    steps = [
        ("reg a big", reg_call("reg a big")),
        ("decode_roi a", lambda k: k.decode_roi(*args(a, 13), 0, 0, 41, 27, origins=dev["reg a small"])),
        ("reg a 13", reg_call("reg a 13")),
        ("project a", lambda k: k.project(*args(a, 70), 3, 5, 41, 27)),
        ("reg a small", reg_call("reg a small")),
        ("pairs b", lambda k: k.project_pairs(*args(b, rc.N_ALL), 8)),
        ("reg b", reg_call("reg b")),
        ("lag a", lambda k: k.project_lag(*args(a, 70), 3, ("product", "sqdiff", "maxdiff"), 0, 3, 5, 41, 27)),
        ("reg16 c", reg_call("reg16 c")),
        ("project16 c", lambda k: k.project16(*args(c, 70), 3, 5, 41, 27)),
        ("reg a big", None), ("reg a 13", None), ("project a", None), ("reg b", None), ("reg16 c", None),
    ]
    calls = dict((name, fn) for name, fn in steps if fn)

    def tensors(ret):
        out = []
        for r in ret:
            if torch.is_tensor(r):
                out.append(r)
            elif r is not None:
                out += [t for t in vars(r).values() if torch.is_tensor(t)]
        return out

    alone = {}
    for name, fn in calls.items():      # every call on a context of its own
        k = dv.Codec(0)
        try:
            ret = fn(k)
            k.sync()
            alone[name] = (ret, [t.clone() for t in tensors(ret)])
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
                assert len(ts) == len(alone[name][1]) > 0
                for t, want in zip(ts, alone[name][1]):
                    assert torch.equal(t, want), f"{mode}: step {i} ({name}) differs from the call on a fresh context"
    finally:
        shared.close()

    # and the registered planes are the reference's
    for name, (s, n, rw, rh, origins, mask, bits) in reg_steps.items():
        want = rr.registered(s.images[:n], origins, rw, rh, bits)
        rg.compare(alone[name][0][0], want, rr.names_of(mask), name)
    assert np.array_equal(alone["project a"][0][0].sum.cpu().numpy(),
                          sum(im[5:32, 3:44].astype(np.int64) for im in a.images))
