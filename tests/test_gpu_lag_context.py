"""GPU: the lag projection on the state other calls leave in ONE context.

A chain on a single context, three streams (200 x 123 and 72 x 40 at 8 bits, 200 x 123 at 16): project_lag is
interleaved with project, project_pairs, project_counts and decode_roi, with windows and frame counts that take the
projections' shared workspace up and down (no partials at n = 13, partials of 1 to 5 statistics at n = 70, U64 partials
at 16 bits, project's and project_pairs' own layouts in between), and the first calls come again at the end.  Every lag
result equals tests/lag_ref.py, and every call's outputs equal what the same call gave on a context of its own.
"""
import numpy as np
import pytest

import lag_cases as lc
import lag_gpu as lg
import lag_ref as lr

pytestmark = pytest.mark.gpu


def test_lag_projection_between_other_families():
    import torch
    import dbde_video_cpp_amd as dv
    a = lg.stream(*lc.noise(8, 70))
    b = lg.stream("noise", 5, 72, 40, 70, 8, (3, 40))
    c = lg.stream(*lc.noise(16, 70))
    full, small, one = lg.WINDOWS[0], lg.SMALL, lg.WINDOWS[3]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert dv.lag_plan(*lg.FRAME, 70, *small, lag=3, n_cu=cus)["segments"] > 1
    assert dv.lag_plan(*lg.FRAME, 70, *full, lag=8, stats=1, n_cu=cus)["workspace_bytes"] > \
        dv.lag_plan(*lg.FRAME, 70, *small, lag=3, n_cu=cus)["workspace_bytes"] > 0
    assert dv.lag_plan(*lg.FRAME, 13, *full, n_cu=cus)["workspace_bytes"] == 0
    assert dv.lag16_plan(*lg.FRAME, 70, *small, lag=2, n_cu=cus)["segments"] > 1

    def args(s, n):
        return (s.buf, s.lead, s.total, s.offs, s.W, s.H, n)

    lag_steps = {      # name: (stream, n, lag, stats mask, lead, window, bits)
        "lag a small": (a, 70, 3, 31, 0, small, 8),
        "lag a 13": (a, 13, 1, 8, 0, full, 8),
        "lag a full": (a, 70, 8, 1, 0, full, 8),
        "lag b": (b, 70, 2, 28, 5, (0, 0, 72, 40), 8),
        "lag a pixel": (a, 33, 5, 3, 0, one, 8),
        "lag16 c": (c, 70, 2, 31, 0, small, 16),
    }

    def lag_call(name):
        s, n, lag, mask, lead, win, bits = lag_steps[name]
        return lambda k: (k.project_lag if bits == 8 else k.project_lag16)(*args(s, n), lag, lr.names_of(mask), lead, *win)

    steps = [
        ("lag a small", lag_call("lag a small")),
        ("decode_roi a", lambda k: k.decode_roi(*args(a, 13), *small)),
        ("lag a 13", lag_call("lag a 13")),
        ("project a", lambda k: k.project(*args(a, 70), *small)),
        ("lag a full", lag_call("lag a full")),
        ("pairs b", lambda k: k.project_pairs(*args(b, 70), 8)),
        ("lag b", lag_call("lag b")),
        ("counts a", lambda k: k.project_counts(*args(a, 70), [10, 100, 200], *small)),
        ("lag a pixel", lag_call("lag a pixel")),
        ("lag16 c", lag_call("lag16 c")),
        ("project16 c", lambda k: k.project16(*args(c, 70), *small)),
        ("lag a small", None), ("lag a 13", None), ("project a", None), ("lag b", None), ("lag16 c", None),
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

    # and the lag planes are the reference's
    for name, (s, n, lag, mask, lead, win, bits) in lag_steps.items():
        want = lg.cap(s.images[:n], lag, win, lead, bits)
        lg.compare(alone[name][0][0], want, lr.names_of(mask), name)
    assert np.array_equal(alone["project a"][0][0].sum.cpu().numpy(),
                          sum(im[5:32, 3:44].astype(np.int64) for im in a.images))
