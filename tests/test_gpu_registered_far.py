"""GPU: the registered projections at stream offsets past 2^31 and 2^32 bytes.

The buffers follow tests/far.py's layout rules (a sentinel lead in front of every buffer a kernel is given, a tail
behind it, every offset below 2^33), so a narrowed offset lands inside the test's own allocation and the test fails
with wrong values rather than a fault.

project_registered and project_registered16 read the six far placements of far.SLOTS (two of them rejected frames),
once for each field that crosses 2^32, with origins that differ from frame to frame; the planes lie in far.guarded
buffers.  Expected: tests/registered_ref.py over the oracle's decode of every frame; the same call on a near copy of the
stream, element for element; results rows are the real frames'; origins_used rows of the rejected frames keep their
sentinel.
"""
import numpy as np
import pytest

import far
import registered_gpu as rg
import registered_ref as rr
from test_gpu_far_offsets import (assert_rows, assert_same, codec, device_memory, dv, far_and_near,   # noqa: F401
                                  frames_of)
from test_oracle_u16 import o16   # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("bits,W,H,n", [(8, 200, 123, 13), (16, 200, 123, 13)])
def test_registered_projection_far_streams(dv, codec, oracle, o16, bits, W, H, n):   # noqa: F811
    import torch
    fr = frames_of(oracle, o16, W, H, bits)
    fn = rg.call_of(codec, bits)
    mm = torch.uint8 if bits == 8 else torch.int16
    cases = [(W, H, 15), (41, 27, 5), (W - 11, H - 19, 10)]
    for j, (straddle, lay) in enumerate(fr.layouts.items()):
        rw, rh, mask = cases[j % len(cases)]
        names = rr.names_of(mask)
        ents = far.entries(n)
        refs = fr.refs(lay, ents)
        images = [img for _, img in refs]
        assert any(im is None for im in images) and any(im is not None for im in images)
        rng = np.random.default_rng(j + bits)
        origins = np.stack([rng.integers(-3, W - rw + 4, n), rng.integers(-3, H - rh + 4, n)], 1).astype(np.int64)
        org = rg.device_origins(origins)

        def call(s):
            gs = {k: far.guarded((rh, rw), mm if k in ("max", "min") else torch.int64) for k in names}
            count = torch.full((1,), -1, dtype=torch.int64, device="cuda")
            used = torch.full((n, 2), rg.SENT, dtype=torch.int32, device="cuda")
            out = dv.Projection(count=count, **{k: g.t for k, g in gs.items()})
            _, res = fn(s.buf, s.lead, s.stream_bytes, s.offs, W, H, n, rw, rh, org, out=out, origins_used=used)
            codec.sync()
            for k, g in gs.items():
                g.check(f"{k} {bits}-bit {straddle}")
            return tuple(gs[k].t for k in names) + (count, used, res)

        got, near = far_and_near(lay, ents, call)
        what = f"{bits}-bit registered {W}x{H} window {rw}x{rh} mask={mask} {straddle}"
        assert_same(got, near, what)
        assert_rows(codec, got[-1], refs, what)
        want = rr.registered(images, origins, rw, rh, bits)
        for k, t in zip(names, got):
            g = t.cpu().numpy()
            g = g.view(np.uint64) if k in ("sum", "sumsq") else g.view(np.uint16) if bits == 16 else g
            assert np.array_equal(g, want[k]), (what, k)
        assert got[-3].tolist() == [want["count"]], what
        for f, row in enumerate(got[-2].tolist()):
            assert tuple(row) == want["used"].get(f, (rg.SENT, rg.SENT)), (what, f)
        del got, near
