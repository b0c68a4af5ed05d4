"""GPU: the lag projections at stream offsets past 2^31 and 2^32 bytes.

The buffers follow tests/far.py's layout rules (a sentinel lead in front of every buffer a kernel is given, a tail
behind it, every offset below 2^33), so a narrowed offset lands inside the test's own allocation and the test fails
with wrong values rather than a fault.

project_lag and project_lag16 read the six far placements of far.SLOTS (two of them rejected frames), once for each
field that crosses 2^32; the planes lie in far.guarded buffers.  Expected: tests/lag_ref.py over the oracle's decode of
every frame; the same call on a near copy of the stream, element for element; results rows are the real frames'.

There is no planes-past-4-GiB part: each statistic has its own pointer, so a plane that holds byte 2^32 would need
512 M pixels; the plane offset row * rw + x is 64-bit by construction.
"""
import numpy as np
import pytest

import far
import lag_ref as lr
from test_gpu_far_offsets import (assert_rows, assert_same, codec, device_memory, dv, far_and_near,   # noqa: F401
                                  frames_of)
from test_oracle_u16 import o16   # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("bits,W,H,n", [(8, 200, 123, 13), (16, 200, 123, 13)])
def test_lag_projection_far_streams(dv, codec, oracle, o16, bits, W, H, n):   # noqa: F811
    import torch
    fr = frames_of(oracle, o16, W, H, bits)
    fn = codec.project_lag if bits == 8 else codec.project_lag16
    mx = torch.uint8 if bits == 8 else torch.int16
    cases = [((0, 0, W, H), 1, 31, 0), ((3, 5, 41, 27), 3, 11, 2), ((8, 16, W - 11, H - 19), 2, 20, 0)]
    for j, (straddle, lay) in enumerate(fr.layouts.items()):
        (x, y, rw, rh), lag, mask, lead = cases[j % len(cases)]
        names = lr.names_of(mask)
        ents = far.entries(n)
        refs = fr.refs(lay, ents)
        images = [img for _, img in refs]
        assert any(im is None for im in images) and any(im is not None for im in images)

        def call(s):
            gs = {k: far.guarded((rh, rw), torch.int64 if k != "maxdiff" else mx) for k in names}
            sc = torch.full((2,), -1, dtype=torch.int64, device="cuda")
            out = dv.LagProjection(pairs=sc[0:1], count=sc[1:2], lag=lag, **{k: g.t for k, g in gs.items()})
            _, res = fn(s.buf, s.lead, s.stream_bytes, s.offs, W, H, n, lag, names, lead, x, y, rw, rh, out=out)
            codec.sync()
            for k, g in gs.items():
                g.check(f"{k} {bits}-bit {straddle}")
            return tuple(gs[k].t for k in names) + (sc, res)

        got, near = far_and_near(lay, ents, call)
        what = f"{bits}-bit lag {W}x{H} lag={lag} mask={mask} lead={lead} window {(x, y, rw, rh)} {straddle}"
        assert_same(got, near, what)
        assert_rows(codec, got[-1], refs, what)
        want = lr.lag(images, lag, x, y, rw, rh, lead=lead, bits=bits)
        assert want["pairs"] > 0, what
        for k, t in zip(names, got):
            g = t.cpu().numpy()
            g = g.view(np.uint64) if k != "maxdiff" else g.view(np.uint16) if bits == 16 else g
            assert np.array_equal(g, want[k]), (what, k)
        assert got[-2].tolist() == [want["pairs"], want["count"]], what
        del got, near
