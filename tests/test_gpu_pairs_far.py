"""GPU: the pair projections at stream offsets past 2^31 and 2^32 bytes, and with planes past 2^32 bytes.

The buffers follow tests/far.py's layout rules (a sentinel lead in front of every buffer a kernel is given, a tail
behind it, every offset below 2^33), so a narrowed offset lands inside the test's own allocation and the test fails
with wrong values rather than a fault.

1. project_pairs and project_pairs16 read the six far placements of far.SLOTS (two of them rejected frames), once for
   each field that crosses 2^32; the planes lie in a far.guarded buffer.  Expected: tests/pairs_ref.py over the oracle's
   decode of every frame; the same call on a near copy of the stream, element for element; results rows are the real
   frames'.
2. Planes past 2^32 bytes: 4 U64 planes of 4096 x 38400 (5.03 GB; plane 3 holds byte 2^32) from 3 frames.  Rectangles at
   the first element, across byte 2^32 and at the last element are compared with the reference.
"""
import numpy as np
import pytest

import far
import pairs_ref as pref
from test_gpu_far_offsets import (assert_rows, assert_same, codec, device_memory, dv, far_and_near,   # noqa: F401
                                  frames_of)
from test_gpu_project import Batch
from test_oracle_u16 import o16   # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

G32 = far.G32


@pytest.mark.parametrize("bits,W,H,n", [(8, 200, 123, 13), (16, 200, 123, 13)])
def test_pair_projection_far_streams(dv, codec, oracle, o16, bits, W, H, n):   # noqa: F811
    import torch
    fr = frames_of(oracle, o16, W, H, bits)
    fn = codec.project_pairs if bits == 8 else codec.project_pairs16
    cases = [((0, 0, W, H), 15), ((3, 5, 41, 27), 10), ((8, 16, W - 11, H - 19), 3)]
    for j, (straddle, lay) in enumerate(fr.layouts.items()):
        (x, y, rw, rh), mask = cases[j % len(cases)]
        offsets = pref.offsets_of(mask)
        ents = far.entries(n)
        refs = fr.refs(lay, ents)
        images = [img for _, img in refs]
        assert any(im is None for im in images) and any(im is not None for im in images)

        def call(s):
            g = far.guarded((len(offsets), rh, rw), torch.int64)
            cnt = torch.full((1,), -1, dtype=torch.int64, device="cuda")
            _, res = fn(s.buf, s.lead, s.stream_bytes, s.offs, W, H, n, offsets, x, y, rw, rh,
                        out=dv.PairProjection(g.t, cnt, offsets))
            codec.sync()
            g.check(f"planes {bits}-bit {straddle}")
            return g.t, cnt, res

        got, near = far_and_near(lay, ents, call)
        what = f"{bits}-bit pairs {W}x{H} mask={mask} window {(x, y, rw, rh)} {straddle}"
        assert_same(got, near, what)
        assert_rows(codec, got[2], refs, what)
        want, count = pref.pairs(images, mask, x, y, rw, rh)
        assert np.array_equal(got[0].cpu().numpy().view(np.uint64), want), what
        assert int(got[1].item()) == count
        del got, near


def test_planes_past_4gib(dv, codec):   # noqa: F811
    import torch
    W, H, n = 4096, 38400, 3
    P = W * H
    assert 4 * P * 8 > G32 > 3 * P * 8
    b = Batch(codec, "mixed", W, H, n)
    planes = far.guarded((4, H, W), torch.int64)
    out = dv.PairProjection(planes.t, torch.zeros(1, dtype=torch.int64, device="cuda"), dv.PAIR_OFFSETS)
    assert dv.pairs_plan(W, H, n, n_cu=torch.cuda.get_device_properties(0).multi_processor_count)["segments"] == 1
    codec.project_pairs(b.buf, b.lead, b.total, b.offs, W, H, n, 8, out=out)
    codec.sync()
    planes.check("four planes")
    assert int(out.count.item()) == n
    row = (G32 - 3 * P * 8) // 8 // W
    assert 0 < row < H - 8
    # (plane, y, x, rh, rw): each rectangle's reference is computed on the rectangle grown by one pixel where the frame
    # has one, so that the partners at its edges are the frame's
    for k, y, x, rh, rw in [(0, 0, 0, 9, 70), (3, row - 3, 0, 7, W), (3, row - 1, W - 50, 3, 50), (3, H - 9, W - 70, 9, 70),
                            (1, H - 5, 0, 5, 64), (2, 250, 200, 20, 300)]:
        ya, yb, xa, xb = max(y - 1, 0), min(y + rh + 1, H), max(x - 1, 0), min(x + rw + 1, W)
        images = list(b.images[:, ya:yb, xa:xb].cpu().numpy())
        want, _ = pref.pairs(images, 1 << k, 0, 0, xb - xa, yb - ya)
        got = planes.t[k, y:y + rh, x:x + rw].cpu().numpy().view(np.uint64)
        assert np.array_equal(got, want[0][y - ya:y - ya + rh, x - xa:x - xa + rw]), f"plane {k} rows {y}.. columns {x}.."
        assert got.any()
