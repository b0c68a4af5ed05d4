"""GPU: the weighted projections at stream offsets past 2^31 and 2^32 bytes, and with planes past 2^32 bytes.

The buffers follow tests/far.py's layout rules (a sentinel lead in front of every buffer a kernel is given, a tail
behind it, every offset below 2^33), so a narrowed offset lands inside the test's own allocation and the test fails
with wrong values rather than a fault.

1. project_weighted and project_weighted16 read the six far placements of far.SLOTS (two of them rejected frames, whose
   weights are NaN), once for each field that crosses 2^32; the planes lie in a far.guarded buffer.  Expected:
   tests/wproject_ref.py's chain over the oracle's decode of every frame, bit for bit; the same call on a near copy of
   the stream, element for element; results rows are the real frames'.
2. Planes past 2^32 bytes: 8 planes of 4096 x 38400 F32 (5.03 GB; plane 6 holds byte 2^32, plane 7 lies wholly behind
   it) from 3 frames.  With small integer weights every partial sum of the chain is an exact integer below 2^24, so the
   defined value is the integer sum and every element is compared with torch's int64 arithmetic on the decoded images;
   with arbitrary weights, rectangles at the first element, across byte 2^32 and at the last element are compared with
   the reference chain bit for bit.
"""
import numpy as np
import pytest

import far
import wproject_gpu as wg
import wproject_ref as wr
from test_gpu_far_offsets import (assert_rows, assert_same, codec, device_memory, dv, far_and_near,   # noqa: F401
                                  frames_of)
from test_gpu_project import Batch
from test_oracle_u16 import o16   # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

G32 = far.G32


@pytest.mark.parametrize("bits,W,H,n", [(8, 200, 123, 13), (16, 200, 123, 13)])
def test_weighted_projection_far_streams(dv, codec, oracle, o16, bits, W, H, n):   # noqa: F811
    import torch
    fr = frames_of(oracle, o16, W, H, bits)
    fn = codec.project_weighted if bits == 8 else codec.project_weighted16
    plan = dv.wproject_plan if bits == 8 else dv.wproject16_plan
    cus = wg.cus_of(codec)
    rng = np.random.default_rng(bits + n)
    cases = [((0, 0, W, H), 3), ((3, 5, 41, 27), 8), ((8, 16, W - 11, H - 19), 1)]
    for j, (straddle, lay) in enumerate(fr.layouts.items()):
        (x, y, rw, rh), R = cases[j % len(cases)]
        ents = far.entries(n)
        refs = fr.refs(lay, ents)
        images = [img for _, img in refs]
        assert any(im is None for im in images) and any(im is not None for im in images)
        w = wg.family(rng, "normal", R, n)
        w[:, [f for f in range(n) if images[f] is None]] = np.nan
        wd = wg.strided(w)

        def call(s):
            g = far.guarded((R, rh, rw), torch.float32)
            cnt = torch.full((1,), -1, dtype=torch.int64, device="cuda")
            _, res = fn(s.buf, s.lead, s.stream_bytes, s.offs, W, H, n, wd, x, y, rw, rh,
                        out=dv.WeightedProjection(g.t, cnt))
            codec.sync()
            g.check(f"planes {bits}-bit {straddle}")
            return g.t.view(torch.int32), cnt, res

        got, near = far_and_near(lay, ents, call)
        what = f"{bits}-bit weighted {W}x{H} R={R} window {(x, y, rw, rh)} {straddle}"
        assert_same(got, near, what)
        assert_rows(codec, got[2], refs, what)
        p = plan(W, H, n, x, y, rw, rh, regressors=R, n_cu=cus)
        want, count = wr.wproject(images, w, x, y, rw, rh, segments=p["segments"], fps=p["frames_per_segment"])
        wg.assert_bits(got[0].view(torch.float32), want, what)
        assert int(got[1].item()) == count
        del got, near


def test_planes_past_4gib(dv, codec):   # noqa: F811
    import torch
    W, H, n, R = 4096, 38400, 3, 8
    P = W * H
    assert (R - 1) * P * 4 > G32 > (R - 2) * P * 4
    b = Batch(codec, "mixed", W, H, n)
    planes = far.guarded((R, H, W), torch.float32)
    out = dv.WeightedProjection(planes.t, torch.zeros(1, dtype=torch.int64, device="cuda"))
    assert dv.wproject_plan(W, H, n, regressors=R, n_cu=wg.cus_of(codec))["segments"] == 1

    # small integer weights: the chain is exact, the planes are the integer sums
    wi = np.array([[1, 1, 1], [1, -2, 3], [0, 5, -5], [-7, 0, 2], [8, 8, 8], [3, -1, -1], [-4, 6, 1], [2, -3, 9]], np.float32)
    assert np.abs(wi).sum(1).max() * 255 < 2 ** 24
    codec.project_weighted(b.buf, b.lead, b.total, b.offs, W, H, n, torch.from_numpy(wi).cuda(), out=out)
    codec.sync()
    planes.check("integer weights")
    assert int(out.count.item()) == n
    for r in range(R):
        want = sum(int(wi[r, f]) * b.images[f].to(torch.int32) for f in range(n))
        assert torch.equal(planes.t[r], want.to(torch.float32)), f"plane {r}"
        del want

    # arbitrary weights: rectangles at the first element, across byte 2^32 (plane 6) and at the last element
    w = wg.family(np.random.default_rng(1), "normal", R, n)
    planes.t.view(torch.int32).fill_(0x7FC5A5A5)
    codec.project_weighted(b.buf, b.lead, b.total, b.offs, W, H, n, wg.strided(w), out=out)
    codec.sync()
    planes.check("arbitrary weights")
    row = (G32 - 6 * P * 4) // 4 // W
    assert 0 < row < H - 8
    for r, y, x, rh, rw in [(0, 0, 0, 9, 70), (6, row - 3, 0, 7, W), (6, row - 1, W - 50, 3, 50), (7, H - 9, W - 70, 9, 70),
                            (7, 0, 0, 5, 64)]:
        images = list(b.images[:, y:y + rh, x:x + rw].cpu().numpy())
        want, _ = wr.wproject(images, w[r:r + 1], 0, 0, rw, rh)
        wg.assert_bits(planes.t[r, y:y + rh, x:x + rw], want[0], f"plane {r} rows {y}.. columns {x}..")
