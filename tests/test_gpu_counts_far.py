"""GPU: the count projections at stream offsets past 2^31 and 2^32 bytes, and with planes past 2^32 bytes.

The buffers follow tests/far.py's layout rules (a sentinel lead in front of every buffer a kernel is given, a tail
behind it, every offset below 2^33), so a narrowed offset lands inside the test's own allocation and the test fails
with wrong values rather than a fault.

1. project_counts and project_counts16 read the six far placements of far.SLOTS (two of them rejected frames), once for
   each field that crosses 2^32; the planes lie in a far.guarded buffer.  Expected: tests/counts_ref.py over the
   oracle's decode of every frame; the same call on a near copy of the stream, element for element; results rows are
   the real frames'.
2. Planes past 2^32 bytes: 8 U32 planes of 4096 x 38400 (5.03 GB; plane 6 holds byte 2^32, plane 7 lies wholly behind
   it) from 3 frames with scalar thresholds.  Rectangles at the first element, across byte 2^32 and at the last element
   are compared with the reference; every plane's total is compared with torch's count on the decoded images.
"""
import numpy as np
import pytest

import counts_gpu as cg
import counts_ref as cref
import far
from test_gpu_far_offsets import (assert_rows, assert_same, codec, device_memory, dv, far_and_near,   # noqa: F401
                                  frames_of)
from test_gpu_project import Batch
from test_oracle_u16 import o16   # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

G32 = far.G32


@pytest.mark.parametrize("bits,W,H,n", [(8, 200, 123, 13), (16, 200, 123, 13)])
def test_count_projection_far_streams(dv, codec, oracle, o16, bits, W, H, n):   # noqa: F811
    import torch
    fr = frames_of(oracle, o16, W, H, bits)
    fn = codec.project_counts if bits == 8 else codec.project_counts16
    rng = np.random.default_rng(bits + n)
    cases = [((0, 0, W, H), 3, True), ((3, 5, 41, 27), 8, False), ((8, 16, W - 11, H - 19), 1, True)]
    for j, (straddle, lay) in enumerate(fr.layouts.items()):
        (x, y, rw, rh), K, maps = cases[j % len(cases)]
        ents = far.entries(n)
        refs = fr.refs(lay, ents)
        images = [img for _, img in refs]
        assert any(im is None for im in images) and any(im is not None for im in images)
        thr = cg.draw(rng, images, (x, y, rw, rh), K, bits, maps)
        td = cg.device(thr)

        def call(s):
            g = far.guarded((K, rh, rw), torch.int32)
            cnt = torch.full((1,), -1, dtype=torch.int64, device="cuda")
            _, res = fn(s.buf, s.lead, s.stream_bytes, s.offs, W, H, n, td, x, y, rw, rh,
                        out=dv.CountProjection(g.t, cnt))
            codec.sync()
            g.check(f"planes {bits}-bit {straddle}")
            return g.t, cnt, res

        got, near = far_and_near(lay, ents, call)
        what = f"{bits}-bit counts {W}x{H} K={K} window {(x, y, rw, rh)} {straddle}"
        assert_same(got, near, what)
        assert_rows(codec, got[2], refs, what)
        want, count = cref.counts(images, thr, x, y, rw, rh)
        assert np.array_equal(got[0].cpu().numpy().view(np.uint32), want), what
        assert int(got[1].item()) == count
        del got, near


def test_planes_past_4gib(dv, codec):   # noqa: F811
    import torch
    W, H, n, K = 4096, 38400, 3, 8
    P = W * H
    assert (K - 1) * P * 4 > G32 > (K - 2) * P * 4
    b = Batch(codec, "mixed", W, H, n)
    planes = far.guarded((K, H, W), torch.int32)
    out = dv.CountProjection(planes.t, torch.zeros(1, dtype=torch.int64, device="cuda"))
    assert dv.counts_plan(W, H, n, levels=K, n_cu=torch.cuda.get_device_properties(0).multi_processor_count)["segments"] == 1
    thr = np.array([16, 40, 77, 100, 128, 160, 200, 250], np.uint8)
    codec.project_counts(b.buf, b.lead, b.total, b.offs, W, H, n, cg.device(thr), out=out)
    codec.sync()
    planes.check("scalar thresholds")
    assert int(out.count.item()) == n
    for k in range(K):      # every plane's total, and its spread: some pixel strictly between 0 and n
        want = sum(int((b.images[f] <= int(thr[k])).sum()) for f in range(n))
        assert int(planes.t[k].sum(dtype=torch.int64)) == want, f"plane {k}"
        assert bool(((planes.t[k] > 0) & (planes.t[k] < n)).any()), f"plane {k}"
    row = (G32 - 6 * P * 4) // 4 // W
    assert 0 < row < H - 8
    for k, y, x, rh, rw in [(0, 0, 0, 9, 70), (6, row - 3, 0, 7, W), (6, row - 1, W - 50, 3, 50), (7, H - 9, W - 70, 9, 70),
                            (7, 0, 0, 5, 64)]:
        images = list(b.images[:, y:y + rh, x:x + rw].cpu().numpy())
        want, _ = cref.counts(images, thr[k:k + 1], 0, 0, rw, rh)
        got = planes.t[k, y:y + rh, x:x + rw].cpu().numpy().view(np.uint32)
        assert np.array_equal(got, want[0]), f"plane {k} rows {y}.. columns {x}.."
