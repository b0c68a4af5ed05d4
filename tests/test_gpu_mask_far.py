"""GPU: the threshold mask decode at stream offsets past 2^31 and 2^32 bytes.

The buffers follow tests/far.py's layout rules (a sentinel lead in front of every buffer a kernel is given, a tail
behind it, every offset below 2^33), so a narrowed offset lands inside the test's own allocation: on a decoy frame, on
sentinel bytes or on the wrong word, and the test fails with wrong values rather than a fault.

decode_mask and decode_mask16 read the six far placements of far.SLOTS, once for each field that crosses 2^32, with
scalar thresholds (the decided-tile form) and with both maps, fixed and per-frame origins; the words, counts and boxes
lie in far.guarded buffers.  Expected: tests/mask_ref.py over the oracle's decode of every frame; the same call on a
near copy of the stream, word for word; rejected entries keep the sentinel words, count 0 and the empty box; results
rows are the real frames' (a decoy's index would show).
"""
import numpy as np
import pytest

import far
import mask_ref as mr
from test_gpu_far_offsets import (assert_rows, assert_same, codec, device_memory, dv, far_and_near,   # noqa: F401
                                  frames_of)
from test_oracle_u16 import o16   # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

S8 = far.SENTINEL


@pytest.mark.parametrize("bits,W,H,n", [(8, 200, 123, 13), (16, 200, 123, 13)])
def test_mask_far(dv, codec, oracle, o16, bits, W, H, n):   # noqa: F811
    import torch
    fr = frames_of(oracle, o16, W, H, bits)
    rng = np.random.default_rng(W + n + bits)
    fn = codec.decode_mask if bits == 8 else codec.decode_mask16
    top = (1 << bits) - 1
    dt = np.uint8 if bits == 8 else np.uint16
    lo_map = rng.integers(0, top // 2, (H, W)).astype(dt)
    hi_map = (lo_map.astype(np.int64) + rng.integers(0, top // 2, (H, W))).astype(dt)
    dev = lambda a: torch.from_numpy(a.view(np.int16) if bits == 16 else a).cuda()   # noqa: E731
    d_lo, d_hi = dev(lo_map), dev(hi_map)
    k = 0
    for (x, y, rw, rh), per_frame in (((W // 3, H // 5, W // 2, H // 3), True), ((0, 0, W, H), False),
                                      ((W - 139, 1, 130, H - 2), False)):
        org = None
        if per_frame:
            org = np.stack([rng.integers(-3, W + 3, n), rng.integers(-3, H + 3, n)], 1).astype(np.int32)
        words = (rw + 63) // 64
        for straddle, lay in fr.layouts.items():
            maps = k % 2 == 1
            outside = k % 3 == 0
            k += 1
            lo, hi = (lo_map, hi_map) if maps else (top // 4, top // 2)
            ents = far.entries(n)

            def call(s):
                gm = far.guarded((n, rh, words), torch.int64)
                gc = far.guarded((n,), torch.int32)
                gb = far.guarded((n, 4), torch.int32)
                m = dv.Mask(gm.t, gc.t, gb.t)
                _, res = fn(s.buf, s.lead, s.stream_bytes, s.offs, W, H, n, x, y, rw, rh, lo=d_lo if maps else lo,
                            hi=d_hi if maps else hi, outside=outside,
                            origins=None if org is None else torch.from_numpy(org).cuda(), mask=m)
                codec.sync()
                for g in (gm, gc, gb):
                    g.check(f"mask {bits}-bit {straddle}")
                return gm.t, gc.t, gb.t, res

            got, near = far_and_near(lay, ents, call)
            what = f"{bits}-bit mask {W}x{H} window {(x, y, rw, rh)} per-frame {per_frame} maps {maps} {straddle}"
            assert_same(got, near, what)
            refs = fr.refs(lay, ents)
            assert_rows(codec, got[3], refs, what)
            gw = got[0].cpu().numpy().view(np.uint64)
            gc_, gb_ = got[1].cpu().numpy().view(np.uint32), got[2].cpu().numpy()
            sent = np.uint64(S8 * 0x0101010101010101)
            for f, (_, img) in enumerate(refs):
                if img is None:
                    assert (gw[f] == sent).all(), f"{what}: rejected entry {f}'s words were written"
                    assert gc_[f] == 0 and (gb_[f] == [rw, rh, -1, -1]).all(), f"{what}: rejected entry {f}"
                    continue
                ww, wc, wb = mr.expected(img[None], x, y, rw, rh, lo, hi, mr.OUTSIDE if outside else mr.INSIDE,
                                         None if org is None else org[f:f + 1])
                assert np.array_equal(gw[f], ww[0]), f"{what}: entry {f} words"
                assert gc_[f] == wc[0] and (gb_[f] == wb[0]).all(), f"{what}: entry {f} count / box"
            del got, near
