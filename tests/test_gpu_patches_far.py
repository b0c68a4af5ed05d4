"""GPU: the patch decode at stream and output offsets past 2^31 and 2^32 bytes.

The buffers follow tests/far.py's layout rules (a sentinel lead in front of every buffer a kernel is given, a tail
behind it, every offset below 2^33), so a narrowed offset lands inside the test's own allocation: on a decoy frame, on
sentinel bytes or on the wrong patch, and the test fails with wrong values rather than a fault.

decode_patches and decode_patches16 read the six far placements of far.SLOTS, once for each field that crosses 2^32, in
both edge modes; the patches and used origins lie in far.guarded buffers.  Expected: tests/patch_ref.py over the oracle's
decode of every frame; the same call on a near copy of the stream, element for element; rejected entries keep the
sentinel; results rows are the real frames' (a decoy's index would show).  One more case puts the OUTPUT past 2^32
bytes: 13 x 2,400 patches of 505 x 300 bytes, of which counts leaves three per frame live.
"""
import numpy as np
import pytest

import far
import patch_ref as pr
from test_gpu_far_offsets import (assert_rows, assert_same, codec, device_memory, dv, far_and_near,   # noqa: F401
                                  frames_of)
from test_gpu_patches import origins_for
from test_oracle_u16 import o16   # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

S8 = far.SENTINEL
S32 = int(np.array([S8] * 4, np.uint8).view(np.int32)[0])


@pytest.mark.parametrize("bits,W,H,n", [(8, 200, 123, 13), (16, 200, 123, 13)])
def test_patches_far_streams(dv, codec, oracle, o16, bits, W, H, n):   # noqa: F811
    import torch
    fr = frames_of(oracle, o16, W, H, bits)
    rng = np.random.default_rng(W + n + bits)
    fn = codec.decode_patches if bits == 8 else codec.decode_patches16
    pdt, ndt = (torch.uint8, np.uint8) if bits == 8 else (torch.int16, np.uint16)
    sent = S8 if bits == 8 else S8 * 0x0101
    j = 0
    for pw, ph in ((32, 32), (58, 58), (200, 3)):
        org = origins_for(rng, W, H, pw, ph, n)
        K = org.shape[1]
        d_org = torch.from_numpy(org.astype(np.int32)).cuda()
        for straddle, lay in fr.layouts.items():
            mode = (pr.CLAMP, pr.FILL)[j % 2]
            fill = (1 << bits) - 2
            j += 1
            ents = far.entries(n)

            def call(s):
                gp = far.guarded((n, K, ph, pw), pdt)
                gu = far.guarded((n, K, 2), torch.int32)
                _, res = fn(s.buf, s.lead, s.stream_bytes, s.offs, W, H, n, pw, ph, d_org,
                            edge="clamp" if mode == pr.CLAMP else "fill", fill=fill, out=gp.t, used=gu.t)
                codec.sync()
                gp.check(f"patches {bits}-bit {straddle}")
                gu.check(f"used origins {bits}-bit {straddle}")
                return gp.t, gu.t, res

            got, near = far_and_near(lay, ents, call)
            what = f"{bits}-bit patches {W}x{H} {pw}x{ph} mode {mode} {straddle}"
            assert_same(got, near, what)
            refs = fr.refs(lay, ents)
            assert_rows(codec, got[2], refs, what)
            want, want_used, live = pr.expected([img for _, img in refs], W, H, pw, ph, org, None, mode, fill,
                                                untouched=sent, dtype=ndt)
            want_used[~live] = S32
            assert np.array_equal(got[0].cpu().numpy().view(ndt), want), what
            assert np.array_equal(got[1].cpu().numpy(), want_used), what + ": used origins"
            del got, near


def test_patches_far_output(dv, codec, oracle, o16):   # noqa: F811
    """The last frame's patches start past 2^32 bytes of the output, the used origins' index past 2^16 patches."""
    import torch
    W, H, n, pw, ph, K, live = 200, 123, 13, 505, 300, 2400, 3
    assert (n - 1) * K * ph * pw > 1 << 32
    fr = frames_of(oracle, o16, W, H, 8)
    lay = fr.layouts["payload"]
    ents = far.entries(n)
    refs = fr.refs(lay, ents)
    s = far.NearStream(lay, ents)
    rng = np.random.default_rng(3)
    org = np.zeros((n, K, 2), np.int64)
    org[:, :live] = np.stack([rng.integers(-pw, W, (n, live)), rng.integers(-ph, H, (n, live))], -1)
    gp = far.guarded((n, K, ph, pw), torch.uint8)
    gu = far.guarded((n, K, 2), torch.int32)
    counts = torch.full((n,), live, dtype=torch.int32, device="cuda")
    _, res = codec.decode_patches(s.buf, s.lead, s.stream_bytes, s.offs, W, H, n, pw, ph,
                                  torch.from_numpy(org.astype(np.int32)).cuda(), counts=counts, edge="fill", fill=7,
                                  out=gp.t, used=gu.t)
    codec.sync()
    gp.check("patches")
    gu.check("used origins")
    assert_rows(codec, res, refs, "far output")
    for f, (_, img) in enumerate(refs):
        got = gp.t[f, :live].cpu().numpy()
        used = gu.t[f, :live].cpu().numpy()
        if img is None:
            assert (got == S8).all() and (used == S32).all(), f"rejected entry {f} was written"
            continue
        for k in range(live):
            want, _ = pr.patch(img, W, H, pw, ph, org[f, k, 0], org[f, k, 1], pr.FILL, 7)
            assert np.array_equal(got[k], want), (f, k)
        assert np.array_equal(used, org[f, :live]), f
        gp.t[f, :live] = S8
        gu.t[f, :live] = S32
    assert far.all_equal(gp.t.view(-1), S8), "a patch at k >= count was written"
    assert far.all_equal(gu.t.view(-1), S32), "a used origin at k >= count was written"
