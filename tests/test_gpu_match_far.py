"""GPU: the patch match at stream and surface offsets past 2^31 and 2^32 bytes.

The buffers follow tests/far.py's layout rules (a sentinel lead in front of every buffer a kernel is given, a tail
behind it, every offset below 2^33), so a narrowed offset lands inside the test's own allocation: on a decoy frame, on
sentinel bytes or on the wrong tile row, and the test fails with wrong sums rather than a fault.

match_patches and match_patches16 read the six far placements of far.SLOTS, once for each field that crosses 2^32, in
both edge modes; the surfaces and used origins lie in far.guarded buffers.  Expected: tests/match_ref.py over the
oracle's decode of every frame; the same call on a near copy of the stream, element for element; rejected entries keep
the sentinel; results rows are the real frames'.  One more case puts the SURFACE past 2^32 bytes: 13 x 42,000 patches of
33 x 33 entries, of which counts leaves three per frame live, so that the last frames' entries start past 2^31 and 2^32
bytes of prod.
"""
import numpy as np
import pytest

import far
import match_ref as mr
import patch_ref as pr
from test_gpu_far_offsets import (assert_rows, assert_same, codec, device_memory, dv, far_and_near,   # noqa: F401
                                  frames_of)
from test_oracle_u16 import o16   # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

S8 = far.SENTINEL
S32 = int(np.array([S8] * 4, np.uint8).view(np.int32)[0])
S64 = int(np.array([S8] * 8, np.uint8).view(np.int64)[0])


@pytest.mark.parametrize("bits,W,H,n", [(8, 200, 123, 13), (16, 200, 123, 13)])
def test_match_far_streams(dv, codec, oracle, o16, bits, W, H, n):   # noqa: F811
    import torch
    fr = frames_of(oracle, o16, W, H, bits)
    rng = np.random.default_rng(W + n + bits)
    fn = codec.match_patches if bits == 8 else codec.match_patches16
    top = (1 << bits) - 1
    tw, th, S, K = 16, 12, 2, 6
    T = rng.integers(0, top + 1, size=(K, th, tw)).astype(np.uint8 if bits == 8 else np.uint16)
    d_T = torch.from_numpy(T if bits == 8 else T.view(np.int16)).cuda()
    pw, ph = tw + 2 * S, th + 2 * S
    org = np.stack([rng.integers(-pw // 2, W - pw // 2, (n, K)), rng.integers(-ph // 2, H - ph // 2, (n, K))], -1)
    d_org = torch.from_numpy(org.astype(np.int32)).cuda()
    D = 2 * S + 1
    for mode in (pr.CLAMP, pr.FILL):
        for straddle, lay in fr.layouts.items():
            ents = far.entries(n)

            def call(s):
                gs = [far.guarded((n, K, D, D), torch.int64) for _ in range(3)]
                gu = far.guarded((n, K, 2), torch.int32)
                _, res = fn(s.buf, s.lead, s.stream_bytes, s.offs, W, H, n, d_T, S, d_org,
                            edge="clamp" if mode == pr.CLAMP else "fill", fill=top // 3,
                            out=dict(zip(mr.NAMES, (g.t for g in gs))), used=gu.t)
                codec.sync()
                for g, nm in zip(gs, mr.NAMES):
                    g.check(f"{nm} {bits}-bit {straddle}")
                gu.check(f"used origins {bits}-bit {straddle}")
                return gs[0].t, gs[1].t, gs[2].t, gu.t, res

            got, near = far_and_near(lay, ents, call)
            what = f"{bits}-bit match {W}x{H} {tw}x{th} S {S} mode {mode} {straddle}"
            assert_same(got, near, what)
            refs = fr.refs(lay, ents)
            assert_rows(codec, got[4], refs, what)
            assert not all(img is not None for _, img in refs), "no rejected entry: the sentinel is never checked"
            want = mr.expected([img for _, img in refs], W, H, T, S, org, None, mode, top // 3)
            live = want[4]
            for i, nm in enumerate(mr.NAMES):
                w = want[i].copy()
                w[~live] = S64
                assert np.array_equal(got[i].cpu().numpy(), w), f"{what}: {nm}"
            used = want[3].copy()
            used[~live] = S32
            assert np.array_equal(got[3].cpu().numpy(), used), what + ": used origins"
            del got, near


def test_match_far_surface(dv, codec, oracle, o16):   # noqa: F811
    """prod alone, 1 x 1 templates at S = 16 (33 x 33 entries, 8,712 bytes a patch): 13 x 42,000 patches make 4.7 GB,
    frames 6 and up start past 2^31 bytes, frames 12 past 2^32.  The index is (frame * K + patch) * D * D + shift in a
    size_t; a 32-bit product would put the last frames' entries among the first frames'."""
    import torch
    W, H, n, S, K, live = 200, 123, 13, 16, 42_000, 3
    D = 2 * S + 1
    assert 6 * K * D * D * 8 > 1 << 31 and (n - 1) * K * D * D * 8 > 1 << 32
    fr = frames_of(oracle, o16, W, H, 8)
    lay = fr.layouts["payload"]
    ents = far.entries(n)
    refs = fr.refs(lay, ents)
    s = far.NearStream(lay, ents)
    rng = np.random.default_rng(5)
    lorg = np.stack([rng.integers(-D, W, (n, live)), rng.integers(-D, H, (n, live))], -1)
    d_org = torch.zeros((n, K, 2), dtype=torch.int32, device="cuda")
    d_org[:, :live] = torch.from_numpy(lorg.astype(np.int32)).cuda()
    T = np.array([[[3]]], np.uint8)
    gp = far.guarded((n, K, D, D), torch.int64)
    counts = torch.full((n,), live, dtype=torch.int32, device="cuda")
    _, res = codec.match_patches(s.buf, s.lead, s.stream_bytes, s.offs, W, H, n, torch.from_numpy(T).cuda(), S, d_org,
                                 counts=counts, edge="fill", fill=9, stats=("prod",), out=dict(prod=gp.t))
    codec.sync()
    gp.check("prod")
    assert_rows(codec, res, refs, "far surface")
    for f, (_, img) in enumerate(refs):
        got = gp.t[f, :live].cpu().numpy()
        if img is None:
            assert (got == S64).all(), f"rejected entry {f} was written"
            continue
        for k in range(live):
            P, _ = pr.patch(img, W, H, D, D, lorg[f, k, 0], lorg[f, k, 1], pr.FILL, 9)
            assert np.array_equal(got[k], 3 * P.astype(np.int64)), (f, k)
        gp.t[f, :live] = S64
    assert far.all_equal(gp.t.view(-1), S64), "an entry of a patch at k >= count was written"
