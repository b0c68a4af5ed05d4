"""GPU: the patch moments at stream offsets past 2^31 and 2^32 bytes.

The buffers follow tests/far.py's layout rules (a sentinel lead in front of every buffer a kernel is given, a tail
behind it, every offset below 2^33), so a narrowed offset lands inside the test's own allocation: on a decoy frame, on
sentinel bytes or on the wrong tile row, and the test fails with wrong sums rather than a fault.

patch_moments and patch_moments16 read the six far placements of far.SLOTS, once for each field that crosses 2^32, in
both edge modes and with two patch sizes (32 x 32, and 24 x 300 -- more than 256 rows, which only the fill mode takes
on a frame of 123); the moments, boxes and used origins lie in far.guarded buffers.  Expected: tests/moments_ref.py
over the oracle's decode of every frame; the same call on a near copy of the stream, element for element; rejected
entries keep the sentinel; results rows are the real frames' (a decoy's index would show).  One more case puts the
OUTPUT past 2^32 bytes, which takes more than 2^26 patches and so more than 2^32 work-items: the moments and, beside
them, the patch decode (1 x 1 patches, so that the output stays small) in launches of that size.
"""
import numpy as np
import pytest

import far
import moments_ref as mr
import patch_ref as pr
from test_gpu_far_offsets import (assert_rows, assert_same, codec, device_memory, dv, far_and_near,   # noqa: F401
                                  frames_of)
from test_gpu_patches import origins_for
from test_oracle_u16 import o16   # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

S8 = far.SENTINEL
S32 = int(np.array([S8] * 4, np.uint8).view(np.int32)[0])
S64 = int(np.array([S8] * 8, np.uint8).view(np.int64)[0])


def sentinel_where_dead(want, box, used, live):
    """moments_ref's expectation as int64 / int32 arrays, the far buffers' sentinel where the call writes nothing."""
    want = np.array(want.tolist(), dtype=np.int64).reshape(live.shape + (8,))
    box, used = box.astype(np.int32), used.astype(np.int32)
    want[~live], box[~live], used[~live] = S64, S32, S32
    return want, box, used


@pytest.mark.parametrize("bits,W,H,n", [(8, 200, 123, 13), (16, 200, 123, 13)])
def test_moments_far_streams(dv, codec, oracle, o16, bits, W, H, n):   # noqa: F811
    import torch
    fr = frames_of(oracle, o16, W, H, bits)
    rng = np.random.default_rng(W + n + bits)
    fn = codec.patch_moments if bits == 8 else codec.patch_moments16
    top = (1 << bits) - 1
    j = 0
    for pw, ph, modes in ((32, 32, (pr.CLAMP, pr.FILL)), (24, 300, (pr.FILL,))):
        assert all(m == pr.FILL for m in modes) or (pw <= W and ph <= H)
        org = origins_for(rng, W, H, pw, ph, n)[:, :24]   # (shuffled per frame: the frames together still hold every kind)
        K = org.shape[1]
        d_org = torch.from_numpy(org.astype(np.int32)).cuda()
        for mode in modes:
            for straddle, lay in fr.layouts.items():
                weight = j % 4
                lo, hi = ((top // 8, top - top // 16), (0, top), (top // 3, top // 2))[j % 3]
                j += 1
                ents = far.entries(n)

                def call(s):
                    gm = far.guarded((n, K, 8), torch.int64)
                    gb = far.guarded((n, K, 4), torch.int32)
                    gu = far.guarded((n, K, 2), torch.int32)
                    _, res = fn(s.buf, s.lead, s.stream_bytes, s.offs, W, H, n, pw, ph, d_org, lo, hi,
                                weight=mr.WEIGHTS[weight], edge="clamp" if mode == pr.CLAMP else "fill", out=gm.t, bbox=gb.t,
                                used=gu.t)
                    codec.sync()
                    gm.check(f"moments {bits}-bit {straddle}")
                    gb.check(f"boxes {bits}-bit {straddle}")
                    gu.check(f"used origins {bits}-bit {straddle}")
                    return gm.t, gb.t, gu.t, res

                got, near = far_and_near(lay, ents, call)
                what = (f"{bits}-bit moments {W}x{H} {pw}x{ph} mode {mode} band [{lo}, {hi}] weight {mr.WEIGHTS[weight]} "
                        f"{straddle}")
                assert_same(got, near, what)
                refs = fr.refs(lay, ents)
                assert_rows(codec, got[3], refs, what)
                want, want_box, want_used = sentinel_where_dead(
                    *mr.expected([img for _, img in refs], W, H, pw, ph, org, None, mode, lo, hi, weight))
                assert not all(img is not None for _, img in refs), "no rejected entry: the sentinel is never checked"
                assert np.array_equal(got[0].cpu().numpy(), want), what
                assert np.array_equal(got[1].cpu().numpy(), want_box), what + ": boxes"
                assert np.array_equal(got[2].cpu().numpy(), want_used), what + ": used origins"
                del got, near


def test_moments_far_output(dv, codec, oracle, o16):   # noqa: F811
    """The last frame's moments start past 2^32 bytes of the output: 13 x 5,600,000 patches of which counts leaves three
    per frame live (one workgroup per patch, dead ones included: 72,800,000 workgroups).

    Measured in one run on an MI355X: 1.94 s, against 0.03 s of test_patches_far_output (the dead workgroups are not
    what costs: the same grid of the patch decode below takes 0.04 s; the rest is 31 GB of guarded buffers, three leads
    of 2^33 bytes among them).  That is far more than twice the other test, and as a test of the index expressions
    8u * pi, 4u * pi and 2u * pi (pi a size_t) alone it would not have been kept.  It stays for what it found: 2^26
    workgroups of 64 lanes are 2^32 work-items, more than one launch takes, and the call returned DBDE_HIP_OK with the
    moments of frame 3 onwards never written.  launch_patch_moments now cuts such a grid into several launches; this is
    the only test of the moments whose grid is large enough to need more than one."""
    import torch
    W, H, n, pw, ph, K, live = 200, 123, 13, 32, 32, 5_600_000, 3
    assert (n - 1) * K * 8 * 8 > 1 << 32
    fr = frames_of(oracle, o16, W, H, 8)
    lay = fr.layouts["payload"]
    ents = far.entries(n)
    refs = fr.refs(lay, ents)
    s = far.NearStream(lay, ents)
    rng = np.random.default_rng(5)
    lorg = np.stack([rng.integers(-pw, W, (n, live)), rng.integers(-ph, H, (n, live))], -1)
    d_org = torch.zeros((n, K, 2), dtype=torch.int32, device="cuda")
    d_org[:, :live] = torch.from_numpy(lorg.astype(np.int32)).cuda()
    gm = far.guarded((n, K, 8), torch.int64)
    gb = far.guarded((n, K, 4), torch.int32)
    gu = far.guarded((n, K, 2), torch.int32)
    counts = torch.full((n,), live, dtype=torch.int32, device="cuda")
    lo, hi = 40, 230
    _, res = codec.patch_moments(s.buf, s.lead, s.stream_bytes, s.offs, W, H, n, pw, ph, d_org, lo, hi, weight="above",
                                 counts=counts, edge="fill", out=gm.t, bbox=gb.t, used=gu.t)
    codec.sync()
    gm.check("moments")
    gb.check("boxes")
    gu.check("used origins")
    assert_rows(codec, res, refs, "far output")
    for f, (_, img) in enumerate(refs):
        got = gm.t[f, :live].cpu().numpy()
        box = gb.t[f, :live].cpu().numpy()
        used = gu.t[f, :live].cpu().numpy()
        if img is None:
            assert (got == S64).all() and (box == S32).all() and (used == S32).all(), f"rejected entry {f} was written"
            continue
        for k in range(live):
            want, want_box, _ = mr.moments(img, W, H, pw, ph, lorg[f, k, 0], lorg[f, k, 1], pr.FILL, lo, hi, mr.ABOVE)
            assert got[k].tolist() == want and tuple(box[k].tolist()) == want_box, (f, k)
        assert np.array_equal(used, lorg[f]), f
        gm.t[f, :live] = S64
        gb.t[f, :live] = S32
        gu.t[f, :live] = S32
    assert far.all_equal(gm.t.view(-1), S64), "the moments of a patch at k >= count were written"
    assert far.all_equal(gb.t.view(-1), S32), "the box of a patch at k >= count was written"
    assert far.all_equal(gu.t.view(-1), S32), "a used origin at k >= count was written"


def test_patches_grid_past_2_26_workgroups(dv, codec, oracle, o16):   # noqa: F811
    """decode_patches launches its workgroups the same way: the same 13 x 5,600,000 patches, of 1 x 1 pixel, three per
    frame live.  Before launch_decode_patches cut the grid, a launch of 2^26 workgroups or more had the same defect as
    the moments' (found by reading, after test_moments_far_output had failed)."""
    import torch
    W, H, n, K, live = 200, 123, 13, 5_600_000, 3
    assert dv.patches_plan(W, H, n, 1, 1, K, "fill")["grid"] == n * K > 1 << 26
    fr = frames_of(oracle, o16, W, H, 8)
    lay = fr.layouts["payload"]
    ents = far.entries(n)
    refs = fr.refs(lay, ents)
    s = far.NearStream(lay, ents)
    rng = np.random.default_rng(7)
    lorg = np.stack([rng.integers(0, W, (n, live)), rng.integers(0, H, (n, live))], -1)
    d_org = torch.zeros((n, K, 2), dtype=torch.int32, device="cuda")
    d_org[:, :live] = torch.from_numpy(lorg.astype(np.int32)).cuda()
    gp = far.guarded((n, K, 1, 1), torch.uint8)
    gu = far.guarded((n, K, 2), torch.int32)
    counts = torch.full((n,), live, dtype=torch.int32, device="cuda")
    _, res = codec.decode_patches(s.buf, s.lead, s.stream_bytes, s.offs, W, H, n, 1, 1, d_org, counts=counts, edge="fill",
                                  fill=7, out=gp.t, used=gu.t)
    codec.sync()
    gp.check("patches")
    gu.check("used origins")
    assert_rows(codec, res, refs, "large grid")
    for f, (_, img) in enumerate(refs):
        got = gp.t[f, :live].cpu().numpy().reshape(live)
        used = gu.t[f, :live].cpu().numpy()
        if img is None:
            assert (got == S8).all() and (used == S32).all(), f"rejected entry {f} was written"
            continue
        assert got.tolist() == [int(img[y, x]) for x, y in lorg[f]], f
        assert np.array_equal(used, lorg[f]), f
        gp.t[f, :live] = S8
        gu.t[f, :live] = S32
    assert far.all_equal(gp.t.view(-1), S8), "a patch at k >= count was written"
    assert far.all_equal(gu.t.view(-1), S32), "a used origin at k >= count was written"
