"""GPU: patch decode of DBDE16 streams -- dbde16_hip_decode_patches (Codec.decode_patches16).

As tests/test_gpu_patches.py with U16 pixels: expected values are tests/patch_ref.py's over the images
dbde16_hip_decode_frames writes for the same frames (for crafted frames: crafted.decode_frame's), compared exactly.
Also the chain of calls on one shared context, which the 8- and 16-bit calls share.
"""
import numpy as np
import pytest

import patch_ref as pr
from test_gpu_mask16 import Batch16
from test_gpu_patches import check_patches, origins_for, run_patches, sizes_for
from test_gpu_project16 import Crafted16
from test_gpu_roi import Batch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dv():
    import dbde_video_cpp_amd as m
    return m


@pytest.fixture(scope="module")
def codec(dv):
    c = dv.Codec(0)
    assert c.arch.startswith("gfx950")
    yield c
    c.close()


@pytest.mark.parametrize("W,H,n", [(4096, 24, 2), (8200, 17, 2), (513, 17, 3), (1921, 25, 3), (72, 72, 4), (10, 10, 3),
                                   (1, 1, 3)])
def test_patches16_match_patch_ref(codec, W, H, n):
    import torch
    rng = np.random.default_rng(W * 31 + H)
    batches = [Batch16(codec, kind, W, H, n) for kind in ("mixed", "full")]
    for j, (pw, ph) in enumerate(sizes_for(W, H)):
        b = batches[j % 2]
        frames = list(b.images)
        org = origins_for(rng, W, H, pw, ph, n)
        K = org.shape[1]
        counts = [None, [K] * n, [0] * n, [K + 5, 1, K // 2, 0][:n], None][j % 5]
        res = check_patches(codec, b, frames, W, H, pw, ph, org, counts, pr.FILL, fill=(0xBEEF, 0, 0xFFFF)[j % 3],
                            out_misalign=j % 8, bits=16, what="fill")
        assert torch.equal(res, b.results)
        if pw <= W and ph <= H:
            check_patches(codec, b, frames, W, H, pw, ph, org, counts, pr.CLAMP, out_misalign=(j + 3) % 8, bits=16,
                          what="clamp")


def test_clamp_patches16_equal_decode_roi16(codec):
    import torch
    W, H, n = 1921, 97, 3
    b = Batch16(codec, "full", W, H, n)
    rng = np.random.default_rng(13)
    for pw, ph in ((32, 32), (58, 58), (505, 3)):
        org = origins_for(rng, W, H, pw, ph, n)
        got, _, _ = run_patches(codec, b.buf, b.lead, b.total, b.offs, W, H, n, pw, ph, org, bits=16)
        for k in range(0, org.shape[1], 7):
            d_o = torch.from_numpy(org[:, k].astype(np.int32)).cuda()
            win, _ = codec.decode_roi16(b.buf, b.lead, b.total, b.offs, W, H, n, 0, 0, pw, ph, origins=d_o)
            codec.sync()
            assert np.array_equal(win.cpu().numpy().view(np.uint16), got[:, k]), (pw, ph, k)


@pytest.mark.parametrize("W,H,n,how", [(64, 48, 40, "concat"), (200, 123, 23, "residues"), (1921, 17, 9, "slots")])
def test_crafted16_and_rejected_frames(codec, W, H, n, how):
    """Every depth 0..16 at every payload byte alignment, wrapping minima, broken frames between good ones."""
    import torch
    rng = np.random.default_rng(W * 7919 + H)
    s = Crafted16(rng, W, H, n, how)
    assert any(im is None for im in s.images) and any(im is not None for im in s.images)
    _, want_res = codec.decode_frames16(s.buf, s.lead, s.total, s.offs, W, H, n)
    for pw, ph in ((32, min(H, 32)), (9, 9), (58, min(H, 58))):
        org = origins_for(rng, W, H, pw, ph, n)
        for m in (pr.CLAMP, pr.FILL):
            res = check_patches(codec, s, s.images, W, H, pw, ph, org, None, m, fill=0xC3C4, out_misalign=pw % 8, bits=16,
                                what=f"crafted16 {how}")
            assert torch.equal(res, want_res)


def test_chain_on_one_context(codec, oracle):
    """decode_frames -> decode_patches -> decode_roi (other geometry) -> decode_patches16 -> decode_patches (fewer
    frames, in the split-index range): the calls share chunk_off, frame_ok and the split-index counters."""
    import torch
    rng = np.random.default_rng(77)
    a = Batch(codec, oracle, "mixed", 513, 97, 5, first=4)        # 13 tile rows: the index is split
    c = Batch(codec, oracle, "noise8", 200, 123, 3, first=1)
    b16 = Batch16(codec, "mixed", 1921, 25, 2)
    for rep in range(2):
        imgs, _ = codec.decode_frames(a.buf, a.lead, a.total, a.offs, a.W, a.H, a.n)
        codec.sync()
        assert all(np.array_equal(imgs[f].cpu().numpy(), a.full[f]) for f in range(a.n))
        check_patches(codec, a, a.full, a.W, a.H, 32, 32, origins_for(rng, a.W, a.H, 32, 32, a.n), None, pr.FILL, fill=3)
        win, _ = codec.decode_roi(c.buf, c.lead, c.total, c.offs, c.W, c.H, c.n, 5, 7, 100, 50)
        codec.sync()
        assert all(np.array_equal(win[f].cpu().numpy(), c.full[f][7:57, 5:105]) for f in range(c.n))
        check_patches(codec, b16, list(b16.images), 1921, 25, 58, 9, origins_for(rng, 1921, 25, 58, 9, 2), [40, 3], pr.CLAMP,
                      bits=16)
        check_patches(codec, a, a.full[:2], a.W, a.H, 57, 57, origins_for(rng, a.W, a.H, 57, 57, 2), [1, 60], pr.CLAMP)
