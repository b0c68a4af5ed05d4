"""CPU: dbde_hip_patches_plan / dbde16_hip_patches_plan (host arithmetic) on hand-derived cases; no device.

A patch of pw pixels spans at most (pw + 6) / 8 + 1 tiles across (x mod 8 = 7); a 64-lane workgroup takes
G = max(1, 64 / that) tile rows of one patch, a patch ceil(tile rows / G) workgroups.  In CLAMP mode x mod 8 only reaches
min(7, W - pw), as in dbde_hip_roi_plan.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.fixture(scope="module")
def dv():
    import dbde_video_cpp_amd as m
    if not os.path.exists(m.LIB_PATH):
        m.build()
    return m


# (W, H, n, pw, ph, K, edge) -> max_tiles_x, max_tiles_y, rows_per_workgroup, groups_per_patch
CASES = [
    ((4096, 3072, 10, 32, 32, 8, "clamp"), (5, 5, 12, 1)),
    ((4096, 3072, 10, 57, 57, 8, "clamp"), (8, 8, 8, 1)),
    ((4096, 3072, 10, 58, 58, 8, "clamp"), (9, 9, 7, 2)),
    ((4096, 3072, 10, 505, 3, 8, "fill"), (64, 2, 1, 2)),
    ((4096, 3072, 10, 3, 300, 8, "clamp"), (2, 39, 32, 2)),     # (3 + 14) / 8 = 2; (300 + 14) / 8 = 39
    ((4096, 3072, 10, 1, 1, 1, "fill"), (1, 1, 64, 1)),
    ((36, 40, 3, 32, 32, 2, "clamp"), (5, 5, 12, 1)),           # W - pw = 4: (4 + 32 + 7) / 8 = 5; H - ph = 8
    ((33, 32, 3, 32, 32, 2, "clamp"), (5, 4, 12, 1)),           # W - pw = 1: (1 + 32 + 7) / 8 = 5; H - ph = 0: 4 rows
    ((32, 32, 3, 32, 32, 2, "clamp"), (4, 4, 16, 1)),           # the patch is the frame: tile-aligned
    ((32, 32, 3, 32, 32, 2, "fill"), (5, 5, 12, 1)),            # fill mode: any origin
    ((64, 64, 3, 57, 64, 2, "clamp"), (8, 8, 8, 1)),            # W - pw = 7: the general case
    ((64, 64, 3, 58, 64, 2, "clamp"), (8, 8, 8, 1)),            # W - pw = 6: (6 + 58 + 7) / 8 = 8, not 9
    ((10, 10, 3, 400, 500, 2, "fill"), (51, 64, 1, 64)),        # larger than the frame, fill mode only
]


@pytest.mark.parametrize("args,want", CASES)
def test_hand_derived_plans(dv, args, want):
    W, H, n, pw, ph, K, edge = args
    for pix, fn in ((1, dv.patches_plan), (2, dv.patches16_plan)):
        pl = fn(*args)
        got = (pl["max_tiles_x"], pl["max_tiles_y"], pl["rows_per_workgroup"], pl["groups_per_patch"])
        assert got == want, (args, got)
        assert pl["threads"] == 64
        assert pl["grid"] == n * K * want[3]
        assert pl["out_bytes"] == n * K * ph * pw * pix
        assert pl["lds_bytes"] == 4096 * pix + 2048


REJECTED = [
    (300, 200, 2, 506, 8, 4, "fill"),        # 65 tiles across
    (4096, 200, 2, 506, 8, 4, "clamp"),
    (300, 200, 2, 8, 8, 0, "clamp"),         # no patch
    (300, 200, 2, 8, 8, -1, "fill"),
    (300, 200, 2, 0, 8, 4, "clamp"),
    (300, 200, 2, 8, 0, 4, "fill"),
    (300, 200, 2, 301, 8, 4, "clamp"),       # pw > W in CLAMP mode
    (300, 200, 2, 8, 201, 4, "clamp"),
    (300, 200, 2, 8, 8, 4, 2),               # unknown edge mode
    (300, 200, 2, 8, 8, 4, -1),
    (300, 200, -1, 8, 8, 4, "clamp"),
    (0, 200, 2, 8, 8, 4, "fill"),
    (300, 200, 1 << 16, 8, 8, 1 << 15, "clamp"),            # 2^31 workgroups
    (300, 200, 1 << 15, 58, 58, 1 << 15, "clamp"),          # 2^30 patches of two workgroups each
    (16, 8 * 32768 * 512 + 8, 1, 8, 8, 1, "clamp"),         # more than 32768 plain 512-tile chunks
]


@pytest.mark.parametrize("args", REJECTED)
def test_rejections(dv, args):
    for fn in (dv.patches_plan, dv.patches16_plan):
        with pytest.raises(ValueError):
            fn(*args)


def test_accepted_at_the_limits(dv):
    assert dv.patches_plan(300, 200, 2, 505, 8, 4, "fill")["max_tiles_x"] == 64
    assert dv.patches_plan(300, 200, 2, 301, 201, 4, "fill")["max_tiles_x"] == 39     # pw > W is legal in FILL mode
    assert dv.patches_plan(300, 200, 1 << 16, 8, 8, (1 << 15) - 1, "clamp")["grid"] == (1 << 31) - (1 << 16)
    assert dv.patches_plan(300, 200, 0, 8, 8, 4)["grid"] == 0
    with pytest.raises(ValueError):
        dv.patches_plan(300, 200, 2, 8, 8, 4, "wrap")


@pytest.mark.parametrize("W,H,n", [(4096, 3072, 1024), (4096, 3072, 3), (8200, 17, 5), (513, 17, 40), (16, 262152, 2),
                                   (1, 1, 1)])
def test_index_geometry_is_roi_plans(dv, W, H, n):
    for pfn, rfn in ((dv.patches_plan, dv.roi_plan), (dv.patches16_plan, dv.roi16_plan)):
        p, r = pfn(W, H, n, 1, 1, 3, "fill"), rfn(W, H, n, 0, 0, 1, 1)
        for k in ("chunks_per_frame", "chunk_tiles", "chunk_pieces", "index_split"):
            assert p[k] == r[k], (k, p[k], r[k])


def test_origins_from_centres(dv):
    import torch
    c = np.array([[[10.49, 10.5], [-0.5, -0.51], [0.0, 31.9]]])
    want = np.array([[[10 - 16, 11 - 4], [0 - 16, -1 - 4], [0 - 16, 32 - 4]]], np.int32)
    assert np.array_equal(dv.origins_from_centres(c, 32, 9), want)
    got = dv.origins_from_centres(torch.from_numpy(c), 32, 9)
    assert got.dtype == torch.int32 and np.array_equal(got.numpy(), want)
    assert np.array_equal(dv.origins_from_centres(np.array([[[7, 9]]]), 5, 4), [[[5, 7]]])
    assert np.array_equal(dv.origins_from_centres(np.array([[[1e12, -1e12]]]), 5, 4), [[[2 ** 31 - 1, -2 ** 31]]])
    with pytest.raises(ValueError):
        dv.origins_from_centres(np.zeros((3, 2)), 4, 4)
