"""CPU: dbde_hip_patch_moments_plan / dbde16_hip_patch_moments_plan (host arithmetic) on hand-derived cases; no device.

The sizes and the edge mode are the patch decoder's: a patch of pw pixels spans at most (pw + 6) / 8 + 1 tiles across
(in CLAMP mode (min(7, W - pw) + pw + 7) / 8), a step takes G = max(1, 64 / that) tile rows.  What differs: ONE workgroup
per patch walks steps_per_patch = ceil(tile rows / G) steps, so the grid is n * K; ph is at most 512 (the sums' 64-bit
bound); the output is 64 bytes a patch.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.fixture(scope="module")
def dv():
    import dbde_video_cpp_amd as m
    if not os.path.exists(m.LIB_PATH):
        m.build()
    return m


# (W, H, n, pw, ph, K, edge) -> max_tiles_x, max_tiles_y, rows_per_workgroup, steps_per_patch
CASES = [
    ((4096, 3072, 10, 32, 32, 8, "clamp"), (5, 5, 12, 1)),
    ((4096, 3072, 10, 57, 57, 8, "clamp"), (8, 8, 8, 1)),
    ((4096, 3072, 10, 58, 58, 8, "clamp"), (9, 9, 7, 2)),
    ((4096, 3072, 10, 505, 3, 8, "fill"), (64, 2, 1, 2)),
    ((4096, 3072, 10, 3, 300, 8, "clamp"), (2, 39, 32, 2)),      # (3 + 14) / 8 = 2; (300 + 14) / 8 = 39
    ((4096, 3072, 10, 3, 512, 8, "fill"), (2, 65, 32, 3)),       # (512 + 14) / 8 = 65 tile rows, 32 a step
    ((4096, 3072, 10, 505, 512, 8, "fill"), (64, 65, 1, 65)),    # the largest patch: 65 steps of one wave
    ((4096, 3072, 10, 1, 1, 1, "fill"), (1, 1, 64, 1)),
    ((36, 40, 3, 32, 32, 2, "clamp"), (5, 5, 12, 1)),            # W - pw = 4: (4 + 32 + 7) / 8 = 5
    ((32, 32, 3, 32, 32, 2, "clamp"), (4, 4, 16, 1)),            # the patch is the frame: tile-aligned
    ((32, 32, 3, 32, 32, 2, "fill"), (5, 5, 12, 1)),             # fill mode: any origin
    ((512, 512, 3, 505, 512, 2, "clamp"), (64, 64, 1, 64)),      # H - ph = 0: 64 tile rows
    ((10, 10, 3, 400, 500, 2, "fill"), (51, 64, 1, 64)),         # larger than the frame, fill mode only
]


@pytest.mark.parametrize("args,want", CASES)
def test_hand_derived_plans(dv, args, want):
    W, H, n, pw, ph, K, edge = args
    for pix, fn, pfn in ((1, dv.patch_moments_plan, dv.patches_plan), (2, dv.patch_moments16_plan, dv.patches16_plan)):
        pl = fn(*args)
        got = (pl["max_tiles_x"], pl["max_tiles_y"], pl["rows_per_workgroup"], pl["steps_per_patch"])
        assert got == want, (args, got)
        assert pl["rows_per_workgroup"] == max(1, 64 // pl["max_tiles_x"])
        assert pl["steps_per_patch"] == -(-pl["max_tiles_y"] // pl["rows_per_workgroup"])
        assert pl["threads"] == 64
        assert pl["grid"] == n * K
        assert pl["moments_bytes"] == n * K * 64
        assert pl["lds_bytes"] == 4096 * pix + 2048
        dec = pfn(*args)   # the patch decoder's plan of the same sizes: the same tiles, its groups are the steps
        assert (dec["max_tiles_x"], dec["max_tiles_y"], dec["rows_per_workgroup"], dec["groups_per_patch"]) == want
        for k in ("chunks_per_frame", "chunk_tiles", "chunk_pieces", "index_split"):
            assert pl[k] == dec[k], k


REJECTED = [
    (4096, 3072, 2, 8, 513, 4, "fill"),      # ph > 512
    (4096, 3072, 2, 8, 513, 4, "clamp"),
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
    (300, 200, 1 << 16, 8, 8, 1 << 15, "clamp"),            # 2^31 patches
    (300, 200, 1 << 15, 58, 58, 1 << 15, "clamp"),          # what decode_patches refuses: 2^30 patches of two groups each
    (16, 8 * 32768 * 512 + 8, 1, 8, 8, 1, "clamp"),         # more than 32768 plain 512-tile chunks
]


@pytest.mark.parametrize("args", REJECTED)
def test_rejections(dv, args):
    for fn in (dv.patch_moments_plan, dv.patch_moments16_plan):
        with pytest.raises(ValueError):
            fn(*args)


def test_accepted_at_the_limits(dv):
    assert dv.patch_moments_plan(4096, 3072, 2, 8, 512, 4, "fill")["steps_per_patch"] == 3      # 65 tile rows, 32 a step
    assert dv.patch_moments_plan(4096, 3072, 2, 8, 512, 4, "clamp")["max_tiles_y"] == 65
    assert dv.patch_moments_plan(300, 200, 2, 505, 8, 4, "fill")["max_tiles_x"] == 64
    assert dv.patch_moments_plan(300, 200, 2, 301, 201, 4, "fill")["max_tiles_x"] == 39        # pw > W is legal in FILL mode
    assert dv.patch_moments_plan(300, 200, 1 << 16, 8, 8, (1 << 15) - 1, "clamp")["grid"] == (1 << 31) - (1 << 16)
    p = dv.patch_moments_plan(300, 200, 0, 8, 8, 4)
    assert p["grid"] == 0 and p["moments_bytes"] == 0
    with pytest.raises(ValueError):
        dv.patch_moments_plan(300, 200, 2, 8, 8, 4, "wrap")


def test_null_plan_and_weight_names(dv):
    L = dv.lib()
    assert L.dbde_hip_patch_moments_plan(300, 200, 2, 8, 8, 4, 0, None) == dv.ERR_ARG
    assert L.dbde16_hip_patch_moments_plan(300, 200, 2, 8, 8, 4, 0, None) == dv.ERR_ARG
    assert [dv.moment_weight_mode(w) for w in ("count", "value", "above", "below")] == [0, 1, 2, 3]
    assert dv.moment_weight_mode(3) == 3
    with pytest.raises(ValueError):
        dv.moment_weight_mode("mass")
