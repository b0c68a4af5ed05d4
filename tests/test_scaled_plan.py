"""CPU: dbde_hip_scaled_plan / dbde16_hip_scaled_plan (pure host arithmetic; no device): the argument rules of the
scaled float decode, its geometry (the window decoder's), its launch, LDS and output bytes."""
import pytest

import dbde_video_cpp_amd as dv

PLANS = [(dv.scaled_plan, dv.roi_plan, 1), (dv.scaled16_plan, dv.roi16_plan, 2)]
ELEM = {dv.OUT_F32: 4, dv.OUT_F16: 2, dv.OUT_BF16: 2}
SHARED = ("tile_x", "tile_y", "tiles_x", "tiles_y", "max_tiles_x", "max_tiles_y", "chunks_per_frame", "chunk_tiles",
          "chunk_pieces", "index_split", "threads", "pieces_x", "grid", "grid_origins")


@pytest.fixture(scope="module", autouse=True)
def built():
    import os
    if not os.path.exists(dv.LIB_PATH):
        dv.build()


@pytest.mark.parametrize("plan,roi,pix", PLANS)
def test_argument_rules(plan, roi, pix):
    W, H = 64, 48
    for kw in (dict(x=1, rw=64), dict(y=1, rh=48), dict(x=-1, rw=8), dict(y=-1, rh=8), dict(x=64, rw=1),
               dict(rw=0), dict(rh=0), dict(rw=65), dict(rh=49), dict(rw=-3)):
        with pytest.raises(ValueError):
            plan(W, H, 2, **kw)
    for bad in (3, -1, 7, 256):
        with pytest.raises(ValueError):
            plan(W, H, 2, dtype=bad)
    with pytest.raises(ValueError):
        plan(W, H, -1)
    with pytest.raises(ValueError):
        plan(0, H, 1)
    z = plan(W, H, 0)
    assert z["grid"] == 0 and z["out_bytes"] == 0 and z["threads"] == 64


def test_output_types():
    import torch
    for t, es in ((torch.float32, 4), (torch.float16, 2), (torch.bfloat16, 2)):
        assert dv.scaled_plan(64, 48, 3, dtype=t)["out_bytes"] == 3 * 64 * 48 * es
    assert dv.scaled_plan(64, 48, 3, dtype=dv.OUT_BF16)["out_bytes"] == 3 * 64 * 48 * 2
    for bad in (torch.float64, torch.uint8, 5, -1):
        with pytest.raises(ValueError):
            dv.scaled_plan(64, 48, 3, dtype=bad)


@pytest.mark.parametrize("plan,roi,pix", PLANS)
@pytest.mark.parametrize("W,H,n,win", [(64, 48, 3, (0, 0, 64, 48)), (64, 48, 3, (5, 3, 41, 30)),
                                       (4096, 3072, 2, (0, 0, 4096, 3072)), (4096, 3072, 7, (1000, 696, 256, 256)),
                                       (4200, 24, 3, (0, 0, 4200, 24)), (4200, 24, 3, (4090, 1, 110, 23)),
                                       (1921, 1081, 2, (275, 217, 959, 537)), (1, 1, 5, (0, 0, 1, 1))])
def test_geometry_is_the_window_decoders_and_bytes(plan, roi, pix, W, H, n, win):
    x, y, rw, rh = win
    want = roi(W, H, n, x, y, rw, rh)
    for t, es in ELEM.items():
        got = plan(W, H, n, x, y, rw, rh, dtype=t)
        assert {k: got[k] for k in SHARED} == {k: want[k] for k in SHARED}
        assert got["elem_bytes"] == es and got["out_bytes"] == n * rw * rh * es


def test_grid_and_lds():
    # 64 x 48: 8 x 6 tiles, one wave per window tile row
    for plan, lds in ((dv.scaled_plan, 64 * 64 + 64 + 8), (dv.scaled16_plan, 64 * 128 + 32 + 8)):
        p = plan(64, 48, 5)
        assert (p["threads"], p["pieces_x"], p["grid"], p["lds_bytes"]) == (64, 1, 5 * 6, lds)
    # 4096 x 3072: 512 x 384 tiles; pieces of 256 tiles (DBDE16: 128)
    p = dv.scaled_plan(4096, 3072, 2)
    assert (p["threads"], p["pieces_x"], p["grid"], p["lds_bytes"]) == (256, 2, 2 * 384 * 2, 256 * 64 + 64 + 32)
    assert p["out_bytes"] == 2 * 4096 * 3072 * 4
    p = dv.scaled16_plan(4096, 3072, 2, dtype=dv.OUT_F16)
    assert (p["threads"], p["pieces_x"], p["grid"], p["lds_bytes"]) == (128, 4, 2 * 384 * 4, 128 * 128 + 32 + 16)
    # 4200 wide: 525 tiles across, more than one 512-tile index chunk per tile row
    p = dv.scaled_plan(4200, 24, 3)
    assert (p["tiles_x"], p["chunk_pieces"], p["chunk_tiles"], p["chunks_per_frame"]) == (525, 2, 512, 6)
    assert (p["threads"], p["pieces_x"], p["grid"], p["lds_bytes"]) == (256, 3, 3 * 3 * 3, 16480)
    p = dv.scaled16_plan(4200, 24, 3)
    assert (p["threads"], p["pieces_x"], p["grid"], p["lds_bytes"]) == (128, 5, 3 * 3 * 5, 16432)
    # a moving window needs one more tile column and row than the window at a multiple of 8
    p = dv.scaled_plan(4096, 3072, 4, 1000, 696, 256, 256)
    assert (p["tiles_x"], p["max_tiles_x"], p["max_tiles_y"], p["grid"], p["grid_origins"]) == (32, 33, 33, 4 * 32, 4 * 33)
    # past 2^32 output bytes at 86 frames of 4096 x 3072 in F32
    assert dv.scaled_plan(4096, 3072, 86)["out_bytes"] == 86 * 4096 * 3072 * 4 > 1 << 32
