"""CPU: dbde_hip_project_plan -- the tile window, index geometry, launch and workspace of a temporal projection, and
the argument checks dbde_hip_project shares with it.  Pure host arithmetic; no GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALL = ("max", "min", "sum", "sumsq")
U32_BOUND = 65536   # frames one workgroup may sum in U32: 65,536 * 255^2 < 2^32


@pytest.fixture(scope="module")
def dv():
    import dbde_video_cpp_amd as m
    if not os.path.exists(m.LIB_PATH):
        m.build()
    return m


def expect_window(W, H, x, y, rw, rh):
    """The window and index geometry worked out independently from the format: 8x8 tiles, index chunks at every tile
    row (512-tile pieces of wider rows), plain 512-tile chunks when that would exceed 32,768 chunks."""
    w, h = (W + 7) // 8, (H + 7) // 8
    tx0, ty0 = x // 8, y // 8
    ntx, nty = (x + rw - 1) // 8 + 1 - tx0, (y + rh - 1) // 8 + 1 - ty0
    pieces = (w + 511) // 512
    if h * pieces <= 32768:
        cpf, ct, cp = h * pieces, (w if pieces == 1 else 512), pieces
    else:
        cpf, ct, cp = (w * h + 511) // 512, 512, (1 if w == 512 else 0)
    return dict(tile_x=tx0, tile_y=ty0, tiles_x=ntx, tiles_y=nty, chunks_per_frame=cpf, chunk_tiles=ct,
                chunk_pieces=cp)


CASES = [
    # (W, H, n, x, y, rw, rh)
    (4096, 3072, 1024, 0, 0, 4096, 3072),
    (4096, 3072, 16, 1003, 701, 256, 256),
    (4096, 3072, 1024, 0, 0, 512, 512),
    (1921, 1081, 7, 1920, 1080, 1, 1),
    (1921, 1081, 7, 1, 1, 1920, 1080),
    (200, 123, 5, 3, 0, 1, 123),            # one column
    (8200, 9, 4, 4090, 0, 20, 9),            # across a 512-tile index piece
    (4200, 24, 3, 0, 0, 4200, 24),           # a row wider than 512 tiles
    (8, 262152, 2, 0, 0, 8, 262152),         # 32,769 tile rows: plain 512-tile chunks
    (64, 64, 100000, 0, 0, 64, 64),
    (8, 8, 70000, 0, 0, 8, 8),
    (16, 16, 70000, 0, 0, 16, 16),
    (9, 9, 0, 0, 0, 9, 9),
    (1, 1, 1, 0, 0, 1, 1),
]


@pytest.mark.parametrize("W,H,n,x,y,rw,rh", CASES)
def test_plan_geometry_and_invariants(dv, W, H, n, x, y, rw, rh):
    p = dv.project_plan(W, H, n, x, y, rw, rh, ALL, n_cu=256)
    for k, v in expect_window(W, H, x, y, rw, rh).items():
        assert p[k] == v, (k, p[k], v)
    # the index split follows dbde_hip_decode_frames (and dbde_hip_roi_plan)
    assert p["index_split"] == dv.roi_plan(W, H, n, x, y, rw, rh)["index_split"]
    tiles_per_wg = p["threads"] // 8   # one lane per tile row
    assert p["pieces_x"] == (p["tiles_x"] + tiles_per_wg - 1) // tiles_per_wg
    assert p["segments"] >= 1
    assert p["segments"] * p["frames_per_segment"] >= n
    assert (p["segments"] - 1) * p["frames_per_segment"] < max(n, 1)   # no empty segment
    assert p["frames_per_segment"] <= p["max_frames_per_segment"] == U32_BOUND
    assert U32_BOUND * 255 ** 2 < 2 ** 32
    assert p["grid"] == p["pieces_x"] * p["tiles_y"] * p["segments"]
    if p["segments"] == 1:
        assert p["workspace_bytes"] == 0 and p["combine_grid"] == 0
    else:
        assert p["workspace_bytes"] >= p["segments"] * rw * rh * (1 + 1 + 4 + 4)
        assert p["combine_grid"] == (rw * rh + 255) // 256


@pytest.mark.parametrize("W,H,n", [(4096, 3072, 1024), (64, 64, 100000)])
def test_large_batches_fill_256_cus(dv, W, H, n):
    p = dv.project_plan(W, H, n, n_cu=256)
    assert p["grid"] >= 256, p


def test_segments_respect_the_u32_bound(dv):
    """A batch longer than 65,536 frames is cut into segments even when the window alone fills the device."""
    p = dv.project_plan(4096, 3072, 200000, n_cu=256)
    assert p["segments"] >= 4 and p["frames_per_segment"] <= U32_BOUND
    p = dv.project_plan(8, 8, 70000, n_cu=1)
    assert p["segments"] >= 2 and p["frames_per_segment"] <= U32_BOUND


def test_workspace_grows_with_the_statistics(dv):
    args = (64, 64, 100000)
    sizes = {s: dv.project_plan(*args, stats=s)["workspace_bytes"] for s in
             [("max",), ("min",), ("sum",), ("sumsq",), ("max", "min"), ("sum", "sumsq"), ALL]}
    assert sizes[("max",)] == sizes[("min",)] > 0
    assert sizes[("sum",)] == sizes[("sumsq",)] > sizes[("max",)]
    assert sizes[("max", "min")] == 2 * sizes[("max",)]
    assert sizes[("sum", "sumsq")] == 2 * sizes[("sum",)]
    assert sizes[ALL] == sizes[("max", "min")] + sizes[("sum", "sumsq")]
    # the launch itself does not depend on the statistics
    grids = {dv.project_plan(*args, stats=s)["grid"] for s in sizes}
    assert len(grids) == 1


def test_plan_examples_pinned(dv):
    """A few plans spelled out, so that a change of the launch shape is a visible diff."""
    p = dv.project_plan(4096, 3072, 1024)
    assert (p["pieces_x"], p["tiles_y"], p["segments"], p["frames_per_segment"], p["grid"]) == (16, 384, 1, 1024, 6144)
    assert (p["threads"], p["workspace_bytes"], p["combine_grid"]) == (256, 0, 0)
    p = dv.project_plan(64, 64, 100000)
    assert (p["pieces_x"], p["tiles_y"], p["segments"], p["frames_per_segment"], p["grid"]) == (1, 8, 128, 782, 1024)
    p = dv.project_plan(9, 9, 0, stats="max")
    assert (p["segments"], p["frames_per_segment"], p["grid"], p["workspace_bytes"]) == (1, 0, 2, 0)


@pytest.mark.parametrize("args,stats", [
    ((64, 64, 1, 0, 0, 0, 8), ALL),            # rw = 0
    ((64, 64, 1, 0, 0, 8, 0), ALL),            # rh = 0
    ((64, 64, 1, 0, 0, 65, 8), ALL),           # rw > W
    ((64, 64, 1, 0, 0, 8, 65), ALL),           # rh > H
    ((64, 64, 1, -1, 0, 8, 8), ALL),           # origin outside the frame
    ((64, 64, 1, 0, -8, 8, 8), ALL),
    ((64, 64, 1, 57, 0, 8, 8), ALL),           # x + rw > W
    ((64, 64, 1, 0, 60, 8, 8), ALL),           # y + rh > H
    ((64, 64, 1, 2 ** 31 - 1, 0, 8, 8), ALL),  # origins whose end overflows an int
    ((64, 64, -1, 0, 0, 8, 8), ALL),           # n < 0
    ((0, 64, 1, 0, 0, 1, 1), ALL),             # bad frame
    ((64, 64, 1, 0, 0, 8, 8), 0),              # no statistic
    ((64, 64, 1, 0, 0, 8, 8), 16),             # an unknown one
    ((40000, 40000, 1, 0, 0, 8, 8), ALL),      # too large for the index (more than 32,768 chunks of 512 tiles)
    ((8, 8, 2 ** 30, 0, 0, 8, 8), ALL),        # too many index chunks in one call
    ((4096, 3072, 2 ** 22, 0, 0, 4096, 3072), ALL),   # too many workgroups in one call
])
def test_plan_rejects(dv, args, stats):
    with pytest.raises(ValueError):
        dv.project_plan(*args, stats=stats)


def test_unknown_statistic_name(dv):
    with pytest.raises(ValueError):
        dv.project_plan(64, 64, 1, stats=("max", "median"))


def test_project_argument_errors_without_a_device(dv):
    """dbde_hip_project with a null context is DBDE_HIP_ERR_ARG before anything touches a device."""
    L = dv.lib()
    assert L.dbde_hip_project(None, None, 0, None, 64, 64, 1, 0, 0, 8, 8, 0, None, None, None, None, None,
                              None) == dv.ERR_ARG
