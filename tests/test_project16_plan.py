"""CPU: dbde16_hip_project_plan -- the tile window, index geometry, launch and workspace of a DBDE16 temporal
projection, and the argument checks dbde16_hip_project shares with it.  Pure host arithmetic; no GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALL = ("max", "min", "sum", "sumsq")
U32_BOUND = 65536   # frames one workgroup sums per pixel in U32: 65,536 * 65,535 < 2^32
TILES_PER_WG = 16   # one lane per half tile row: 16 lanes per tile, 256 lanes


@pytest.fixture(scope="module")
def dv():
    import dbde_video_cpp_amd as m
    if not os.path.exists(m.LIB_PATH):
        m.build()
    return m


CASES = [
    # (W, H, n, x, y, rw, rh)
    (4096, 3072, 128, 0, 0, 4096, 3072),
    (4096, 3072, 16, 1003, 701, 256, 256),
    (4096, 3072, 1024, 0, 0, 512, 512),
    (1024, 768, 2048, 0, 0, 1024, 768),
    (1921, 1081, 7, 1920, 1080, 1, 1),
    (1921, 1081, 7, 1, 1, 1920, 1080),
    (200, 123, 5, 3, 0, 1, 123),
    (8200, 9, 4, 4090, 0, 20, 9),
    (4104, 16, 3, 0, 0, 4104, 16),
    (8, 262152, 2, 0, 0, 8, 262152),
    (64, 64, 100000, 0, 0, 64, 64),
    (8, 8, 70000, 0, 0, 8, 8),
    (16, 16, 70000, 3, 5, 9, 10),
    (10, 10, 33, 1, 2, 9, 7),
    (9, 9, 0, 0, 0, 9, 9),
    (1, 1, 1, 0, 0, 1, 1),
]


@pytest.mark.parametrize("W,H,n,x,y,rw,rh", CASES)
def test_window_and_index_geometry_equal_the_roi16_plan(dv, W, H, n, x, y, rw, rh):
    p = dv.project16_plan(W, H, n, x, y, rw, rh, ALL, n_cu=256)
    r = dv.roi16_plan(W, H, n, x, y, rw, rh)
    for k in ("tile_x", "tile_y", "tiles_x", "tiles_y", "chunks_per_frame", "chunk_tiles", "chunk_pieces",
              "index_split"):
        assert p[k] == r[k], (k, p[k], r[k])


@pytest.mark.parametrize("W,H,n,x,y,rw,rh", CASES)
@pytest.mark.parametrize("n_cu", [1, 32, 256])
def test_plan_invariants(dv, W, H, n, x, y, rw, rh, n_cu):
    p = dv.project16_plan(W, H, n, x, y, rw, rh, ALL, n_cu=n_cu)
    assert p["threads"] == 256
    assert p["pieces_x"] == (p["tiles_x"] + TILES_PER_WG - 1) // TILES_PER_WG
    assert p["grid"] == p["pieces_x"] * p["tiles_y"] * p["segments"]
    assert p["segments"] >= 1
    assert p["segments"] * p["frames_per_segment"] >= n
    assert (p["segments"] - 1) * p["frames_per_segment"] < max(n, 1)   # no empty segment
    assert p["frames_per_segment"] <= p["max_frames_per_segment"] == U32_BOUND
    assert U32_BOUND * 65535 < 2 ** 32
    if p["segments"] == 1:
        assert p["workspace_bytes"] == 0 and p["combine_grid"] == 0
    else:
        assert p["workspace_bytes"] >= p["segments"] * rw * rh * (2 + 2 + 4 + 8)
        assert p["combine_grid"] == (rw * rh + 255) // 256


@pytest.mark.parametrize("W,H,n,x,y,rw,rh", CASES)
def test_segment_rule_is_the_8bit_one(dv, W, H, n, x, y, rw, rh):
    """The same rule on the 16-bit launch: segments follow from the workgroups of one segment, as for DBDE."""
    p16 = dv.project16_plan(W, H, n, x, y, rw, rh, n_cu=256)
    p8 = dv.project_plan(W, H, n, x, y, rw, rh, n_cu=256)
    if p16["pieces_x"] == p8["pieces_x"]:   # windows of at most 16 tiles across: the same launch shape
        assert (p16["segments"], p16["frames_per_segment"]) == (p8["segments"], p8["frames_per_segment"])
    else:
        assert p16["segments"] <= p8["segments"]


def test_plan_examples_pinned(dv):
    p = dv.project16_plan(4096, 3072, 128)
    assert (p["pieces_x"], p["tiles_y"], p["segments"], p["frames_per_segment"], p["grid"]) == (32, 384, 1, 128, 12288)
    assert (p["threads"], p["workspace_bytes"], p["combine_grid"]) == (256, 0, 0)
    p = dv.project16_plan(1024, 768, 2048)
    assert (p["pieces_x"], p["tiles_y"], p["segments"], p["frames_per_segment"], p["grid"]) == (8, 96, 2, 1024, 1536)
    assert p["workspace_bytes"] == 2 * 1024 * 768 * (2 + 2 + 4 + 8) and p["combine_grid"] == 3072
    p = dv.project16_plan(64, 64, 100000)
    assert (p["pieces_x"], p["tiles_y"], p["segments"], p["frames_per_segment"], p["grid"]) == (1, 8, 128, 782, 1024)
    assert p["workspace_bytes"] == 128 * 4096 * (2 + 2 + 4 + 8)
    p = dv.project16_plan(4096, 3072, 16, 1003, 701, 256, 256)
    assert (p["tile_x"], p["tiles_x"], p["pieces_x"], p["tiles_y"]) == (125, 33, 3, 33)
    p = dv.project16_plan(9, 9, 0, stats="max")
    assert (p["segments"], p["frames_per_segment"], p["grid"], p["workspace_bytes"]) == (1, 0, 2, 0)


def test_workspace_grows_with_the_statistics(dv):
    """U16 max / min, U32 sum and U64 sumsq partials: 2, 2, 4 and 8 bytes per pixel per segment."""
    args = (64, 64, 100000)
    sizes = {s: dv.project16_plan(*args, stats=s)["workspace_bytes"] for s in
             [("max",), ("min",), ("sum",), ("sumsq",), ("max", "min"), ("sum", "sumsq"), ALL]}
    per = dv.project16_plan(*args)["segments"] * 64 * 64
    assert sizes[("max",)] == sizes[("min",)] == 2 * per
    assert sizes[("sum",)] == 4 * per
    assert sizes[("sumsq",)] == 8 * per
    assert sizes[("max", "min")] == 2 * sizes[("max",)]
    assert sizes[ALL] == sizes[("max", "min")] + sizes[("sum",)] + sizes[("sumsq",)]
    grids = {dv.project16_plan(*args, stats=s)["grid"] for s in sizes}
    assert len(grids) == 1


REJECTED = [
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
    ((40000, 40000, 1, 0, 0, 8, 8), ALL),      # too large for the index
    ((8, 8, 2 ** 30, 0, 0, 8, 8), ALL),        # too many index chunks in one call
    ((4096, 3072, 2 ** 22, 0, 0, 4096, 3072), ALL),   # too many workgroups in one call
]


@pytest.mark.parametrize("args,stats", REJECTED)
def test_plan_rejects_what_the_8bit_plan_rejects(dv, args, stats):
    with pytest.raises(ValueError):
        dv.project_plan(*args, stats=stats)
    with pytest.raises(ValueError):
        dv.project16_plan(*args, stats=stats)


@pytest.mark.parametrize("args,stats", REJECTED)
def test_entry_point_rejects_without_a_device(dv, args, stats):
    """dbde16_hip_project: a NULL context, and the plan's rejections, are DBDE_HIP_ERR_ARG before any device work."""
    L = dv.lib()
    W, H, n, x, y, rw, rh = args
    assert L.dbde16_hip_project(None, None, 0, None, W, H, n, x, y, rw, rh, 0, None, None, None, None, None,
                                None) == dv.ERR_ARG


def test_null_context(dv):
    L = dv.lib()
    assert L.dbde16_hip_project(None, None, 0, None, 64, 64, 1, 0, 0, 8, 8, 0, None, None, None, None, None,
                                None) == dv.ERR_ARG


@pytest.mark.parametrize("args,stats,want", [
    ((4096, 3072, 1024, 0, 0, 4096, 3072), ALL,
     dict(tile_x=0, tile_y=0, tiles_x=512, tiles_y=384, chunks_per_frame=384, chunk_tiles=512, chunk_pieces=1,
          index_split=1, threads=256, pieces_x=16, segments=1, frames_per_segment=1024, max_frames_per_segment=65536,
          grid=6144, combine_grid=0, workspace_bytes=0)),
    ((64, 64, 100000, 0, 0, 64, 64), ALL,
     dict(tile_x=0, tile_y=0, tiles_x=8, tiles_y=8, chunks_per_frame=8, chunk_tiles=8, chunk_pieces=1, index_split=1,
          threads=256, pieces_x=1, segments=128, frames_per_segment=782, max_frames_per_segment=65536, grid=1024,
          combine_grid=16, workspace_bytes=128 * 4096 * (1 + 1 + 4 + 4))),
    ((200, 123, 5, 3, 0, 1, 123), ("max", "sumsq"),
     dict(tile_x=0, tile_y=0, tiles_x=1, tiles_y=16, chunks_per_frame=16, chunk_tiles=25, chunk_pieces=1,
          index_split=4, threads=256, pieces_x=1, segments=1, frames_per_segment=5, max_frames_per_segment=65536,
          grid=16, combine_grid=0, workspace_bytes=0)),
])
def test_8bit_plan_unchanged(dv, args, stats, want):
    """dbde_hip_project_plan reports what it reported before the 16-bit projection shared its segment rule."""
    assert dv.project_plan(*args, stats=stats, n_cu=256) == want
