"""CPU: dbde_hip_trace_plan / dbde16_hip_trace_plan -- the index geometry, trace launch and workspace of region traces
and the argument rules dbde_hip_traces shares with them.  Pure host arithmetic; no GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALL = ("max", "min", "sum", "sumsq")


@pytest.fixture(scope="module")
def dv():
    import dbde_video_cpp_amd as m
    if not os.path.exists(m.LIB_PATH):
        m.build()
    return m


def info(W, H, L=10, active=None, whole=0):
    """A map info without building a map: `active` tiles (default all)."""
    T = ((W + 7) // 8) * ((H + 7) // 8)
    a = T if active is None else active
    return dict(W=W, H=H, n_labels=L, tiles=T, tiles_active=a, tiles_whole=whole, tiles_mixed=a - whole,
                device_bytes=0)


def expect(W, H, n, inf, stats, n_cu, pix):
    """The plan worked out from the format: 8x8 tiles, index chunks at every tile row (512-tile pieces of wider rows),
    spans of 256 / (8 pix) tile columns, segments of >= 16 frames until ~4 busy workgroups per CU."""
    w, h = (W + 7) // 8, (H + 7) // 8
    pieces = (w + 511) // 512
    if h * pieces <= 32768:
        cpf, ct = h * pieces, (w if pieces == 1 else 512)
    else:
        cpf, ct = (w * h + 511) // 512, 512
    K = 32 // pix
    sx = (w + K - 1) // K
    busy = max(1, (inf["tiles_active"] + K - 1) // K)
    target = 4 * n_cu
    seg = 1 if busy >= target else (target + busy - 1) // busy
    seg = min(seg, (n + 15) // 16)
    seg = max(seg, 1)
    fps = (n + seg - 1) // seg
    if fps:
        seg = (n + fps - 1) // fps
    mask = sum({"max": 1, "min": 2, "sum": 4, "sumsq": 8}[s] for s in stats)
    ws = ((4 * n * inf["n_labels"] + 15) // 16) * 16
    return dict(chunks_per_frame=cpf, chunk_tiles=ct, threads=256, tiles_per_workgroup=K, spans_x=sx, spans=sx * h,
                segments=seg, frames_per_segment=fps, grid=sx * h * seg,
                row_grid=(n * inf["n_labels"] + 255) // 256,
                workspace_bytes=ws * ((mask & 1) + ((mask >> 1) & 1)))


CASES = [
    # (W, H, n, active, L)
    (4096, 3072, 1024, None, 2000),
    (4096, 3072, 1024, 9830, 2000),     # ~5 % of the tiles
    (4096, 3072, 128, 12, 3),
    (1921, 1081, 7, None, 100),
    (100, 75, 11, 20, 3),
    (64, 64, 100000, 64, 65535),
    (8, 8, 1, 1, 1),
    (4200, 24, 3, 100, 5),              # a row wider than 512 tiles
    (8, 262152, 2, 5, 5),               # 32,769 tile rows: plain 512-tile chunks
    (9, 9, 0, 4, 2),
]


@pytest.mark.parametrize("pix", [1, 2])
@pytest.mark.parametrize("W,H,n,active,L", CASES)
@pytest.mark.parametrize("stats", [ALL, ("sum",), ("max", "min"), ("min", "sumsq")])
def test_plan_geometry(dv, pix, W, H, n, active, L, stats):
    inf = info(W, H, L, active)
    fn = dv.trace_plan if pix == 1 else dv.trace16_plan
    p = fn(W, H, n, inf, stats, n_cu=256)
    for k, v in expect(W, H, n, inf, stats, 256, pix).items():
        assert p[k] == v, (k, p[k], v)
    assert p["grid"] < 2 ** 31 and p["segments"] * p["frames_per_segment"] >= n


@pytest.mark.parametrize("W,H,n,active,L", CASES)
def test_8_and_16_bit_plans_differ_only_in_the_lane_mapping(dv, W, H, n, active, L):
    """DBDE16 takes 16 lanes per tile: half the tiles per workgroup, so spans and grid change with it (and the
    segments, which follow the busy spans); the index geometry and the workspace are the same."""
    inf = info(W, H, L, active)
    a, b = dv.trace_plan(W, H, n, inf), dv.trace16_plan(W, H, n, inf)
    assert a["tiles_per_workgroup"] == 32 and b["tiles_per_workgroup"] == 16
    same = {k for k in a if k not in ("tiles_per_workgroup", "spans_x", "spans", "segments", "frames_per_segment",
                                      "grid")}
    assert {k: a[k] for k in same} == {k: b[k] for k in same}
    w = (W + 7) // 8
    assert b["spans_x"] == (w + 15) // 16 and a["spans_x"] == (w + 31) // 32


def test_plan_from_a_real_summary(dv):
    lab = np.zeros((3072, 4096), np.int32)
    lab[:64, :64] = 1
    s = dv.trace_map_summary(lab)
    p = dv.trace_plan(4096, 3072, 1024, s)
    assert s["tiles_active"] == 64 and p["segments"] == 64 and p["frames_per_segment"] == 16


def test_argument_rules(dv):
    inf = info(200, 123)
    for fn in (dv.trace_plan, dv.trace16_plan):
        fn(200, 123, 5, inf)
        with pytest.raises(ValueError):   # W / H other than the map's
            fn(201, 123, 5, inf)
        with pytest.raises(ValueError):
            fn(200, 120, 5, inf)
        with pytest.raises(ValueError):   # no statistic
            fn(200, 123, 5, inf, stats=0)
        with pytest.raises(ValueError):   # an unknown statistic bit
            fn(200, 123, 5, inf, stats=16)
        with pytest.raises(ValueError):   # bad n_cu
            fn(200, 123, 5, inf, n_cu=0)
        with pytest.raises(ValueError):
            fn(200, 123, 5, inf, n_cu=-3)
        with pytest.raises(ValueError):   # negative n_frames
            fn(200, 123, -1, inf)
        with pytest.raises(ValueError):   # an info that does not describe a map of this size
            fn(200, 123, 5, dict(inf, tiles=inf["tiles"] + 1))
        with pytest.raises(ValueError):
            fn(200, 123, 5, dict(inf, n_labels=0))
        with pytest.raises(ValueError):   # too many chunks in one call
            fn(8, 8, 2 ** 31 - 1, info(8, 8))
