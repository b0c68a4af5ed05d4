"""CPU: dbde_hip_project_counts_plan -- the launch, the segments and the workspace of a count projection, and every
argument rule dbde_hip_project_counts shares with it.  Pure host arithmetic; no GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GEOMETRY = ("tile_x", "tile_y", "tiles_x", "tiles_y", "chunks_per_frame", "chunk_tiles", "chunk_pieces", "index_split",
            "threads", "pieces_x", "segments", "frames_per_segment", "max_frames_per_segment", "grid", "combine_grid")
CASES = [(4096, 3072, 1024, 0, 0, 4096, 3072, 256), (4096, 3072, 1024, 1000, 1000, 1024, 1024, 256),
         (4096, 3072, 1024, 77, 5, 256, 256, 256), (64, 64, 65536, 0, 0, 64, 64, 256), (64, 64, 70000, 0, 0, 64, 64, 1),
         (1921, 1081, 7, 1, 1, 1920, 1080, 304), (4200, 24, 3, 0, 0, 4200, 24, 256), (200, 123, 5, 3, 0, 1, 123, 256),
         (72, 40, 70, 0, 0, 72, 40, 8), (72, 40, 100, 3, 5, 41, 27, 256), (8, 8, 1, 0, 0, 8, 8, 256),
         (64, 64, 0, 0, 0, 64, 64, 256)]


@pytest.fixture(scope="module")
def dv():
    import dbde_video_cpp_amd as m
    if not os.path.exists(m.LIB_PATH):
        m.build()
    return m


@pytest.mark.parametrize("W,H,n,x,y,rw,rh,n_cu", CASES)
def test_geometry_and_segments_are_project_plans(dv, W, H, n, x, y, rw, rh, n_cu):
    for plan, ref in ((dv.counts_plan, dv.project_plan), (dv.counts16_plan, dv.project16_plan)):
        for K in (1, 3, 8):
            for maps in (False, True):
                p = plan(W, H, n, x, y, rw, rh, levels=K, n_cu=n_cu, maps=maps)
                for stats in (("sum",), ("max", "min", "sum", "sumsq")):
                    q = ref(W, H, n, x, y, rw, rh, stats=stats, n_cu=n_cu)
                    for k in GEOMETRY:
                        assert p[k] == q[k], (k, W, H, n, K)
                assert p["levels"] == K and p["lds_bytes"] == 272


@pytest.mark.parametrize("W,H,n,x,y,rw,rh,n_cu", CASES)
def test_workspace_bytes(dv, W, H, n, x, y, rw, rh, n_cu):
    for plan in (dv.counts_plan, dv.counts16_plan):
        for K in (1, 2, 5, 8):
            p = plan(W, H, n, x, y, rw, rh, levels=K, n_cu=n_cu)
            S = p["segments"]
            want = (4 * S * K * rw * rh + 15) // 16 * 16 if S > 1 else 0
            assert p["workspace_bytes"] == want, (W, H, n, K, S)
            assert p["combine_grid"] == (-(-rw * rh // 256) if S > 1 else 0)


def test_some_cases_have_several_segments(dv):
    assert dv.counts_plan(64, 64, 65536)["segments"] > 1
    assert dv.counts_plan(4096, 3072, 1024, 77, 5, 256, 256)["segments"] > 1
    assert dv.counts_plan(4096, 3072, 1024)["segments"] == 1
    assert dv.counts_plan(64, 64, 70000, n_cu=1)["segments"] == 2       # the 65,536 cap is kept
    # an odd workspace: 3 segments x 1 level x 1 pixel = 12 bytes -> 16
    p = dv.counts_plan(200, 123, 96, 7, 7, 1, 1, levels=1)
    assert p["segments"] == 3 and p["workspace_bytes"] == 16


def test_argument_rules(dv):
    for plan, pix in ((dv.counts_plan, 1), (dv.counts16_plan, 2)):
        def bad(*a, **k):
            with pytest.raises(ValueError):
                plan(*a, **k)
        plan(64, 64, 10, levels=1)
        plan(64, 64, 10, levels=8)
        bad(64, 64, 10, levels=0)                                           # K outside 1..8
        bad(64, 64, 10, levels=9)
        bad(64, 64, 10, levels=-1)
        # level_stride: ignored for scalars, >= rw * rh for maps
        plan(64, 64, 10, levels=2, level_stride=0)
        plan(64, 64, 10, levels=2, maps=True, level_stride=4096)
        plan(64, 64, 10, levels=2, maps=True, level_stride=1 << 40)
        bad(64, 64, 10, levels=2, maps=True, level_stride=4095)
        bad(64, 64, 10, levels=1, maps=True, level_stride=0)                # also for one level
        plan(64, 64, 10, 3, 5, 41, 27, levels=2, maps=True, level_stride=41 * 27)
        bad(64, 64, 10, 3, 5, 41, 27, levels=2, maps=True, level_stride=41 * 27 - 1)
        plan(64, 64, 10, maps=1)
        for flags in (2, 3, 4, 0x100, -2):                                  # unknown flag bits
            bad(64, 64, 10, maps=flags)
        for name in ("thresholds", "out", "count"):
            bad(64, 64, 10, addresses={name: 0})                            # NULL
        if pix == 1:
            for a in (4097, 4098, 4099):
                plan(64, 64, 10, addresses={"thresholds": a})               # U8 thresholds: any address
        else:
            for a in (4097, 4099):
                bad(64, 64, 10, addresses={"thresholds": a})                # U16 thresholds: 2-byte aligned
            plan(64, 64, 10, addresses={"thresholds": 4098})
        for a in (4097, 4098, 4099):
            bad(64, 64, 10, addresses={"out": a})                           # U32: 4-byte aligned
        plan(64, 64, 10, addresses={"out": 4100})
        for a in (4097, 4098, 4100):
            bad(64, 64, 10, addresses={"count": a})                         # U64: 8-byte aligned
        plan(64, 64, 10, addresses={"count": 4104})
        plan(64, 64, 0)                                                     # n_frames == 0 is a valid call
        # the window errors are dbde_hip_project's
        bad(64, 64, 10, 60, 0, 8, 8)
        bad(64, 64, 10, 0, 60, 8, 8)
        bad(64, 64, 10, -1, 0, 8, 8)
        bad(64, 64, 10, 0, 0, 0, 8)
        bad(64, 64, 10, 0, 0, 8, 0)
        bad(64, 64, -1)
        bad(0, 64, 10, 0, 0, 1, 1)
        for args in [(64, 64, 10, 60, 0, 8, 8), (64, 64, -1, 0, 0, 64, 64), (64, 64, 10, 0, 0, 0, 8)]:
            with pytest.raises(ValueError):
                dv.project_plan(*args)
