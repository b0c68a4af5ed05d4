"""CPU: dbde_hip_project_lag_plan -- the launch, the segments, the history frames, the instance and the workspace of a
lag projection against the formulas written in include/dbde_hip.h, and every argument rule dbde_hip_project_lag shares
with it.  Pure host arithmetic; no GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SAME = ("tile_x", "tile_y", "tiles_x", "tiles_y", "chunks_per_frame", "chunk_tiles", "chunk_pieces", "index_split",
        "threads", "pieces_x", "segments", "frames_per_segment", "max_frames_per_segment", "grid", "combine_grid")
CASES = [(4096, 3072, 1024, 0, 0, 4096, 3072, 256), (4096, 3072, 1024, 1000, 1000, 1024, 1024, 256),
         (4096, 3072, 1024, 77, 5, 256, 256, 256), (64, 64, 65536, 0, 0, 64, 64, 256), (64, 64, 70000, 0, 0, 64, 64, 1),
         (1921, 1081, 7, 1, 1, 1920, 1080, 304), (200, 123, 5, 3, 0, 1, 123, 256), (72, 40, 70, 0, 0, 72, 40, 8),
         (72, 40, 100, 3, 5, 41, 27, 256), (8, 8, 1, 0, 0, 8, 8, 256), (64, 64, 0, 0, 0, 64, 64, 256),
         (300, 20, 13, 0, 0, 300, 20, 256), (64, 64, 33, 0, 0, 64, 64, 256)]


@pytest.fixture(scope="module")
def dv():
    import dbde_video_cpp_amd as m
    if not os.path.exists(m.LIB_PATH):
        m.build()
    return m


def instance_of(mask):
    return 3 if mask & ~3 == 0 else 28 if mask & ~28 == 0 else 31


def workspace_of(mask, S, pixels, pix):
    """Per requested statistic S * pixels elements rounded up to 16 bytes: product, pairsum, sqdiff 4 * pix bytes,
    absdiff 4, maxdiff pix; nothing for one segment."""
    if S <= 1:
        return 0
    width = {1: 4 * pix, 2: 4 * pix, 4: 4, 8: 4 * pix, 16: pix}
    return sum((w * S * pixels + 15) // 16 * 16 for bit, w in width.items() if mask & bit)


@pytest.mark.parametrize("W,H,n,x,y,rw,rh,n_cu", CASES)
def test_the_plan_follows_the_headers_formulas(dv, W, H, n, x, y, rw, rh, n_cu):
    for plan, ref, pix in ((dv.lag_plan, dv.project_plan, 1), (dv.lag16_plan, dv.project16_plan, 2)):
        q = ref(W, H, n, x, y, rw, rh, stats=("sum",), n_cu=n_cu)
        for lag, lead in ((1, 0), (3, 0), (8, 0), (2, min(n, 5)), (8, min(n, 3)), (4, n)):
            for mask in range(1, 32):
                p = plan(W, H, n, x, y, rw, rh, lag=lag, lead=lead, stats=mask, n_cu=n_cu)
                for k in SAME:      # segments and fps are dbde_hip_project_plan's for the same window, n and n_cu
                    assert p[k] == q[k], (k, W, H, n, mask)
                assert p["instance"] == instance_of(mask) and p["instance"] & mask == mask   # a superset of the request
                assert p["planes"] == bin(mask).count("1")
                S, fps = p["segments"], p["frames_per_segment"]
                first = max(lead, lag)
                assert p["first_pair"] == first and p["first_frame"] == max(lead - lag, 0) == first - lag
                # the segments that count a pair: segment s holds [s fps, (s + 1) fps) cut at n
                active = sum(1 for s in range(S) if max(s * fps, first) < min((s + 1) * fps, n)) if S < 5000 else None
                if active is not None:
                    assert p["history_frames"] == max(active - 1, 0) * lag, (W, H, n, lag, lead)
                assert p["workspace_bytes"] == workspace_of(mask, S, rw * rh, pix), (W, H, n, mask, S)
                assert p["lds_bytes"] == 8 * 256 * 8 + 2 * 4 * 2 * 16 + 32 == 16672


def test_two_segments_of_17_decode_the_history_twice(dv):
    """n_cu = 256, a 64 x 64 window, n = 33: 2 segments of 17; segment 1 counts the pairs whose later frame is 17..32
    and decodes frames 17 - lag..16 a second time."""
    for plan in (dv.lag_plan, dv.lag16_plan):
        for lag in range(1, 9):
            p = plan(64, 64, 33, lag=lag, n_cu=256)
            assert (p["segments"], p["frames_per_segment"]) == (2, 17)
            assert p["first_frame"] == 0 and p["first_pair"] == lag and p["history_frames"] == lag
            # a lead past segment 0: only segment 1 counts, from frame lead - lag on, and nothing is decoded twice
            q = plan(64, 64, 33, lag=lag, lead=20, n_cu=256)
            assert q["first_frame"] == 20 - lag and q["first_pair"] == 20 and q["history_frames"] == 0
            # no pair at all
            assert plan(64, 64, 33, lag=lag, lead=33, n_cu=256)["history_frames"] == 0
            assert plan(64, 64, lag, lag=lag, n_cu=256)["history_frames"] == 0
        assert plan(64, 64, 70, lag=5, n_cu=256)["segments"] == 3 and plan(64, 64, 70, lag=5)["history_frames"] == 10
    p = dv.lag_plan(200, 123, 96, 7, 7, 1, 1, stats=16)                # 3 segments x 1 pixel x 1 byte -> 16
    assert p["segments"] == 3 and p["workspace_bytes"] == 16
    assert dv.lag16_plan(200, 123, 96, 7, 7, 1, 1, stats=31)["workspace_bytes"] == 3 * 32 + 16 + 16   # 24 -> 32, 12 -> 16, 6 -> 16
    assert dv.lag_plan(64, 64, 70000, n_cu=1)["segments"] == 2         # the 65,536 cap is kept


def test_argument_rules(dv):
    for plan in (dv.lag_plan, dv.lag16_plan):
        def bad(*a, **k):
            with pytest.raises(ValueError):
                plan(*a, **k)
        for lag in range(1, 9):
            plan(64, 64, 10, lag=lag)
        for lag in (0, 9, -1, 64):                                          # lag outside 1..8
            bad(64, 64, 10, lag=lag)
        for lead in (0, 1, 10):
            plan(64, 64, 10, lead=lead)
        for lead in (-1, 11, 1 << 20):                                      # lead outside 0..n_frames
            bad(64, 64, 10, lead=lead)
        bad(64, 64, 0, lead=1)
        for mask in (0, 32, 33, 255, -1):                                   # no plane requested, unknown statistics
            bad(64, 64, 10, stats=mask)
        for name in ("pairs", "count"):
            bad(64, 64, 10, addresses={name: 0})                            # NULL
        for name in ("sums", "pairs", "count"):
            for a in (4097, 4098, 4100):
                bad(64, 64, 10, addresses={name: a})                        # U64: 8-byte aligned
            plan(64, 64, 10, addresses={name: 4104})
        plan(64, 64, 10, addresses={"maxdiff": 4098})
        plan(64, 64, 10, stats=15, addresses={"maxdiff": 0, "sums": 4096})  # a NULL plane is only not computed
        plan(64, 64, 0)                                                     # n_frames == 0 is a valid call
        # the window errors are dbde_hip_project's
        bad(64, 64, 10, 60, 0, 8, 8)
        bad(64, 64, 10, 0, 60, 8, 8)
        bad(64, 64, 10, -1, 0, 8, 8)
        bad(64, 64, 10, 0, 0, 0, 8)
        bad(64, 64, 10, 0, 0, 8, 0)
        bad(64, 64, -1)
        bad(0, 64, 10, 0, 0, 1, 1)
    dv.lag_plan(64, 64, 10, addresses={"maxdiff": 4097})                    # U8 plane: any address
    with pytest.raises(ValueError):
        dv.lag16_plan(64, 64, 10, addresses={"maxdiff": 4097})              # U16 plane: 2-byte aligned
    assert dv.lib().dbde_hip_project_lag_plan(64, 64, 10, 0, 0, 64, 64, 1, 0, 31, 4096, 4096, 4096, 4096, 256,
                                              None) == dv.ERR_ARG


def test_lag_mask_forms(dv):
    assert dv.LAG_STATS == ("product", "pairsum", "absdiff", "sqdiff", "maxdiff") and dv.LAG_MAX == 8
    assert dv.lag_mask("sqdiff") == 8 and dv.lag_mask(("product", "pairsum")) == 3 and dv.lag_mask(dv.LAG_STATS) == 31
    assert dv.lag_mask(20) == 20 and dv.lag_stats(20) == ("absdiff", "maxdiff")
    for bad in (0, 32, (), ("sum",), "pairs"):
        with pytest.raises(ValueError):
            dv.lag_mask(bad)
