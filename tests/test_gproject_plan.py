"""CPU: dbde_hip_project_groups_plan -- the launch and plane sizes of a grouped projection, and every argument rule
dbde_hip_project_groups shares with it.  Pure host arithmetic; no GPU."""
import os
import sys

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


def test_geometry_is_project_plans(dv):
    for (W, H, n, x, y, rw, rh) in [(4096, 3072, 1024, 0, 0, 4096, 3072), (1921, 1081, 7, 1, 1, 1920, 1080),
                                    (4200, 24, 3, 0, 0, 4200, 24), (200, 123, 5, 3, 0, 1, 123)]:
        for plan, ref in ((dv.project_groups_plan, dv.project_plan), (dv.project_groups16_plan, dv.project16_plan)):
            p, q = plan(W, H, n, x, y, rw, rh, group_frames=2), ref(W, H, n, x, y, rw, rh)
            for k in ("tile_x", "tile_y", "tiles_x", "tiles_y", "chunks_per_frame", "chunk_tiles", "chunk_pieces",
                      "index_split", "threads", "pieces_x"):
                assert p[k] == q[k], (k, W, H)
            assert p["max_group_frames"] == 65536 and p["workspace_bytes"] == 0 and p["stats"] == 15


@pytest.mark.parametrize("W,H,n,g,n_cu", [(4096, 3072, 1024, 2, 256), (4096, 3072, 1024, 1024, 256), (64, 64, 2000, 3, 256),
                                          (64, 64, 2000, 3, 1), (64, 64, 262144, 8, 256), (8, 8, 13, 1, 256),
                                          (200, 123, 13, 16, 256), (1921, 1081, 5, 7, 304)])
def test_runs_and_grid(dv, W, H, n, g, n_cu):
    for pix, plan in ((1, dv.project_groups_plan), (2, dv.project_groups16_plan)):
        p = plan(W, H, n, group_frames=g, n_cu=n_cu)
        ng = -(-n // g)
        assert p["grid"] == p["pieces_x"] * p["tiles_y"] * p["runs"]
        assert p["pieces_x"] == -(-p["tiles_x"] // (32 // pix))
        assert 1 <= p["groups_per_run"] <= ng and p["runs"] == -(-ng // p["groups_per_run"])   # no empty run
        base = p["pieces_x"] * p["tiles_y"]
        if base >= 4 * n_cu:
            assert p["runs"] == 1
        if p["runs"] > 1:   # cut only to fill the device, never below 32 frames a run
            assert p["groups_per_run"] * g >= 32
            assert base * (p["runs"] - 1) < 4 * n_cu + base


def test_one_run_for_a_large_window_and_several_for_a_small_one(dv):
    assert dv.project_groups_plan(4096, 3072, 1024, group_frames=2)["runs"] == 1
    assert dv.project_groups_plan(4096, 3072, 1024, has_group_starts=True, n_groups=300)["runs"] == 1
    assert dv.project_groups_plan(64, 64, 2000, group_frames=3)["runs"] > 1
    assert dv.project_groups16_plan(64, 64, 2000, group_frames=3)["runs"] > 1
    assert dv.project_groups_plan(64, 64, 2000, has_group_starts=True, n_groups=700)["runs"] > 1
    assert dv.project_groups_plan(64, 64, 2000, group_frames=2000)["runs"] == 1   # one group is never split


def test_plane_bytes(dv):
    W, H, n, g = 200, 123, 13, 4
    x, y, rw, rh = 5, 3, 131, 77
    P = 4 * rw * rh
    p = dv.project_groups_plan(W, H, n, x, y, rw, rh, group_frames=g)
    assert (p["max_bytes"], p["min_bytes"], p["sum_bytes"], p["sumsq_bytes"], p["counts_bytes"]) == (P, P, 4 * P, 8 * P, 16)
    p = dv.project_groups_plan(W, H, n, x, y, rw, rh, group_frames=g, stats=("sum", "max"), sum_dtype=dv.SUM_U16)
    assert (p["max_bytes"], p["min_bytes"], p["sum_bytes"], p["sumsq_bytes"], p["stats"]) == (P, 0, 2 * P, 0, 5)
    p = dv.project_groups16_plan(W, H, n, x, y, rw, rh, group_frames=g)
    assert (p["max_bytes"], p["min_bytes"], p["sum_bytes"], p["sumsq_bytes"]) == (2 * P, 2 * P, 4 * P, 8 * P)
    p = dv.project_groups_plan(W, H, n, x, y, rw, rh, has_group_starts=True, n_groups=9, stats=("min",))
    assert (p["min_bytes"], p["counts_bytes"]) == (9 * rw * rh, 36)
    # planes past 2^32 bytes: 342 groups of 4096 x 3072
    p = dv.project_groups_plan(4096, 3072, 684, group_frames=2, stats=("max",))
    assert p["max_bytes"] == 342 * 4096 * 3072 > 2 ** 32


def test_zero_frames(dv):
    p = dv.project_groups_plan(64, 64, 0, group_frames=5)
    assert p["runs"] == 0 and p["grid"] == 0 and p["counts_bytes"] == 0
    p = dv.project_groups_plan(64, 64, 0, has_group_starts=True, n_groups=3)   # three empty groups are still written
    assert p["runs"] >= 1 and p["counts_bytes"] == 12


def test_argument_rules(dv):
    for plan in (dv.project_groups_plan, dv.project_groups16_plan):
        ok = lambda *a, **k: plan(*a, **k)   # noqa: E731

        def bad(*a, **k):
            with pytest.raises(ValueError):
                plan(*a, **k)
        ok(64, 64, 10, group_frames=3, n_groups=4)
        bad(64, 64, 10, group_frames=3, has_group_starts=True, n_groups=4)     # both forms
        bad(64, 64, 10, group_frames=0, has_group_starts=False, n_groups=4)    # neither
        bad(64, 64, 10, group_frames=3, n_groups=3)                            # n_groups != ceil(n / g)
        bad(64, 64, 10, group_frames=3, n_groups=5)
        bad(64, 64, 10, group_frames=-1, n_groups=10)
        ok(64, 64, 70000, group_frames=65536)
        bad(64, 64, 70000, group_frames=65537)                                 # g > 65,536
        ok(64, 64, 65536, has_group_starts=True, n_groups=2)
        bad(64, 64, 65537, has_group_starts=True, n_groups=2)                  # ragged with n > 65,536
        bad(64, 64, 10, has_group_starts=True, n_groups=0)                     # ragged needs a group
        bad(64, 64, 10, group_frames=3, stats=0)                               # no plane
        bad(64, 64, 10, group_frames=3, addresses={"counts": 0})               # d_counts is required
        bad(64, 64, 10, group_frames=3, sum_dtype=2)                           # unknown sum_type
        bad(64, 64, 10, 60, 0, 8, 8, group_frames=3)                           # window outside the frame
        bad(64, 64, -1, group_frames=3, n_groups=0)


def test_u16_sums(dv):
    plan = dv.project_groups_plan
    plan(8, 8, 1000, group_frames=257, sum_dtype=dv.SUM_U16)
    plan(8, 8, 257, has_group_starts=True, n_groups=5, sum_dtype=dv.SUM_U16)
    for kw in (dict(group_frames=258), dict(has_group_starts=True, n_groups=5)):
        with pytest.raises(ValueError):                                       # a group could exceed 257 frames
            plan(8, 8, 1000, sum_dtype=dv.SUM_U16, **kw)
    with pytest.raises(ValueError):                                           # U16 with accumulate
        plan(8, 8, 1000, group_frames=257, sum_dtype=dv.SUM_U16, accumulate=True)
    plan(8, 8, 1000, group_frames=257, accumulate=True)
    with pytest.raises(ValueError):                                           # U16 for DBDE16
        dv.project_groups16_plan(8, 8, 1000, group_frames=2, sum_dtype=dv.SUM_U16)


def test_misaligned_outputs(dv):
    kw = dict(group_frames=3)
    for odd in (1, 3, 4097):
        dv.project_groups_plan(64, 64, 10, addresses={"max": odd, "min": odd}, **kw)         # U8 planes: any address
        for name in ("max", "min"):
            with pytest.raises(ValueError):
                dv.project_groups16_plan(64, 64, 10, addresses={name: odd}, **kw)            # U16 planes: 2-byte
    dv.project_groups16_plan(64, 64, 10, addresses={"max": 4098, "min": 6}, **kw)
    for plan in (dv.project_groups_plan, dv.project_groups16_plan):
        for a in (4097, 4098, 4099):
            with pytest.raises(ValueError):
                plan(64, 64, 10, addresses={"sum": a}, **kw)                                 # U32 sums: 4-byte
            with pytest.raises(ValueError):
                plan(64, 64, 10, addresses={"counts": a}, **kw)
        plan(64, 64, 10, addresses={"sum": 4100, "counts": 4100}, **kw)
        for a in (4097, 4098, 4100):
            with pytest.raises(ValueError):
                plan(64, 64, 10, addresses={"sumsq": a}, **kw)                               # U64: 8-byte
        plan(64, 64, 10, addresses={"sumsq": 4104}, **kw)
    dv.project_groups_plan(64, 64, 10, addresses={"sum": 4098}, sum_dtype=dv.SUM_U16, **kw)  # U16 sums: 2-byte
    with pytest.raises(ValueError):
        dv.project_groups_plan(64, 64, 10, addresses={"sum": 4097}, sum_dtype=dv.SUM_U16, **kw)
