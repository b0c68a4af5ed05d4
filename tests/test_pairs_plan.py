"""CPU: dbde_hip_project_pairs_plan -- the launch, the halo, the segments and the workspace of a pair projection against
the formulas written in include/dbde_hip.h, and every argument rule dbde_hip_project_pairs shares with it.  Pure host
arithmetic; no GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SAME = ("tile_x", "tile_y", "tiles_x", "tiles_y", "chunks_per_frame", "chunk_tiles", "chunk_pieces", "index_split",
        "threads", "max_frames_per_segment")
CASES = [(4096, 3072, 1024, 0, 0, 4096, 3072, 256), (4096, 3072, 1024, 1000, 1000, 1024, 1024, 256),
         (4096, 3072, 1024, 77, 5, 256, 256, 256), (64, 64, 65536, 0, 0, 64, 64, 256), (64, 64, 70000, 0, 0, 64, 64, 1),
         (1921, 1081, 7, 1, 1, 1920, 1080, 304), (4200, 24, 3, 0, 0, 4200, 24, 256), (200, 123, 5, 3, 0, 1, 123, 256),
         (72, 40, 70, 0, 0, 72, 40, 8), (72, 40, 100, 3, 5, 41, 27, 256), (8, 8, 1, 0, 0, 8, 8, 256),
         (64, 64, 0, 0, 0, 64, 64, 256), (520, 16, 13, 0, 0, 520, 16, 256), (520, 16, 13, 251, 1, 13, 14, 256)]


@pytest.fixture(scope="module")
def dv():
    import dbde_video_cpp_amd as m
    if not os.path.exists(m.LIB_PATH):
        m.build()
    return m


def instance_of(mask):
    return 1 if mask == 1 else 3 if mask in (2, 3) else 15


def segments_of(base, n, n_cu):
    """dbde_hip_project_plan's rule for `base` workgroups per segment."""
    target = 4 * max(n_cu, 1)
    seg = 1 if base >= target else -(-target // base)
    seg = min(seg, -(-n // 32))
    seg = max(seg, -(-n // 65536), 1)
    fps = -(-n // seg)
    if fps:
        seg = -(-n // fps)
    return seg, fps


@pytest.mark.parametrize("W,H,n,x,y,rw,rh,n_cu", CASES)
def test_the_plan_follows_the_headers_formulas(dv, W, H, n, x, y, rw, rh, n_cu):
    for plan, ref, pix in ((dv.pairs_plan, dv.project_plan, 1), (dv.pairs16_plan, dv.project16_plan, 2)):
        q = ref(W, H, n, x, y, rw, rh, stats=("sum",), n_cu=n_cu)
        for mask in range(1, 16):
            p = plan(W, H, n, x, y, rw, rh, pairs=mask, n_cu=n_cu)
            for k in SAME:
                assert p[k] == q[k], (k, W, H, n, mask)
            inst = instance_of(mask)
            P = 256 // (8 * pix)
            hl, hr = int(bool(inst & 8)), int(bool(inst & 5))
            s = P - hl - hr
            ntx = p["tiles_x"]
            pieces = 1 if ntx <= P else 1 + -(-(ntx - P) // s)
            assert (p["instance"], p["piece_tiles"], p["halo_left"], p["halo_right"], p["piece_stride"]) == (inst, P, hl, hr, s)
            assert p["pieces_x"] == pieces and p["planes"] == bin(mask).count("1")
            # every tile has an owner: the last piece reaches the window's last tile, and the one before does not
            assert (pieces - 1) * s + P >= ntx and (pieces == 1 or (pieces - 2) * s + P < ntx)
            assert p["rows_below"] == (p["tiles_y"] - 1 if inst != 1 else 0)
            S, fps = segments_of(pieces * p["tiles_y"], n, n_cu)
            assert (p["segments"], p["frames_per_segment"]) == (S, fps), (W, H, n, mask)
            assert p["grid"] == pieces * p["tiles_y"] * S
            assert p["combine_grid"] == (-(-rw * rh // 256) if S > 1 else 0)
            want = (4 * pix * S * p["planes"] * rw * rh + 15) // 16 * 16 if S > 1 else 0
            assert p["workspace_bytes"] == want, (W, H, n, mask, S)
            R = 8 if inst == 1 else 9
            assert p["lds_bytes"] == 2 * 4 * R * 288 + 2 * 4 * (R - 7) * 32 + 16
            if pieces == q["pieces_x"]:     # the same grid: the same segments as dbde_hip_project
                assert (p["segments"], p["frames_per_segment"]) == (q["segments"], q["frames_per_segment"])


def test_pieces_overlap_from_264_and_136_pixels(dv):
    for mask in range(1, 16):
        assert dv.pairs_plan(256, 16, 13, pairs=mask)["pieces_x"] == 1
        assert dv.pairs_plan(264, 16, 13, pairs=mask)["pieces_x"] == 2
        assert dv.pairs_plan(520, 16, 13, 255, 7, 2, 2, pairs=mask)["pieces_x"] == 1      # two tiles
        assert dv.pairs16_plan(128, 16, 13, pairs=mask)["pieces_x"] == 1
        assert dv.pairs16_plan(136, 16, 13, pairs=mask)["pieces_x"] == 2
    # 65 tiles: strides of 31 (instances 1 and 3; DOWN alone runs instance 3) and 30 (instance 15) both give 3 pieces
    assert [dv.pairs_plan(520, 16, 13, pairs=m)["pieces_x"] for m in (2, 1, 3, 15)] == [3, 3, 3, 3]
    assert [dv.pairs_plan(768, 16, 13, pairs=m)["pieces_x"] for m in (2, 1, 3, 15)] == [4, 4, 4, 4]
    assert [dv.pairs_plan(4096, 16, 13, pairs=m)["pieces_x"] for m in (1, 15)] == [17, 17]
    assert [dv.pairs16_plan(264, 16, 13, pairs=m)["pieces_x"] for m in (1, 15)] == [3, 3]


def test_some_cases_have_several_segments(dv):
    assert dv.pairs_plan(64, 64, 65536)["segments"] > 1
    assert dv.pairs_plan(4096, 3072, 1024, 77, 5, 256, 256)["segments"] > 1
    assert dv.pairs_plan(4096, 3072, 1024)["segments"] == 1
    assert dv.pairs_plan(64, 64, 70000, n_cu=1)["segments"] == 2       # the 65,536 cap is kept
    p = dv.pairs_plan(200, 123, 96, 7, 7, 1, 1, pairs=1)               # 3 segments x 1 plane x 1 pixel = 12 bytes -> 16
    assert p["segments"] == 3 and p["workspace_bytes"] == 16
    assert dv.pairs16_plan(200, 123, 96, 7, 7, 1, 1, pairs=3)["workspace_bytes"] == 48


def test_argument_rules(dv):
    for plan in (dv.pairs_plan, dv.pairs16_plan):
        def bad(*a, **k):
            with pytest.raises(ValueError):
                plan(*a, **k)
        for mask in range(1, 16):
            plan(64, 64, 10, pairs=mask)
        for mask in (0, 16, 17, 255, -1, -15):                              # pairs outside 1..15
            bad(64, 64, 10, pairs=mask)
        for name in ("out", "count"):
            bad(64, 64, 10, addresses={name: 0})                            # NULL
            for a in (4097, 4098, 4100):
                bad(64, 64, 10, addresses={name: a})                        # U64: 8-byte aligned
            plan(64, 64, 10, addresses={name: 4104})
        plan(64, 64, 0)                                                     # n_frames == 0 is a valid call
        # the window errors are dbde_hip_project's
        bad(64, 64, 10, 60, 0, 8, 8)
        bad(64, 64, 10, 0, 60, 8, 8)
        bad(64, 64, 10, -1, 0, 8, 8)
        bad(64, 64, 10, 0, 0, 0, 8)
        bad(64, 64, 10, 0, 0, 8, 0)
        bad(64, 64, -1)
        bad(0, 64, 10, 0, 0, 1, 1)
    assert dv.lib().dbde_hip_project_pairs_plan(64, 64, 10, 0, 0, 64, 64, 15, 4096, 4096, 256, None) == dv.ERR_ARG


def test_pairs_mask_forms(dv):
    assert dv.pairs_mask(4) == 3 and dv.pairs_mask(8) == 15 and dv.pairs_mask(10) == 10 and dv.pairs_mask(1) == 1
    assert dv.pairs_mask([(1, 1)]) == dv.PAIR_DOWN_RIGHT == 4 and dv.pairs_mask([(-1, 1)]) == dv.PAIR_DOWN_LEFT == 8
    assert dv.pairs_mask(dv.PAIR_RIGHT | dv.PAIR_DOWN_LEFT) == 9
    assert dv.pair_offsets(15) == dv.PAIR_OFFSETS == ((1, 0), (0, 1), (1, 1), (-1, 1))
    assert dv.pair_offsets(10) == ((0, 1), (-1, 1))
    for bad in (0, 16, -3, [], [(0, 0)], [(1, -1)], True):
        with pytest.raises((ValueError, TypeError)):
            dv.pairs_mask(bad)
