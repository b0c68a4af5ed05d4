"""CPU: dbde_hip_binned_plan / dbde16_hip_binned_plan -- what a binned decode validates and launches (host arithmetic).

The plan validates exactly what dbde_hip_decode_binned validates of its sizes: the window decoder's rules (every
rejection must be dbde_hip_roi_plan's verdict for the same window), a bin of 2, 4 or 8, an origin that is a multiple
of the bin, at least one statistic.  It reports dbde_hip_roi_plan's tile window and index geometry, the planes' shape
and bytes, and the binning kernel's launch.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import binned_ref as br   # noqa: E402

SHAPES = [(4096, 3072, 3), (1921, 1081, 3), (200, 123, 7), (1, 1, 5), (8, 8, 9), (9, 9, 9), (4200, 24, 3)]
GEOMETRY = ("tile_x", "tile_y", "tiles_x", "tiles_y", "chunks_per_frame", "chunk_tiles", "chunk_pieces", "index_split")
ALL = ("sum", "max", "min")


@pytest.fixture(scope="module")
def dv():
    import dbde_video_cpp_amd as m
    if not os.path.exists(m.LIB_PATH):
        m.build()
    return m


def both(dv):
    """(pixel bytes, binned plan, window plan, threads of a window more than 64 tiles across)."""
    return ((1, dv.binned_plan, dv.roi_plan, 256), (2, dv.binned16_plan, dv.roi16_plan, 128))


@pytest.mark.parametrize("W,H,n", SHAPES)
def test_plans_of_the_tested_shapes(dv, W, H, n):
    for pix, plan_fn, roi_fn, wide in both(dv):
        for b in (2, 4, 8):
            for (x, y, rw, rh) in br.windows(W, H, b):
                for stats in (ALL, ("sum",), ("max",), ("min", "sum")):
                    pl = plan_fn(W, H, n, b, x, y, rw, rh, stats=stats)
                    roi = roi_fn(W, H, n, x, y, rw, rh)
                    assert {k: pl[k] for k in GEOMETRY} == {k: roi[k] for k in GEOMETRY}
                    oh, ow = -(-rh // b), -(-rw // b)
                    assert (pl["out_h"], pl["out_w"]) == (oh, ow) == br.out_shape(rw, rh, b)
                    assert pl["sum_bytes"] == (n * oh * ow * 2 * pix if "sum" in stats else 0)
                    assert pl["max_bytes"] == (n * oh * ow * pix if "max" in stats else 0)
                    assert pl["min_bytes"] == (n * oh * ow * pix if "min" in stats else 0)
                    threads = 64 if pl["tiles_x"] <= 64 else wide
                    assert pl["threads"] == threads and pl["pieces_x"] == -(-pl["tiles_x"] // threads)
                    assert pl["grid"] == n * pl["tiles_y"] * pl["pieces_x"]
                    assert pl["lds_bytes"] == threads * 64 * pix + (64 if pix == 1 else 32) + 8 * (threads // 64)


def test_the_documented_example(dv):
    for b, (oh, ow) in ((2, (57, 96)), (4, (29, 48)), (8, (15, 24))):
        pl = dv.binned_plan(200, 123, 7, b, 8, 8, 191, 113, stats=ALL)
        assert (pl["out_h"], pl["out_w"]) == (oh, ow)
        assert (pl["tile_x"], pl["tile_y"], pl["tiles_x"], pl["tiles_y"]) == (1, 1, 24, 15)
        assert (pl["threads"], pl["pieces_x"], pl["grid"], pl["lds_bytes"]) == (64, 1, 7 * 15, 4168)
    pl = dv.binned_plan(4096, 3072, 1024, 4)
    assert (pl["threads"], pl["pieces_x"], pl["grid"], pl["lds_bytes"]) == (256, 2, 1024 * 384 * 2, 16480)
    assert pl["sum_bytes"] == 1024 * 768 * 1024 * 2 and pl["max_bytes"] == 0
    pl = dv.binned16_plan(4096, 3072, 128, 2, stats=ALL)
    assert (pl["threads"], pl["pieces_x"], pl["lds_bytes"]) == (128, 4, 16432)
    assert (pl["sum_bytes"], pl["max_bytes"], pl["min_bytes"]) == (128 * 1536 * 2048 * 4, 128 * 1536 * 2048 * 2,
                                                                  128 * 1536 * 2048 * 2)
    assert dv.binned_plan(200, 123, 0, 2)["grid"] == 0


def test_bin_origin_and_statistic_rules(dv):
    for pix, plan_fn, roi_fn, _ in both(dv):
        for b in (-2, 0, 1, 3, 5, 6, 7, 9, 16):
            with pytest.raises(ValueError):
                plan_fn(200, 123, 7, b)
        for b, x, y in ((2, 1, 0), (2, 0, 1), (4, 2, 0), (4, 0, 6), (8, 4, 0), (8, 0, 12), (8, 2, 8)):
            roi_fn(200, 123, 7, x, y, 50, 40)   # a good window for the window decoder
            with pytest.raises(ValueError):
                plan_fn(200, 123, 7, b, x, y, 50, 40)
        for b, x, y in ((2, 6, 10), (4, 12, 4), (8, 8, 16)):
            plan_fn(200, 123, 7, b, x, y, 50, 40)
        for stats in ((), 0, 8, 15):
            with pytest.raises(ValueError):
                plan_fn(200, 123, 7, 2, stats=stats)
        for stats in range(1, 8):
            plan_fn(200, 123, 7, 2, stats=stats)
        with pytest.raises(ValueError):
            plan_fn(200, 123, 7, 2, stats=("mean",))


WINDOWS = [  # (W, H, n, x, y, rw, rh)
    (200, 123, 7, 0, 0, 200, 123), (200, 123, -1, 0, 0, 200, 123), (0, 123, 1, 0, 0, 1, 1), (200, 0, 1, 0, 0, 1, 1),
    (200, 123, 7, 0, 0, 201, 123), (200, 123, 7, 0, 0, 200, 124), (200, 123, 7, 0, 0, 0, 5), (200, 123, 7, 0, 0, 5, 0),
    (200, 123, 7, -8, 0, 50, 50), (200, 123, 7, 0, -8, 50, 50), (200, 123, 7, 152, 0, 50, 50), (200, 123, 7, 0, 80, 50, 50),
    (200, 123, 7, 144, 72, 56, 51), (8, 262152, 2, 0, 0, 8, 262152), (8, 8 * 40000, 70000, 0, 0, 8, 8),
    (4096, 3072, 1 << 20, 0, 0, 4096, 3072), (1 << 20, 1 << 12, 1, 0, 0, 8, 8), (16, 16, 1 << 27, 0, 0, 16, 16)]


@pytest.mark.parametrize("W,H,n,x,y,rw,rh", WINDOWS)
def test_window_rules_are_the_window_decoders(dv, W, H, n, x, y, rw, rh):
    """Origins here are multiples of 8, so the only verdict is plan_roi's: the two plans accept or reject alike."""
    for pix, plan_fn, roi_fn, _ in both(dv):
        try:
            roi = roi_fn(W, H, n, x, y, rw, rh)
        except ValueError:
            roi = None
        for b in (2, 4, 8):
            if roi is None:
                with pytest.raises(ValueError):
                    plan_fn(W, H, n, b, x, y, rw, rh, stats=ALL)
            else:
                pl = plan_fn(W, H, n, b, x, y, rw, rh, stats=ALL)
                assert {k: pl[k] for k in GEOMETRY} == {k: roi[k] for k in GEOMETRY}


def test_some_windows_are_rejected_and_some_accepted(dv):
    verdicts = []
    for (W, H, n, x, y, rw, rh) in WINDOWS:
        try:
            dv.roi_plan(W, H, n, x, y, rw, rh)
            verdicts.append(True)
        except ValueError:
            verdicts.append(False)
    assert verdicts.count(True) >= 3 and verdicts.count(False) >= 10, verdicts
