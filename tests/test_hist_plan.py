"""CPU: dbde_hip_histogram_plan / dbde16_hip_histogram_plan (pure host arithmetic, no GPU).

The plans validate exactly what the histogram calls validate: the window rules of dbde_hip_decode_roi, the bins /
shift rules of each format and at least one output.  The tile window and index geometry are dbde_hip_roi_plan's; the
launch, LDS and workspace figures follow DESIGN.md 4.9.
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


PLANS = {1: "histogram_plan", 2: "histogram16_plan"}
ROI = {1: "roi_plan", 2: "roi16_plan"}


def plan(dv, pix, *a, **kw):
    return getattr(dv, PLANS[pix])(*a, **kw)


@pytest.mark.parametrize("pix", (1, 2))
def test_bins_and_shift_rules_at_each_boundary(dv, pix):
    top = 8 * pix - 1
    for shift in range(0, top + 1):
        most = dv.max_bins(pix, shift)
        assert most == ((256 >> shift) if pix == 1 else min(4096, 65536 >> shift))
        for bins in (1, most):
            assert plan(dv, pix, 64, 48, 3, shift=shift, bins=bins)["segments"] >= 1
        for bins in (0, most + 1, -1):
            with pytest.raises(ValueError):
                plan(dv, pix, 64, 48, 3, shift=shift, bins=bins)
    for shift in (-1, top + 1):
        with pytest.raises(ValueError):
            plan(dv, pix, 64, 48, 3, shift=shift, bins=1)


def test_bins_default_to_the_most(dv):
    assert plan(dv, 1, 64, 48, 3)["lds_bins"] == 256
    assert plan(dv, 2, 64, 48, 3)["lds_bins"] == 4096
    assert plan(dv, 2, 64, 48, 3, shift=8)["lds_bins"] == 256          # 65536 >> 8 = 256 bins
    assert plan(dv, 2, 64, 48, 3, shift=4, bins=4096)["lds_bins"] == 4096
    assert plan(dv, 2, 64, 48, 3, bins=257)["lds_bins"] == 4096


@pytest.mark.parametrize("pix", (1, 2))
def test_window_rules(dv, pix):
    W, H = 200, 123
    for args in [(0, 0, W, H), (W - 1, H - 1, 1, 1), (3, 5, W - 3, H - 5), (0, 0, 1, H)]:
        plan(dv, pix, W, H, 2, *args)
    for args in [(0, 0, W + 1, H), (0, 0, W, H + 1), (0, 0, 0, H), (0, 0, W, 0), (-1, 0, W, H), (1, 0, W, H),
                 (0, 1, W, H), (W, 0, 1, 1)]:
        with pytest.raises(ValueError):
            plan(dv, pix, W, H, 2, *args)
    for bad in [(0, H), (W, 0), (-8, H)]:
        with pytest.raises(ValueError):
            plan(dv, pix, bad[0], bad[1], 2, 0, 0, 1, 1)
    with pytest.raises(ValueError):
        plan(dv, pix, W, H, -1)
    with pytest.raises(ValueError):   # more than 32768 index chunks
        plan(dv, pix, 40000, 40000, 1, 0, 0, 8, 8)


@pytest.mark.parametrize("pix", (1, 2))
def test_no_output_is_an_error(dv, pix):
    with pytest.raises(ValueError):
        plan(dv, pix, 64, 48, 3, per_frame=False, total=False)
    a = plan(dv, pix, 64, 48, 3, per_frame=False, total=True)
    b = plan(dv, pix, 64, 48, 3, per_frame=True, total=True)
    c = plan(dv, pix, 64, 48, 3)
    assert 2 * a["global_atomics_per_frame"] == b["global_atomics_per_frame"] == 2 * c["global_atomics_per_frame"]


@pytest.mark.parametrize("pix", (1, 2))
@pytest.mark.parametrize("W,H,n,win", [(200, 123, 7, (0, 0, 200, 123)), (1921, 1081, 5, (3, 7, 1000, 500)),
                                       (4096, 3072, 1024, (0, 0, 4096, 3072)), (4096, 3072, 1024, (1001, 999, 256, 256)),
                                       (4200, 24, 5, (4090, 1, 110, 23)), (8, 262152, 2, (0, 0, 8, 262152)),
                                       (1, 1, 3, (0, 0, 1, 1))])
def test_geometry_equals_roi_plan(dv, pix, W, H, n, win):
    x, y, rw, rh = win
    h = plan(dv, pix, W, H, n, x, y, rw, rh)
    r = getattr(dv, ROI[pix])(W, H, n, x, y, rw, rh)
    for k in ("tile_x", "tile_y", "tiles_x", "tiles_y", "chunks_per_frame", "chunk_tiles", "chunk_pieces",
              "index_split"):
        assert h[k] == r[k], k


@pytest.mark.parametrize("pix", (1, 2))
def test_launch_and_workspace_figures(dv, pix):
    tiles = 32 // pix
    for (W, H, n, win, n_cu) in [(4096, 3072, 1024, (0, 0, 4096, 3072), 256), (4096, 3072, 4, (0, 0, 4096, 3072), 256),
                                 (4096, 3072, 1024, (1001, 999, 256, 256), 256), (200, 123, 7, (5, 3, 131, 77), 8),
                                 (1, 1, 3, (0, 0, 1, 1), 256), (4096, 3072, 0, (0, 0, 4096, 3072), 256)]:
        x, y, rw, rh = win
        for bins in (1, 200, dv.max_bins(pix)):
            h = plan(dv, pix, W, H, n, x, y, rw, rh, bins=bins, total=True, n_cu=n_cu)
            assert h["threads"] == 256 and h["tiles_per_piece"] == tiles
            assert h["pieces_x"] == -(-h["tiles_x"] // tiles)
            assert h["pieces"] == h["pieces_x"] * h["tiles_y"]
            seg, pps = h["segments"], h["pieces_per_segment"]
            assert 1 <= seg and (seg - 1) * pps < h["pieces"] <= seg * pps        # no empty segment
            min_pieces = max(16, -(-64 * bins // (64 * tiles)))
            assert seg <= max(1, -(-h["pieces"] // min_pieces))                      # segments of >= 64 * bins pixels
            assert seg <= max(1, -(-16 * n_cu // max(n, 1)))
            assert h["grid"] == n * seg
            assert h["init_grid"] == -(-max(n, 1) * bins // 256)
            assert h["global_atomics_per_frame"] == 2 * seg * bins
            lds_bins = 256 if bins <= 256 else 4096
            copies = 4 if lds_bins == 256 else 1
            assert (h["lds_bins"], h["lds_copies"]) == (lds_bins, copies)
            assert h["lds_bytes"] == 4 * copies * lds_bins + 256
            assert h["workspace_bytes"] == n * 4 * (h["chunks_per_frame"] + 1) + 4 * n
    big = plan(dv, pix, 4096, 3072, 1024)
    assert big["segments"] == 4 and big["grid"] == 4096     # 16 workgroups per CU over 1,024 frames
    few = plan(dv, pix, 4096, 3072, 2)
    min_pieces = max(16, -(-64 * dv.max_bins(pix) // (64 * tiles)))
    assert few["segments"] == min(2048, -(-few["pieces"] // min_pieces))   # 16 per CU, but >= 64 * bins pixels each
