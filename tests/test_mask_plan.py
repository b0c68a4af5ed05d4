"""CPU: dbde_hip_mask_plan / dbde16_hip_mask_plan (host arithmetic) against a restatement in Python.

A mask row is words = ceil(rw / 64) U64 words.  Pieces are cut in WINDOW coordinates: a workgroup of `threads` threads
(one tile per thread) owns whole words, and 64 k window pixels overlap at most 8 k + 1 tiles at any x mod 8, so with
per-frame origins a piece has at most threads / 8 - 1 words; at a fixed x0 that is a multiple of 8, threads / 8 words are
exactly `threads` tiles.  The words are spread evenly over the fewest pieces.  Windows of at most 7 words take 64 threads,
wider ones 256 (DBDE16: 128).
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


def ceil_div(a, b):
    return -(-a // b)


def restated(pix, W, H, n, x, y, rw, rh):
    words = ceil_div(rw, 64)
    threads = 64 if words <= 7 else (256 if pix == 1 else 128)
    cap = threads // 8 - 1
    cap_fixed = threads // 8 if x % 8 == 0 else cap
    pieces, pieces_fixed = ceil_div(words, cap), ceil_div(words, cap_fixed)
    nty = (y + rh - 1) // 8 + 1 - y // 8
    max_ty = (min(7, H - rh) + rh + 7) // 8
    pay = threads * 64 + 64 if pix == 1 else threads * 128 + 32
    need = (4 * pix * threads + 1 + 31) // 32 + 1
    waves = threads // 64
    return dict(words=words, threads=threads, pieces_x=pieces, piece_words=ceil_div(words, pieces),
                pieces_x_fixed=pieces_fixed, piece_words_fixed=ceil_div(words, pieces_fixed),
                grid=n * nty * pieces_fixed, grid_origins=n * max_ty * pieces, mask_bytes=n * rh * words * 8,
                lds_bytes=(pay + 8 * waves + 4 * need + 20 * waves + 15) // 16 * 16)


CASES = [(1, 1, 1, 0, 0, 1, 1), (8, 8, 3, 0, 0, 8, 8), (200, 123, 7, 5, 3, 63, 20), (200, 123, 7, 6, 3, 64, 20),
         (200, 123, 7, 7, 9, 65, 100), (200, 123, 2, 64, 0, 129, 123), (1921, 1081, 2, 0, 0, 1921, 1081),
         (1921, 1081, 2, 9, 8, 449, 17), (4200, 24, 1, 3, 1, 4190, 20), (4096, 3072, 4, 0, 0, 4096, 3072),
         (4096, 3072, 4, 8, 8, 4080, 16), (4096, 3072, 4, 4, 0, 4090, 3072), (4096, 3072, 1, 1024, 1024, 1024, 1024),
         (4096, 3072, 1, 77, 5, 448, 9), (4096, 3072, 1, 77, 5, 449, 9), (4096, 3072, 1, 80, 5, 512, 9)]


@pytest.mark.parametrize("pix", [1, 2])
@pytest.mark.parametrize("W,H,n,x,y,rw,rh", CASES)
def test_plan_matches_the_restatement(dv, pix, W, H, n, x, y, rw, rh):
    plan = (dv.mask_plan if pix == 1 else dv.mask16_plan)(W, H, n, x, y, rw, rh)
    roi = (dv.roi_plan if pix == 1 else dv.roi16_plan)(W, H, n, x, y, rw, rh)
    want = restated(pix, W, H, n, x, y, rw, rh)
    for k, v in want.items():
        assert plan[k] == v, (k, plan[k], v)
    for k in ("tile_x", "tile_y", "tiles_x", "tiles_y", "max_tiles_x", "max_tiles_y", "chunks_per_frame", "chunk_tiles",
              "chunk_pieces", "index_split"):
        assert plan[k] == roi[k], k


@pytest.mark.parametrize("pix", [1, 2])
@pytest.mark.parametrize("rw", [1, 63, 64, 65, 129, 448, 449, 1985, 2000, 4088])
def test_pieces_hold_whole_words_and_their_tiles_fit_for_every_x_mod_8(dv, pix, rw):
    """The words of a piece and the tiles they overlap, restated: every word belongs to exactly one piece, and at every
    x mod 8 a piece's tiles are at most one per thread."""
    W, H = 4096, 64
    for x in range(8):
        plan = (dv.mask_plan if pix == 1 else dv.mask16_plan)(W, H, 1, x, 0, rw, 9)
        for fixed in (False, True):
            pw = plan["piece_words_fixed" if fixed else "piece_words"]
            pieces = plan["pieces_x_fixed" if fixed else "pieces_x"]
            assert (pieces - 1) * pw < plan["words"] <= pieces * pw
            for xm in ([x] if fixed else range(x, x + 8)):   # origins: any residue
                for pc in range(pieces):
                    c0, c1 = 64 * pw * pc, min(rw, 64 * pw * (pc + 1))
                    tiles = (xm + c1 - 1) // 8 - (xm + c0) // 8 + 1
                    assert 1 <= tiles <= plan["threads"], (x, xm, pc, tiles)
    wide = (dv.mask_plan if pix == 1 else dv.mask16_plan)(W, H, 1, 3, 0, 4088, 9)
    assert wide["pieces_x"] > 1 and wide["threads"] == (256 if pix == 1 else 128)


@pytest.mark.parametrize("pix", [1, 2])
def test_argument_rules(dv, pix):
    plan = dv.mask_plan if pix == 1 else dv.mask16_plan
    assert plan(64, 48, 0)["mask_bytes"] == 0 and plan(64, 48, 0)["grid"] == 0
    assert plan(64, 48, 2) == plan(64, 48, 2, 0, 0, 64, 48)   # rw / rh default to the rest of the frame
    for bad in ((64, 48, -1), (0, 48, 1), (64, 0, 1), (64, 48, 1, 0, 0, 0, 48), (64, 48, 1, 0, 0, 64, 0),
                (64, 48, 1, 0, 0, 65, 48), (64, 48, 1, 0, 0, 64, 49), (64, 48, 1, -1, 0, 8, 8), (64, 48, 1, 0, -1, 8, 8),
                (64, 48, 1, 57, 0, 8, 8), (64, 48, 1, 0, 41, 8, 8), (64, 48, 1 << 30, 0, 0, 64, 48)):
        with pytest.raises(ValueError):
            plan(*bad)
    fn = dv.lib().dbde_hip_mask_plan if pix == 1 else dv.lib().dbde16_hip_mask_plan
    assert fn(64, 48, 1, 0, 0, 64, 48, None) == dv.ERR_ARG
