"""CPU: dbde_hip_crop_plan / dbde16_hip_crop_plan (host arithmetic of the C-ABI, no GPU) against Python arithmetic."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REC = 144   # bytes of a re-packed tile's record (128 payload, depth, minimum, word offset, pad)


@pytest.fixture(scope="module")
def dv():
    import dbde_video_cpp_amd as m
    if not os.path.exists(m.LIB_PATH):
        m.build()
    return m


def ceil8(v):
    return (v + 7) // 8


def max_frame(rw, rh, bits):
    return 32 + (66 if bits == 8 else 131) * ceil8(rw) * ceil8(rh)


def index_geometry(W, H):
    """(chunks_per_frame, chunk_tiles, chunk_pieces) of roi_index_geometry."""
    w, h = ceil8(W), ceil8(H)
    pieces = (w + 511) // 512
    if h * pieces <= 32768:
        return h * pieces, (w if pieces == 1 else 512), pieces
    return (w * h + 511) // 512, 512, 0


def index_split(n, cpf):
    if n < 1 or n >= 256 or cpf < 8:
        return 1
    return max(1, min(1024 // n, (cpf + 3) // 4))


def recoded(W, H, x, y, rw, rh):
    ntx, nty = ceil8(rw), ceil8(rh)
    cut_col = rw - 8 * (ntx - 1) != min(8, W - 8 * (x // 8 + ntx - 1))
    cut_row = rh - 8 * (nty - 1) != min(8, H - 8 * (y // 8 + nty - 1))
    return (ntx if cut_row else 0) + (nty if cut_col else 0) - (1 if cut_row and cut_col else 0)


CASES = [  # W, H, n, x, y, rw, rh
    (4096, 3072, 1024, 1000, 696, 256, 256),      # narrow: at most 64 tiles across
    (4096, 3072, 1024, 1000, 696, 2045, 2043),    # wide, both edges cut tiles
    (4096, 3072, 3, 0, 0, 4096, 3072),            # the frame
    (1921, 1081, 7, 8, 16, 1913, 1065),           # ends on the frame's own partial edge: nothing re-packed
    (1921, 1081, 7, 8, 16, 1912, 1064),           # ends on tile boundaries
    (1921, 1081, 7, 1912, 1080, 9, 1),            # the corner tile alone
    (8200, 24, 5, 0, 0, 8200, 24),                # more than 512 tiles across
    (8200, 24, 5, 4088, 8, 4100, 9),
    (64, 64, 300, 8, 8, 33, 47),
    (1, 1, 1, 0, 0, 1, 1),
]


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("W,H,n,x,y,rw,rh", CASES)
def test_plan_matches_python_arithmetic(dv, bits, W, H, n, x, y, rw, rh):
    plan = dv.crop_plan if bits == 8 else dv.crop16_plan
    ntx, nty = ceil8(rw), ceil8(rh)
    cpf, ct, pieces = index_geometry(W, H)
    mx = max_frame(rw, rh, bits)
    for stride in (0, mx, mx + 12345):
        p = plan(W, H, n, x, y, rw, rh, slot_stride=stride)
        rows = n * nty
        want = dict(tile_x=x // 8, tile_y=y // 8, tiles_x=ntx, tiles_y=nty, out_tiles=ntx * nty,
                    recoded_tiles=recoded(W, H, x, y, rw, rh), chunks_per_frame=cpf, chunk_tiles=ct, chunk_pieces=pieces,
                    index_split=index_split(n, cpf), size_threads=256, rows_threads=256, place_threads=256,
                    copy_threads=256, repack_threads=256,
                    repack_grid=n * ((ntx + nty - 1 + 255) // 256) if recoded(W, H, x, y, rw, rh) else 0,
                    size_grid=rows, rows_grid=n, place_grid=1, copy_grid=rows, max_out_frame_bytes=mx,
                    out_capacity=(n - 1) * stride + mx if stride else n * mx,
                    workspace_bytes=(12 * rows + 15) // 16 * 16 + 16 * n + n * (ntx + nty - 1) * REC)
        assert {k: p[k] for k in want} == want


def test_recoded_tiles_for_aligned_cut_and_frame_edge_extents(dv):
    W, H = 333, 77    # 42 x 10 tiles, the last column 5 pixels wide, the last row 5 pixels high
    assert dv.crop_plan(W, H, 1, 8, 8, 64, 40)["recoded_tiles"] == 0          # tile boundaries
    assert dv.crop_plan(W, H, 1, 8, 8, 325, 69)["recoded_tiles"] == 0         # the frame's own edge
    assert dv.crop_plan(W, H, 1, 0, 0, W, H)["recoded_tiles"] == 0
    assert dv.crop_plan(W, H, 1, 8, 8, 60, 40)["recoded_tiles"] == 5          # the right edge cuts a column of 5 tiles
    assert dv.crop_plan(W, H, 1, 8, 8, 64, 37)["recoded_tiles"] == 8          # the bottom edge cuts a row of 8 tiles
    assert dv.crop_plan(W, H, 1, 8, 8, 60, 37)["recoded_tiles"] == 8 + 5 - 1
    assert dv.crop_plan(W, H, 1, 320, 72, 13, 5)["recoded_tiles"] == 0        # a tile and the edge tile's 5 valid columns
    assert dv.crop_plan(W, H, 1, 320, 72, 12, 5)["recoded_tiles"] == 1        # one column less: cut inside the edge tile
    assert dv.crop16_plan(W, H, 1, 8, 8, 60, 37)["recoded_tiles"] == 12


def test_capacity_of_no_frames(dv):
    p = dv.crop_plan(640, 480, 0, 0, 0, 100, 100)
    assert (p["out_capacity"], p["size_grid"], p["place_grid"]) == (0, 0, 0)


@pytest.mark.parametrize("bits", [8, 16])
def test_every_argument_rule(dv, bits):
    plan = dv.crop_plan if bits == 8 else dv.crop16_plan
    W, H = 640, 480
    plan(W, H, 4, 8, 16, 100, 100)
    for bad in [(4, 16, 100, 100), (8, 12, 100, 100), (-8, 0, 100, 100), (0, -8, 100, 100),      # origin not on the grid
                (544, 0, 100, 100), (0, 384, 100, 100), (0, 0, 641, 10), (0, 0, 10, 481),       # outside the frame
                (0, 0, 0, 10), (0, 0, 10, 0)]:
        with pytest.raises(ValueError):
            plan(W, H, 4, *bad)
    with pytest.raises(ValueError):
        plan(W, H, -1, 0, 0, 100, 100)
    with pytest.raises(ValueError):
        plan(0, H, 1, 0, 0, 1, 1)
    mx = max_frame(100, 100, bits)
    with pytest.raises(ValueError):
        plan(W, H, 4, 0, 0, 100, 100, slot_stride=mx - 1)            # below the cropped frame's worst case
    plan(W, H, 4, 0, 0, 100, 100, slot_stride=mx)
    # more than 32,768 index chunks: plain 512-tile chunks no longer fit either
    with pytest.raises(ValueError):
        plan(8 * 513, 8 * 40000, 1, 0, 0, 8, 8)
    assert plan(8 * 512, 8 * 32768, 1, 0, 0, 8, 8)["chunks_per_frame"] == 32768
