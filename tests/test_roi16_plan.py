"""CPU: dbde16_hip_roi_plan -- the tile window, index geometry and launch of a DBDE16 window decode, and the argument
checks dbde16_hip_decode_roi shares with it.  Pure host arithmetic; no GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WIDE16 = 128   # tiles per workgroup of 16-bit windows more than 64 tiles across


@pytest.fixture(scope="module")
def dv():
    import dbde_video_cpp_amd as m
    if not os.path.exists(m.LIB_PATH):
        m.build()
    return m


def expect(W, H, n, x, y, rw, rh):
    """The plan worked out independently from the format: 8x8 tiles, index chunks at every tile row."""
    w, h = (W + 7) // 8, (H + 7) // 8
    tx0, ty0 = x // 8, y // 8
    ntx, nty = (x + rw - 1) // 8 + 1 - tx0, (y + rh - 1) // 8 + 1 - ty0
    max_tx = max((ox + rw - 1) // 8 + 1 - ox // 8 for ox in range(0, min(W - rw, 15) + 1))
    max_ty = max((oy + rh - 1) // 8 + 1 - oy // 8 for oy in range(0, min(H - rh, 15) + 1))
    pieces = (w + 511) // 512
    if h * pieces <= 32768:
        cpf, ct, cp = h * pieces, (w if pieces == 1 else 512), pieces
    else:
        cpf, ct, cp = (w * h + 511) // 512, 512, (1 if w == 512 else 0)
    threads = 64 if max_tx <= 64 else WIDE16
    px = (max_tx + threads - 1) // threads
    split = 1 if (n >= 256 or cpf < 8) else max(1, min(1024 // n, (cpf + 3) // 4))
    return dict(tile_x=tx0, tile_y=ty0, tiles_x=ntx, tiles_y=nty, max_tiles_x=max_tx, max_tiles_y=max_ty,
                chunks_per_frame=cpf, chunk_tiles=ct, chunk_pieces=cp, index_split=split, threads=threads,
                pieces_x=px, grid=n * nty * ((ntx + threads - 1) // threads), grid_origins=n * max_ty * px)


CASES = [
    # (W, H, n, x, y, rw, rh)
    (4096, 3072, 128, 1000, 700, 256, 256),
    (4096, 3072, 128, 1003, 701, 256, 256),
    (4096, 3072, 128, 0, 0, 4096, 3072),
    (4096, 3072, 1, 1000, 700, 512, 512),
    (4096, 3072, 128, 1000, 700, 1024, 1024),
    (1921, 1081, 7, 1920, 1080, 1, 1),
    (1921, 1081, 7, 1, 1, 1920, 1080),
    (8200, 9, 4, 0, 0, 8200, 9),
    (8200, 9, 4, 4090, 0, 20, 9),
    (4104, 16, 2, 0, 0, 4104, 16),
    (4096, 8, 1, 0, 0, 1025, 1),               # 129 tiles across: two 128-tile workgroups per tile row
    (33, 31, 3, 5, 7, 20, 20),
    (1, 1, 1, 0, 0, 1, 1),
    (8, 300000, 1, 0, 299992, 8, 8),
]


@pytest.mark.parametrize("W,H,n,x,y,rw,rh", CASES)
def test_plan16_geometry(dv, W, H, n, x, y, rw, rh):
    got = dv.roi16_plan(W, H, n, x, y, rw, rh)
    want = expect(W, H, n, x, y, rw, rh)
    assert got == want
    # the tile window and the index are the 8-bit plan's; only the window kernel's piece width may differ
    p8 = dv.roi_plan(W, H, n, x, y, rw, rh)
    same = ("tile_x", "tile_y", "tiles_x", "tiles_y", "max_tiles_x", "max_tiles_y", "chunks_per_frame", "chunk_tiles",
            "chunk_pieces", "index_split")
    assert {k: got[k] for k in same} == {k: p8[k] for k in same}
    if got["max_tiles_x"] <= 64:
        assert got == p8


def test_plan16_examples_pinned(dv):
    """The plans the issue names, spelled out, so that a change of the launch shape is a visible diff."""
    p = dv.roi16_plan(4096, 3072, 1024, 1000, 700, 256, 256)
    assert (p["tile_x"], p["tile_y"], p["tiles_x"], p["tiles_y"]) == (125, 87, 32, 33)
    assert (p["max_tiles_x"], p["max_tiles_y"], p["threads"], p["pieces_x"]) == (33, 33, 64, 1)
    assert (p["chunks_per_frame"], p["chunk_tiles"], p["chunk_pieces"], p["index_split"]) == (384, 512, 1, 1)
    assert (p["grid"], p["grid_origins"]) == (1024 * 33, 1024 * 33)
    p = dv.roi16_plan(4096, 3072, 1, 0, 0, 4096, 3072)
    assert (p["tiles_x"], p["max_tiles_x"], p["threads"], p["pieces_x"], p["grid"]) == (512, 512, 128, 4, 384 * 4)
    assert p["index_split"] == 96
    p = dv.roi16_plan(8200, 9, 4, 0, 0, 8200, 9)
    assert (p["tiles_x"], p["tiles_y"], p["chunks_per_frame"], p["chunk_tiles"], p["chunk_pieces"]) == (1025, 2, 6, 512, 3)
    assert (p["threads"], p["pieces_x"], p["grid"], p["grid_origins"]) == (128, 9, 4 * 2 * 9, 4 * 2 * 9)
    p = dv.roi16_plan(1, 1, 1, 0, 0, 1, 1)
    assert (p["tiles_x"], p["tiles_y"], p["max_tiles_x"], p["max_tiles_y"], p["threads"], p["grid"]) == (1, 1, 1, 1, 64, 1)
    p = dv.roi16_plan(8, 300000, 1, 0, 0, 8, 8)
    assert (p["chunks_per_frame"], p["chunk_tiles"], p["chunk_pieces"]) == (74, 512, 0)
    p = dv.roi16_plan(72, 72, 0, 0, 0, 8, 8)
    assert (p["grid"], p["grid_origins"]) == (0, 0)   # n_frames == 0: nothing to launch


def test_plan8_unchanged_by_the_16bit_form(dv):
    """dbde_hip_roi_plan keeps 256-tile pieces for wide windows."""
    p = dv.roi_plan(4096, 3072, 1, 0, 0, 4096, 3072)
    assert (p["threads"], p["pieces_x"], p["grid"]) == (256, 2, 384 * 2)


@pytest.mark.parametrize("args", [
    (64, 64, 1, 0, 0, 0, 8),          # rw = 0
    (64, 64, 1, 0, 0, 8, 0),          # rh = 0
    (64, 64, 1, 0, 0, 65, 8),         # rw > W
    (64, 64, 1, 0, 0, 8, 65),         # rh > H
    (64, 64, 1, -1, 0, 8, 8),         # negative origin
    (64, 64, 1, 0, -8, 8, 8),
    (64, 64, 1, 57, 0, 8, 8),         # x + rw > W
    (64, 64, 1, 0, 60, 8, 8),         # y + rh > H
    (64, 64, 1, 2 ** 31 - 1, 0, 8, 8),
    (64, 64, 1, 0, 2 ** 31 - 8, 8, 8),
    (64, 64, -1, 0, 0, 8, 8),         # n < 0
    (0, 64, 1, 0, 0, 1, 1),           # bad frame
    (64, -1, 1, 0, 0, 1, 1),
    (40000, 40000, 1, 0, 0, 8, 8),    # more than 32,768 index chunks even of 512 tiles
])
def test_plan16_rejects(dv, args):
    with pytest.raises(ValueError):
        dv.roi16_plan(*args)


def test_decode_roi16_argument_errors_without_a_device(dv):
    """dbde16_hip_decode_roi with a null context, or with null pointers, is DBDE_HIP_ERR_ARG before anything touches a
    device; so is a null plan."""
    L = dv.lib()
    assert L.dbde16_hip_decode_roi(None, None, 0, None, 64, 64, 1, 0, 0, 8, 8, None, None, None) == dv.ERR_ARG
    assert L.dbde16_hip_decode_roi(None, None, 0, None, 64, 64, 0, 0, 0, 8, 8, None, None, None) == dv.ERR_ARG
    assert L.dbde16_hip_roi_plan(64, 64, 1, 0, 0, 8, 8, None) == dv.ERR_ARG
