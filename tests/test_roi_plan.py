"""CPU: dbde_hip_roi_plan -- the tile window, index geometry and launch of a window decode, and the argument checks
dbde_hip_decode_roi shares with it.  Pure host arithmetic; no GPU."""
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


def expect(W, H, n, x, y, rw, rh):
    """The plan worked out independently from the format: 8x8 tiles, index chunks at every tile row."""
    w, h = (W + 7) // 8, (H + 7) // 8
    tx0, ty0 = x // 8, y // 8
    ntx, nty = (x + rw - 1) // 8 + 1 - tx0, (y + rh - 1) // 8 + 1 - ty0
    # the most any origin in [0, W-rw] x [0, H-rh] needs: brute force over the origins
    max_tx = max((ox + rw - 1) // 8 + 1 - ox // 8 for ox in range(0, min(W - rw, 15) + 1))
    max_ty = max((oy + rh - 1) // 8 + 1 - oy // 8 for oy in range(0, min(H - rh, 15) + 1))
    pieces = (w + 511) // 512
    if h * pieces <= 32768:
        cpf, ct, cp = h * pieces, (w if pieces == 1 else 512), pieces
    else:
        cpf, ct, cp = (w * h + 511) // 512, 512, (1 if w == 512 else 0)
    threads = 64 if max_tx <= 64 else 256
    px = (max_tx + threads - 1) // threads
    return dict(tile_x=tx0, tile_y=ty0, tiles_x=ntx, tiles_y=nty, max_tiles_x=max_tx, max_tiles_y=max_ty,
                chunks_per_frame=cpf, chunk_tiles=ct, chunk_pieces=cp, threads=threads, pieces_x=px,
                grid=n * nty * ((ntx + threads - 1) // threads), grid_origins=n * max_ty * px)


CASES = [
    # (W, H, n, x, y, rw, rh)
    (4096, 3072, 1024, 1000, 700, 256, 256),   # tile-aligned origin
    (4096, 3072, 1024, 1003, 701, 256, 256),   # unaligned: one more tile each way
    (4096, 3072, 1024, 0, 0, 4096, 3072),      # full frame
    (4096, 3072, 1, 1000, 700, 512, 512),
    (1921, 1081, 7, 1920, 1080, 1, 1),         # one pixel in the right / bottom partial tile
    (1921, 1081, 7, 1913, 1073, 8, 8),         # the last whole tile and the partial ones
    (1921, 1081, 7, 1, 1, 1920, 1080),         # touches the right and bottom edges
    (1920, 1080, 3, 5, 9, 1, 1),
    (720, 1283, 2, 3, 1275, 717, 8),
    (8200, 9, 4, 0, 0, 8200, 9),               # 1025 tiles across: three 512-tile index pieces per row
    (8200, 9, 4, 4090, 0, 20, 9),              # a window across the 512-tile piece boundary (column 4096)
    (8200, 9, 4, 4095, 1, 2, 1),
    (513, 17, 5, 505, 9, 8, 8),
    (72, 72, 300, 0, 0, 72, 72),
    (10, 10, 1, 9, 9, 1, 1),
    (1, 1, 1, 0, 0, 1, 1),
    (8, 300000, 1, 0, 299992, 8, 8),           # 37,500 tile rows: more than the index's 32,768 chunks -> plain chunks
    (4096, 8, 1, 0, 0, 2049, 1),               # 257 tiles across: two 256-tile workgroups per tile row
]


@pytest.mark.parametrize("W,H,n,x,y,rw,rh", CASES)
def test_plan_geometry(dv, W, H, n, x, y, rw, rh):
    got = dv.roi_plan(W, H, n, x, y, rw, rh)
    want = expect(W, H, n, x, y, rw, rh)
    for k, v in want.items():
        assert got[k] == v, (k, got[k], v)
    # the index split follows dbde_hip_decode_frames: few frames with >= 8 chunks are cut into pieces
    cpf = want["chunks_per_frame"]
    split = 1 if (n >= 256 or cpf < 8) else max(1, min(1024 // n, (cpf + 3) // 4))
    assert got["index_split"] == split


def test_plan_examples_pinned(dv):
    """A few plans spelled out, so that a change of the launch shape is a visible diff."""
    p = dv.roi_plan(4096, 3072, 1024, 1000, 700, 256, 256)
    assert (p["tile_x"], p["tile_y"], p["tiles_x"], p["tiles_y"]) == (125, 87, 32, 33)
    assert (p["max_tiles_x"], p["max_tiles_y"], p["threads"], p["pieces_x"]) == (33, 33, 64, 1)
    assert (p["chunks_per_frame"], p["chunk_tiles"], p["chunk_pieces"], p["index_split"]) == (384, 512, 1, 1)
    assert (p["grid"], p["grid_origins"]) == (1024 * 33, 1024 * 33)
    p = dv.roi_plan(4096, 3072, 1, 0, 0, 4096, 3072)
    assert (p["tiles_x"], p["max_tiles_x"], p["threads"], p["pieces_x"], p["grid"]) == (512, 512, 256, 2, 384 * 2)
    assert p["index_split"] == 96
    p = dv.roi_plan(8200, 9, 4, 4090, 0, 20, 9)
    assert (p["tile_x"], p["tiles_x"], p["chunks_per_frame"], p["chunk_tiles"], p["chunk_pieces"]) == (511, 3, 6, 512, 3)
    p = dv.roi_plan(1, 1, 1, 0, 0, 1, 1)
    assert (p["tiles_x"], p["tiles_y"], p["max_tiles_x"], p["max_tiles_y"], p["grid"]) == (1, 1, 1, 1, 1)
    p = dv.roi_plan(8, 300000, 1, 0, 0, 8, 8)
    assert (p["chunks_per_frame"], p["chunk_tiles"], p["chunk_pieces"]) == (74, 512, 0)
    assert dv.roi_plan(72, 72, 0, 0, 0, 8, 8)["grid"] == 0   # n_frames == 0: nothing to launch


@pytest.mark.parametrize("args", [
    (64, 64, 1, 0, 0, 0, 8),          # rw = 0
    (64, 64, 1, 0, 0, 8, 0),          # rh = 0
    (64, 64, 1, 0, 0, 65, 8),         # rw > W
    (64, 64, 1, 0, 0, 8, 65),         # rh > H
    (64, 64, 1, -1, 0, 8, 8),         # negative origin
    (64, 64, 1, 0, -8, 8, 8),
    (64, 64, 1, 57, 0, 8, 8),         # x + rw > W
    (64, 64, 1, 0, 60, 8, 8),         # y + rh > H
    (64, 64, 1, 2 ** 31 - 1, 0, 8, 8),   # origins whose end overflows an int
    (64, 64, 1, 0, 2 ** 31 - 8, 8, 8),
    (64, 64, -1, 0, 0, 8, 8),         # n < 0
    (0, 64, 1, 0, 0, 1, 1),           # bad frame
    (64, -1, 1, 0, 0, 1, 1),
    (-5, 64, 1, 0, 0, 1, 1),
    (40000, 40000, 1, 0, 0, 8, 8),    # 25,000,000 tiles: more than 32,768 index chunks even of 512 tiles
])
def test_plan_rejects(dv, args):
    with pytest.raises(ValueError):
        dv.roi_plan(*args)


def test_decode_roi_argument_errors_without_a_device(dv):
    """dbde_hip_decode_roi with a null context is DBDE_HIP_ERR_ARG before anything touches a device;
    the host-pointer form returns 0."""
    L = dv.lib()
    assert L.dbde_hip_decode_roi(None, None, 0, None, 64, 64, 1, 0, 0, 8, 8, None, None, None) == dv.ERR_ARG
    assert L.dbde_hip_unpack_image_roi(None, None, 64, 64, 0, 0, 8, 8, None) == 0

