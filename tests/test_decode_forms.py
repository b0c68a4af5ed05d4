"""CPU: the coverage table of the crafted-stream decoder tests, and the proof that it misses no decoder form.

DECODE_CASES is the contract between this file and tests/test_gpu_decode_forms.py, which runs every row on the device:
(W, H, n, placement of the frames (crafted.layout), image address residue, form), form = the (kernel, image_mode,
index_mode, threads) that dv.decode_plan (host arithmetic only, the function dbde_hip_decode_frames itself calls)
reports for the row on 256 CUs.

A cell is a code path whose edge-tile arithmetic is its own on the right margin rm = W mod 8 (8 for whole tiles).  The
plan does not report every selector; the others were read off the dispatch (dbde_hip_decode_frames in dbde_capi.cpp, the
launchers and decode_kernel in dbde_kernels.hip) and are restated here from the geometry and the image address:

  * kernel 3 (decode_mid_kernel<THREADS, STAGED>): cell ("mid", threads, staged, rm).  threads is the plan's
    (mid_decode_threads_for); launch_decode_mid takes the staged instance (pixels through LDS, 16-byte stores) when
    `p.W % 4 == 0` and the image base is a multiple of 4 -- its line `const bool staged = ...`;
  * kernel 0 (decode_kernel<IMG, INDEX, THREADS>): cell ("chunk", path, threads, rm).  threads is the plan's
    (launch_decode: 192 for whole-tile-row chunks of at most 384 tiles).  path:
      - image_mode 0 (kImgDirect): "direct128" when W % 128 == 0 (plan_decode's first choice, whole cache lines per
        wave, where the image base is a multiple of 128 too, as in every row of the table; at a base of 16 mod 128,
        which the scan visits, such a width comes through plan_decode's last `if` and runs the same instance), else
        "direct16" (plan_decode's last `if`: the 16-byte fallback of the tile-by-tile form);
      - image_mode 1 (kImgLinear), by the copy-out decode_kernel takes: "staged16" where W and the frame's address are
        multiples of 16 (`if (whole_rows && ((img & 15) | (Wu & 15)) == 0 && chunk_words != 8 * n_tiles)`: stores from
        the registers unless the chunk is all of depth 8, then the a8 copy-out), "staged8" where they are multiples
        of 8 (`const bool a8 = ((g7 | Wu) & 7u) == 0u`), else "shifted" (the tile-aligned image at pitch 8 w + 16).
        W * H is a multiple of 8 (16) wherever W is, so every frame of a batch has the base's residue;
      - image_mode 2 (kImgTiles): "tiles".
  * the index of a chunk row (index_of) is the plan's self (1) or fused (2), or for the table (0) whether run_index
    launches the split form: "split" when index_split_for(n, chunks_per_frame) > 1, else "table".  index_split_for is
    restated below (split_for) and pinned against dv.roi_plan, which reports it for its own chunk geometry.

Every decoder cuts the rows below the frame, so every ("mid", threads, staged) and every (path, threads) also appears
with each bottom margin dm = H mod 8 (8 for whole tiles), with each index mode, and -- where image rows are not
aligned: "shifted", "tiles" and the unstaged mid decoder -- at image address residues 1, 2, 4 and 8 besides 0.
"""
import numpy as np
import pytest

import crafted as cr
import dbde_video_cpp_amd as dv

MID, CHUNK = 3, 0
DIRECT, STAGED, TILES = 0, 1, 2
TABLE, SELF, FUSED = 0, 1, 2
C, R, O = "concat", "residues", "offsets"      # crafted.layout: back to back | payloads, frames at every residue
MAX_TILES = 1_200_000                          # most tiles of one row, all frames together (77 MB of pixels)


@pytest.fixture(scope="module", autouse=True)
def built():
    dv.build()


# Self-indexed and fused rows hold three frames of at least three chunks (a first, a middle and a cut last chunk; the
# GPU test decodes as many streams as it takes to put the whole pool of crafted frames through them), the mid decoder
# 40 frames in seven groups and more (test_mid_rows_walk_the_pipelined_loop).  The table index takes launches of 1150
# chunks and more that are too large to index themselves: 256 frames and more for one workgroup per frame, fewer
# frames of eight chunks and more for the split form.
DECODE_CASES = [
    # ---- mid decoder, 256 threads, unstaged (every rm): one or two frames of 102 .. 134 tiles per workgroup
    (9, 402, 40, O, 0, (3, 0, 0, 256)), (10, 401, 40, C, 1, (3, 0, 0, 256)), (11, 532, 40, R, 4, (3, 0, 0, 256)),
    (12, 408, 40, O, 1, (3, 0, 0, 256)), (13, 534, 40, C, 8, (3, 0, 0, 256)), (14, 405, 40, R, 0, (3, 0, 0, 256)),
    (15, 531, 40, O, 2, (3, 0, 0, 256)), (16, 407, 40, C, 1, (3, 0, 0, 256)),
    # ---- mid decoder, 256 threads, staged (rm 4 and 8): groups that start at 4, 8 and 12 mod 16
    (12, 401, 40, O, 0, (3, 0, 0, 256)), (12, 530, 40, C, 0, (3, 0, 0, 256)), (12, 403, 40, R, 0, (3, 0, 0, 256)),
    (12, 532, 40, O, 4, (3, 0, 0, 256)), (12, 405, 40, C, 0, (3, 0, 0, 256)), (12, 534, 40, R, 0, (3, 0, 0, 256)),
    (12, 407, 40, O, 0, (3, 0, 0, 256)), (12, 408, 40, C, 8, (3, 0, 0, 256)), (24, 273, 40, R, 0, (3, 0, 0, 256)),
    # ---- mid decoder, 512 threads, unstaged (every rm)
    (65, 301, 40, C, 0, (3, 0, 0, 512)), (66, 297, 40, R, 4, (3, 0, 0, 512)), (67, 303, 40, O, 1, (3, 0, 0, 512)),
    (68, 304, 40, C, 1, (3, 0, 0, 512)), (69, 299, 40, R, 8, (3, 0, 0, 512)), (70, 300, 40, O, 0, (3, 0, 0, 512)),
    (71, 298, 40, C, 2, (3, 0, 0, 512)), (72, 302, 40, R, 1, (3, 0, 0, 512)),
    # ---- mid decoder, 512 threads, staged (rm 4 and 8)
    (68, 299, 40, O, 0, (3, 0, 0, 512)), (68, 303, 40, C, 0, (3, 0, 0, 512)), (68, 298, 40, R, 0, (3, 0, 0, 512)),
    (68, 300, 40, O, 0, (3, 0, 0, 512)), (68, 302, 40, C, 0, (3, 0, 0, 512)), (68, 297, 40, R, 0, (3, 0, 0, 512)),
    (68, 304, 40, O, 0, (3, 0, 0, 512)), (72, 301, 40, C, 4, (3, 0, 0, 512)),
    # ---- mid decoder, 1024 threads, unstaged (every rm)
    (1025, 14, 40, R, 0, (3, 0, 0, 1024)), (1026, 16, 40, O, 2, (3, 0, 0, 1024)),
    (1027, 11, 40, C, 4, (3, 0, 0, 1024)), (179, 181, 40, R, 1, (3, 0, 0, 1024)),
    (1028, 12, 40, R, 1, (3, 0, 0, 1024)), (1029, 13, 40, O, 0, (3, 0, 0, 1024)),
    (1030, 10, 40, C, 8, (3, 0, 0, 1024)), (1031, 15, 40, R, 0, (3, 0, 0, 1024)),
    (80, 201, 40, O, 1, (3, 0, 0, 1024)),
    # ---- mid decoder, 1024 threads, staged (rm 4 and 8)
    (1028, 10, 40, C, 0, (3, 0, 0, 1024)), (1028, 12, 40, R, 0, (3, 0, 0, 1024)),
    (1028, 14, 40, O, 0, (3, 0, 0, 1024)), (1028, 16, 40, C, 0, (3, 0, 0, 1024)),
    (1028, 11, 40, R, 0, (3, 0, 0, 1024)), (1028, 13, 40, O, 0, (3, 0, 0, 1024)),
    (1028, 15, 40, C, 0, (3, 0, 0, 1024)), (180, 178, 40, O, 0, (3, 0, 0, 1024)),
    (80, 201, 40, R, 4, (3, 0, 0, 1024)),
    # ---- chunk decoder, direct128, 256 threads: self, fused, split, table
    (256, 260, 3, C, 0, (0, 0, 1, 256)), (256, 262, 3, R, 0, (0, 0, 1, 256)), (256, 264, 3, O, 0, (0, 0, 1, 256)),
    (256, 261, 3, C, 0, (0, 0, 1, 256)), (256, 263, 3, R, 0, (0, 0, 1, 256)), (512, 1075, 3, O, 0, (0, 0, 2, 256)),
    (1920, 258, 72, C, 0, (0, 0, 0, 256)), (4096, 57, 257, R, 0, (0, 0, 0, 256)),
    # ---- chunk decoder, direct16, 256 threads: self, fused, split, table
    (2192, 28, 3, O, 0, (0, 0, 1, 256)), (2192, 30, 3, C, 0, (0, 0, 1, 256)), (2192, 32, 3, R, 0, (0, 0, 1, 256)),
    (2192, 29, 3, O, 0, (0, 0, 1, 256)), (2192, 31, 3, C, 0, (0, 0, 1, 256)), (2192, 259, 3, R, 0, (0, 0, 2, 256)),
    (2208, 202, 78, O, 0, (0, 0, 0, 256)), (2192, 113, 256, C, 0, (0, 0, 0, 256)),
    # ---- chunk decoder, staged16, 256 threads: self, fused, split, table
    (688, 84, 3, O, 0, (0, 1, 1, 256)), (688, 86, 3, C, 0, (0, 1, 1, 256)), (688, 88, 3, R, 0, (0, 1, 1, 256)),
    (688, 85, 3, O, 0, (0, 1, 1, 256)), (688, 87, 3, C, 0, (0, 1, 1, 256)), (272, 2003, 3, R, 0, (0, 1, 2, 256)),
    (688, 802, 55, O, 0, (0, 1, 0, 256)), (688, 345, 256, C, 0, (0, 1, 0, 256)),
    # ---- chunk decoder, staged8, 192 threads: self, fused, split, table
    (696, 72, 3, R, 0, (0, 1, 1, 192)), (696, 69, 3, O, 0, (0, 1, 1, 192)), (696, 71, 3, C, 0, (0, 1, 1, 192)),
    (696, 68, 3, R, 0, (0, 1, 1, 192)), (696, 70, 3, O, 0, (0, 1, 1, 192)), (1368, 403, 3, C, 0, (0, 1, 2, 192)),
    (1368, 498, 36, R, 0, (0, 1, 0, 192)), (696, 297, 256, O, 0, (0, 1, 0, 192)),
    # ---- chunk decoder, staged8, 256 threads: self, fused, split, table
    (688, 84, 3, C, 8, (0, 1, 1, 256)), (688, 86, 3, R, 8, (0, 1, 1, 256)), (688, 88, 3, O, 8, (0, 1, 1, 256)),
    (688, 85, 3, C, 8, (0, 1, 1, 256)), (688, 87, 3, R, 8, (0, 1, 1, 256)), (264, 2003, 3, O, 0, (0, 1, 2, 256)),
    (688, 802, 55, C, 8, (0, 1, 0, 256)), (688, 345, 256, R, 8, (0, 1, 0, 256)),
    # ---- chunk decoder, shifted, 192 threads, rm 1 .. 8 in order: split, self, table, fused
    (1361, 498, 36, R, 1, (0, 1, 0, 192)), (690, 69, 3, O, 8, (0, 1, 1, 192)), (683, 297, 257, C, 0, (0, 1, 0, 192)),
    (684, 803, 3, R, 2, (0, 1, 2, 192)), (685, 70, 3, O, 0, (0, 1, 1, 192)), (686, 72, 3, C, 0, (0, 1, 1, 192)),
    (687, 71, 3, R, 0, (0, 1, 1, 192)), (696, 68, 3, O, 4, (0, 1, 1, 192)),
    # ---- chunk decoder, shifted, 256 threads, rm 1 .. 8 in order: split, fused, self, table
    (513, 1074, 58, C, 0, (0, 1, 0, 256)), (258, 2003, 3, R, 2, (0, 1, 2, 256)), (515, 117, 3, O, 8, (0, 1, 1, 256)),
    (516, 120, 3, C, 0, (0, 1, 1, 256)), (517, 118, 3, R, 0, (0, 1, 1, 256)), (518, 119, 3, O, 0, (0, 1, 1, 256)),
    (519, 116, 3, C, 4, (0, 1, 1, 256)), (688, 345, 256, R, 1, (0, 1, 0, 256)),
    # ---- chunk decoder, tiles, 256 threads, rm 1 .. 8 in order: split, fused, self, table
    (4097, 114, 72, O, 1, (0, 2, 0, 256)), (4098, 123, 3, C, 2, (0, 2, 2, 256)), (211, 301, 3, R, 4, (0, 2, 1, 256)),
    (212, 303, 3, O, 8, (0, 2, 1, 256)), (213, 302, 3, C, 0, (0, 2, 1, 256)), (214, 300, 3, R, 0, (0, 2, 1, 256)),
    (215, 304, 3, O, 0, (0, 2, 1, 256)), (8200, 25, 256, C, 0, (0, 2, 0, 256)),
]

FORM_KEYS = ("kernel", "image_mode", "index_mode", "threads")
INDEX_MODES = ("self", "fused", "split", "table")


def form_of(plan):
    return tuple(plan[k] for k in FORM_KEYS)


def split_for(n, cpf):
    """index_split_for (dbde_capi.cpp): workgroups per frame of the decode index kernel."""
    if n < 1 or n >= 256 or cpf < 8:
        return 1
    return max(1, min(1024 // n, (cpf + 3) // 4))


def path_of(W, residue, image_mode):
    if image_mode == DIRECT:
        return "direct128" if W % 128 == 0 else "direct16"
    if image_mode == TILES:
        return "tiles"
    if W % 16 == 0 and residue % 16 == 0:
        return "staged16"
    if W % 8 == 0 and residue % 8 == 0:
        return "staged8"
    return "shifted"


def cell_of(W, H, n, residue, plan):
    rm = W % 8 or 8
    if plan["kernel"] == MID:
        return "mid", plan["threads"], W % 4 == 0 and residue % 4 == 0, rm
    return "chunk", path_of(W, residue, plan["image_mode"]), plan["threads"], rm


def index_of(n, plan):
    """The index mode of a chunk-decoder launch; None for the mid decoder, which has no index."""
    if plan["kernel"] == MID:
        return None
    if plan["index_mode"] != TABLE:
        return "self" if plan["index_mode"] == SELF else "fused"
    return "split" if split_for(n, plan["chunks_per_frame"]) > 1 else "table"


def case_id(case):
    W, H, n, how, residue, form = case
    return f"{W}x{H}x{n}-{how}-r{residue}-k{form[0]}i{form[1]}x{form[2]}t{form[3]}"


def row_cell(case):
    W, H, n, _, residue, _ = case
    return cell_of(W, H, n, residue, dv.decode_plan(W, H, n, residue, n_cu=256))


def row_index(case):
    W, H, n, _, residue, _ = case
    return index_of(n, dv.decode_plan(W, H, n, residue, n_cu=256))


def test_rows_are_distinct():
    assert len({c[:5] for c in DECODE_CASES}) == len(DECODE_CASES)
    assert len({case_id(c) for c in DECODE_CASES}) == len(DECODE_CASES)
    assert {c[3] for c in DECODE_CASES} == {C, R, O}


@pytest.mark.parametrize("case", DECODE_CASES, ids=case_id)
def test_every_case_runs_its_stated_form(case):
    W, H, n, how, residue, form = case
    plan = dv.decode_plan(W, H, n, residue, n_cu=256)
    assert form_of(plan) == form, f"decode_plan {plan} is not {form}"
    # the GPU test places the images at a 256-byte aligned address plus the residue: the same form there
    assert form_of(dv.decode_plan(W, H, n, (1 << 20) + residue, n_cu=256)) == form
    assert cr.tiles(W, H) * n <= MAX_TILES
    # with a margin against a device that reports a few more or fewer CUs than 256 (the fused form: 4 * n_cu chunks)
    index = index_of(n, plan)
    if index == "fused":
        assert plan["n_chunks"] <= 900, plan
    if index in ("table", "split"):
        assert plan["n_chunks"] >= 1150, plan
    for n_cu in (228, 256, 284):
        assert form_of(dv.decode_plan(W, H, n, residue, n_cu=n_cu)) == form, n_cu


def test_split_for_is_the_planners():
    """dv.roi_plan reports index_split_for(n, chunks_per_frame) of its own chunk geometry: the restatement above gives
    the same for every frame size and batch, the thresholds (8 chunks, 256 frames, 1024 workgroups) included."""
    seen = set()
    sizes = ((8, 8), (64, 56), (64, 57), (64, 64), (200, 123), (688, 345), (1920, 258), (4097, 114), (4096, 3072))
    for W, H in sizes:
        for n in list(range(1, 40)) + [63, 64, 85, 86, 127, 128, 129, 255, 256, 257, 511, 512, 1023, 1024, 1025, 2048]:
            p = dv.roi_plan(W, H, n, 0, 0, W, H)
            assert p["index_split"] == split_for(n, p["chunks_per_frame"]), (W, H, n, p)
            seen.add(p["index_split"])
    assert {1, 2, 4, 8, 96} <= seen and len(seen) >= 8, sorted(seen)


SCAN_W = (list(range(1, 301)) + list(range(505, 531)) + list(range(683, 701)) + list(range(1000, 1032))
          + list(range(1360, 1373)) + list(range(1913, 1940)) + list(range(2190, 2211)) + list(range(2990, 3011))
          + list(range(4089, 4105)) + [8200])
SCAN_H = (1, 5, 8, 9, 10, 11, 12, 13, 14, 15, 17, 64, 70, 100, 123, 300, 1081)
SCAN_N = (1, 3, 40, 300, 2048)
SCAN_RESIDUES = (0, 1, 2, 4, 8, 16)


@pytest.fixture(scope="module")
def found():
    """Every (cell, index mode) the planner offers in the scan, with the first place it was seen."""
    out = {}
    for W in SCAN_W:
        for H in SCAN_H:
            for n in SCAN_N:
                for residue in SCAN_RESIDUES:
                    plan = dv.decode_plan(W, H, n, residue, n_cu=256)
                    out.setdefault((cell_of(W, H, n, residue, plan), index_of(n, plan)), (W, H, n, residue))
    return out


def test_the_table_lacks_no_cell_the_planner_offers(found):
    assert {H % 8 or 8 for H in SCAN_H} == set(range(1, 9))
    have = {row_cell(c) for c in DECODE_CASES}
    cells = {}
    for (cell, _), at in found.items():
        cells.setdefault(cell, at)
    missing = {c: at for c, at in cells.items() if c not in have}
    assert not missing, f"cells without a row in DECODE_CASES (cell: first place seen): {missing}"
    # what the scan is known to offer, so that a scan that went blind fails too
    every = set(range(1, 9))
    for threads in (192, 256):
        assert {c[3] for c in cells if c[:3] == ("chunk", "shifted", threads)} == every, threads
    assert {c[2:] for c in cells if c[:2] == ("chunk", "tiles")} == {(256, rm) for rm in every}
    for threads in (256, 512, 1024):
        assert {c[3] for c in cells if c[:3] == ("mid", threads, False)} == every, threads
        assert {c[3] for c in cells if c[:3] == ("mid", threads, True)} == {4, 8}, threads
    aligned = {c[1:] for c in cells if c[0] == "chunk" and c[1] not in ("shifted", "tiles")}
    assert aligned == {("direct128", 256, 8), ("direct16", 256, 8), ("staged16", 256, 8), ("staged8", 192, 8),
                       ("staged8", 256, 8)}
    assert len(cells) == 59
    # a table row outside the scan's cells would be a row that tests nothing the planner offers
    assert have <= set(cells), have - set(cells)


def chunk_paths():
    return sorted({row_cell(c)[1:3] for c in DECODE_CASES if c[5][0] == CHUNK})


def test_index_modes(found):
    """Every (path, workgroup size) of the chunk decoder with each index mode: the scan offers all four for every one."""
    offered = {(cell[1:3], index) for cell, index in found if cell[0] == "chunk"}
    paths = chunk_paths()
    assert len(paths) == 8
    assert offered == {(p, i) for p in paths for i in INDEX_MODES}
    have = {(row_cell(c)[1:3], row_index(c)) for c in DECODE_CASES if c[5][0] == CHUNK}
    assert have == offered, offered - have


def mid_groups(case):
    """decode_mid_kernel: `fpw = THREADS / T` frames per workgroup, `n_groups = (n_frames + fpw - 1) / fpw`."""
    W, H, n, _, _, form = case
    fpw = form[3] // cr.tiles(W, H)
    return fpw, -(-n // fpw)


def test_mid_rows_walk_the_pipelined_loop():
    """A mid row has seven groups of frames and more, so that each of the three workgroups of the "three" context (and
    a workgroup of a device with fewer slots than groups) runs the software-pipelined loop at least twice, with both
    sets of the alternating LDS arrays.  Every (workgroup size, staged) also has a row whose groups do not all start
    at a multiple of 16 bytes: the staged copy-out's partial first and last blocks."""
    unaligned = set()
    for c in DECODE_CASES:
        if c[5][0] != MID:
            continue
        fpw, groups = mid_groups(c)
        assert fpw >= 1 and groups >= 7, f"{case_id(c)}: {groups} groups of {fpw} frames"
        if any((c[4] + g * fpw * c[0] * c[1]) % 16 for g in range(groups)):
            unaligned.add(row_cell(c)[1:3])
    assert unaligned == {(t, s) for t in (256, 512, 1024) for s in (False, True)}, unaligned
    assert {mid_groups(c)[0] for c in DECODE_CASES if c[5] == (MID, 0, 0, 256)} == {1, 2}


def test_bottom_margins():
    groups = {}
    for c in DECODE_CASES:
        cell = row_cell(c)
        groups.setdefault(cell[:3] if cell[0] == "mid" else cell[1:3], set()).add(c[1] % 8 or 8)
    assert len(groups) == 6 + 8
    for key, dms in groups.items():
        assert dms == set(range(1, 9)), f"{key}: bottom margins {sorted(dms)}"


def test_base_residues(found):
    """The paths whose image rows are not aligned, at every base residue at which the planner offers them."""
    def unaligned(cell):
        if cell[0] == "mid":
            return cell[:3] if not cell[2] else None
        return cell[1:3] if cell[1] in ("shifted", "tiles") else None

    offered = {}
    for W in SCAN_W:
        for H in (9, 70, 300):
            for n in (3, 40):
                for residue in (0, 1, 2, 4, 8):
                    key = unaligned(cell_of(W, H, n, residue, dv.decode_plan(W, H, n, residue, n_cu=256)))
                    if key:
                        offered.setdefault(key, set()).add(residue)
    assert set(offered) == {("mid", 256, False), ("mid", 512, False), ("mid", 1024, False), ("shifted", 192),
                            ("shifted", 256), ("tiles", 256)}
    have = {}
    for c in DECODE_CASES:
        key = unaligned(row_cell(c))
        if key:
            have.setdefault(key, set()).add(c[4])
    for key, residues in offered.items():
        assert residues == {0, 1, 2, 4, 8}, (key, residues)
        assert have[key] >= residues, f"{key}: base residues {sorted(have[key])}"


def test_the_checker_sees_one_pixel_and_one_guard_byte(oracle):
    """The checks of the GPU test (check_decode, and images_of, the guard check of decode_into) on the oracle's own
    images pass; with one pixel altered in the last column of a cut tile, or one guard byte, they raise."""
    from test_gpu_crafted_decode import FILL, PAD, Stream, check_decode, images_of
    W, H, n, base = 21, 13, 24, 1
    s = Stream(oracle, np.random.default_rng(2113), W, H, n, "residues", device="cpu")
    rejected = [f for f in range(n) if s.images[f] is None]
    assert rejected and len(rejected) < n - 2

    def canvas():
        c = np.full(PAD + base + n * H * W + PAD, FILL, np.uint8)
        for f in range(n):
            if s.images[f] is not None:
                c[PAD + base + f * H * W: PAD + base + (f + 1) * H * W] = s.images[f].reshape(-1)
        return c

    rows = list(s.rows)
    check_decode(images_of(canvas(), s, base), rows, s, "oracle")
    f = max(k for k in range(n) if s.images[k] is not None)
    for y, x in ((0, W - 1), (H - 1, W - 1), (H - 1, 0), (8, W - 1)):      # last column and last row of the cut tiles
        c = canvas()
        c[PAD + base + (f * H + y) * W + x] ^= 1
        with pytest.raises(AssertionError, match=f"frame {f}: 1 pixels differ"):
            check_decode(images_of(c, s, base), rows, s, "one pixel")
    c = canvas()
    c[PAD + base + (rejected[0] * H + H - 1) * W + W - 1] = 0
    with pytest.raises(AssertionError, match="rejected frame"):
        check_decode(images_of(c, s, base), rows, s, "rejected")
    for at in (0, PAD + base - 1, PAD + base + n * H * W, len(canvas()) - 1):
        c = canvas()
        c[at] ^= 0x80
        with pytest.raises(AssertionError, match="wrote (in front of|behind) the images"):
            images_of(c, s, base)
    wrong = list(rows)
    wrong[f] = rows[f][:3] + (rows[f][3] + 8,)
    with pytest.raises(AssertionError, match=f"frame {f} result"):
        check_decode(images_of(canvas(), s, base), wrong, s, "results row")


def test_the_pool_selection_of_stream(oracle):
    """Stream(select=...) holds exactly the chosen pool entries, in order and cycled; `used` names them."""
    from test_gpu_crafted_decode import POOL, Stream
    W, H = 21, 13
    s = Stream(oracle, np.random.default_rng(5), W, H, 3, "concat", select=[9, 10, POOL - 1], device="cpu")
    assert s.used == {9, 10, POOL - 1}
    assert [img is None for img in s.images] == [False, True, True]
    s = Stream(oracle, np.random.default_rng(5), W, H, 5, "offsets", select=[4, 12], device="cpu")
    assert s.used == {4, 12} and [img is None for img in s.images] == [False, True, False, True, False]
    assert (s.depths[0] == 8).all() and len(s.depths[0]) == cr.tiles(W, H)
    s = Stream(oracle, np.random.default_rng(5), W, H, 40, "residues", device="cpu")
    assert s.used <= set(range(POOL)) and len(s.used) > 10
