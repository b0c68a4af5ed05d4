"""CPU: the coverage table of the crafted-image encoder tests, and the proof that it misses no encoder form.

ENCODE_CASES is the contract between this file and tests/test_gpu_crafted_encode.py, which runs every row on the
device: (W, H, n, slot layout, image address residue, form), form = the (kernel, input_mode, threads, aligned_out) that
dv.encode_plan (host arithmetic only, the function dbde_hip_encode_frames itself calls) reports for the row.

A cell is a code path whose edge-tile padding has arithmetic of its own on the right margin rm = W mod 8 (8 for whole
tiles).  Which plan fields select a code path was read off the dispatch (dbde_hip_encode_frames in dbde_capi.cpp and
the launchers in dbde_kernels.hip):

  * kernels 0 and 1 (persistent, small) are instantiated per input mode (in_mode_of): cell (kernel, input_mode, rm);
  * kernels 2, 3 and 4 (tiny, mid, whole-frame) never read the input mode -- tiny and mid load every tile with
    load_tile_generic, the whole-frame encoder stages whole rows -- but mid and whole-frame are instantiated per
    workgroup size: cell (kernel, threads, rm);
  * kernel 5 (group) does not read it either; its two instances are chosen by launch_encode_group from the
    alignment (whole 16-byte blocks, or rows and bases of 4-byte multiples): cell (5, instance, rm).

Every kernel repeats the last image row below the frame, so every kernel also appears with each bottom margin
dm = H mod 8 in 1..7 (most rows pair the margins: rm = dm).
"""
import pytest

import dbde_video_cpp_amd as dv

PERSISTENT, SMALL, TINY, MID, FRAMES, GROUP = 0, 1, 2, 3, 4, 5
P, S = "packed", "slots"      # frames back to back (slot_stride 0) | one 256-byte aligned worst-case slot per frame


@pytest.fixture(scope="module", autouse=True)
def built():
    dv.build()


def slot_stride(layout, W, H):
    return 0 if layout == P else (dv.max_frame_bytes(W, H) + 255) // 256 * 256


# The persistent encoder takes a launch of at least as many chunks as the device holds workgroups (513): 560 frames of
# one chunk each, 17 of 1921 x 1081.  The small encoder takes what is below that.  A batch smaller than the number of
# image families is encoded several times over (12-megapixel frames: one frame of every family, two or three a call).
ENCODE_CASES = [
    # ---- persistent (kernel 0): input mode 0, 1 (rm 2, 4, 6, 7, 8), 2, 3, 4 (every rm); rm = dm
    (16, 16, 560, P, 0, (0, 0, 512, 1)), (16, 24, 560, P, 0, (0, 0, 512, 0)),
    (18, 10, 560, P, 0, (0, 1, 512, 0)), (20, 12, 560, P, 0, (0, 1, 512, 0)), (22, 14, 560, P, 0, (0, 1, 512, 0)),
    (31, 15, 560, P, 0, (0, 1, 512, 1)), (16, 16, 560, P, 1, (0, 1, 512, 1)),
    (1, 9, 560, P, 0, (0, 2, 512, 0)), (2, 10, 560, P, 0, (0, 2, 512, 0)), (3, 11, 560, P, 0, (0, 2, 512, 0)),
    (4, 12, 560, P, 0, (0, 2, 512, 0)), (5, 13, 560, P, 0, (0, 2, 512, 0)), (6, 14, 560, P, 0, (0, 2, 512, 0)),
    (7, 15, 560, P, 0, (0, 2, 512, 0)), (8, 16, 560, P, 0, (0, 2, 512, 0)), (8, 32, 560, P, 0, (0, 2, 512, 1)),
    (17, 9, 560, P, 0, (0, 3, 512, 0)), (18, 10, 560, P, 1, (0, 3, 512, 0)), (19, 11, 560, P, 0, (0, 3, 512, 0)),
    (20, 12, 560, P, 1, (0, 3, 512, 0)), (21, 13, 560, P, 0, (0, 3, 512, 0)), (22, 14, 560, P, 1, (0, 3, 512, 0)),
    (23, 15, 560, P, 0, (0, 3, 512, 0)), (24, 16, 560, P, 1, (0, 3, 512, 0)), (17, 25, 560, P, 0, (0, 3, 512, 1)),
    (1001, 9, 560, P, 0, (0, 4, 512, 1)), (1002, 10, 560, P, 1, (0, 4, 512, 1)), (1003, 11, 560, P, 0, (0, 4, 512, 1)),
    (1004, 12, 560, P, 1, (0, 4, 512, 1)), (1005, 13, 560, P, 0, (0, 4, 512, 1)), (1926, 14, 560, P, 1, (0, 4, 512, 0)),
    (1927, 15, 560, P, 0, (0, 4, 512, 0)), (1000, 16, 560, P, 1, (0, 4, 512, 0)),
    # ... at the sizes the encoder was built for: many chunks per frame, slots and concatenated frames
    (1921, 1081, 17, S, 0, (0, 4, 512, 1)), (1081, 1921, 17, P, 0, (0, 3, 512, 1)), (1366, 768, 33, P, 0, (0, 1, 512, 1)),
    (4096, 512, 18, S, 0, (0, 0, 512, 1)), (200, 123, 560, S, 0, (0, 1, 512, 1)), (4096, 3072, 3, S, 0, (0, 0, 512, 1)),
    # ---- small (kernel 1): the same cells
    (16, 16, 12, P, 0, (1, 0, 512, 1)), (16, 24, 12, P, 0, (1, 0, 512, 0)),
    (18, 10, 12, P, 0, (1, 1, 512, 0)), (20, 12, 12, P, 0, (1, 1, 512, 0)), (22, 14, 12, P, 0, (1, 1, 512, 0)),
    (31, 15, 12, P, 0, (1, 1, 512, 1)), (16, 16, 12, P, 1, (1, 1, 512, 1)),
    (1, 9, 12, P, 0, (1, 2, 512, 0)), (2, 10, 12, P, 0, (1, 2, 512, 0)), (3, 11, 12, P, 0, (1, 2, 512, 0)),
    (4, 12, 12, P, 0, (1, 2, 512, 0)), (5, 13, 12, P, 0, (1, 2, 512, 0)), (6, 14, 12, P, 0, (1, 2, 512, 0)),
    (7, 15, 12, P, 0, (1, 2, 512, 0)), (8, 16, 12, P, 0, (1, 2, 512, 0)), (8, 32, 12, P, 0, (1, 2, 512, 1)),
    (17, 9, 12, P, 0, (1, 3, 512, 0)), (18, 10, 12, P, 1, (1, 3, 512, 0)), (19, 11, 12, P, 0, (1, 3, 512, 0)),
    (20, 12, 12, P, 1, (1, 3, 512, 0)), (21, 13, 12, P, 0, (1, 3, 512, 0)), (22, 14, 12, P, 1, (1, 3, 512, 0)),
    (23, 15, 12, P, 0, (1, 3, 512, 0)), (24, 16, 12, P, 1, (1, 3, 512, 0)), (17, 25, 12, P, 0, (1, 3, 512, 1)),
    (1001, 9, 12, P, 0, (1, 4, 512, 1)), (1002, 10, 12, P, 1, (1, 4, 512, 1)), (1003, 11, 12, P, 0, (1, 4, 512, 1)),
    (1004, 12, 12, P, 1, (1, 4, 512, 1)), (1005, 13, 12, P, 0, (1, 4, 512, 1)), (1926, 14, 12, P, 1, (1, 4, 512, 0)),
    (1927, 15, 12, P, 0, (1, 4, 512, 0)), (1000, 16, 12, P, 1, (1, 4, 512, 0)),
    (1921, 1081, 6, P, 0, (1, 4, 512, 1)), (1001, 1001, 6, S, 0, (1, 4, 512, 1)), (1928, 1080, 6, P, 1, (1, 4, 512, 0)),
    (4096, 512, 12, S, 0, (1, 0, 512, 1)), (200, 123, 12, P, 0, (1, 1, 512, 1)), (4096, 3072, 2, P, 0, (1, 0, 512, 1)),
    # ---- tiny (kernel 2): every rm = dm
    (1, 9, 40, S, 0, (2, 2, 256, 0)), (2, 10, 40, S, 0, (2, 2, 256, 0)), (3, 11, 40, S, 0, (2, 2, 256, 0)),
    (4, 12, 40, S, 2, (2, 2, 256, 0)), (5, 13, 40, S, 0, (2, 2, 256, 0)), (6, 14, 40, S, 0, (2, 2, 256, 0)),
    (7, 15, 40, S, 0, (2, 2, 256, 0)), (8, 8, 40, S, 0, (2, 2, 256, 0)), (18, 18, 40, S, 0, (2, 1, 256, 0)),
    (61, 59, 40, S, 0, (2, 3, 256, 1)),
    # ---- mid (kernel 3): workgroups of 256, 512 and 1024 threads, every rm = dm
    (209, 17, 40, S, 0, (3, 3, 256, 0)), (210, 18, 40, S, 0, (3, 1, 256, 0)), (211, 19, 40, S, 0, (3, 3, 256, 0)),
    (212, 20, 40, S, 1, (3, 3, 256, 0)), (213, 21, 40, S, 0, (3, 3, 256, 0)), (214, 22, 40, S, 0, (3, 1, 256, 0)),
    (215, 23, 40, S, 0, (3, 3, 256, 0)), (40, 128, 40, S, 1, (3, 3, 256, 1)),
    (273, 9, 40, S, 0, (3, 3, 512, 0)), (274, 10, 40, S, 0, (3, 1, 512, 0)), (275, 11, 40, S, 0, (3, 3, 512, 0)),
    (276, 12, 40, S, 1, (3, 3, 512, 0)), (277, 13, 40, S, 0, (3, 3, 512, 0)), (278, 14, 40, S, 0, (3, 1, 512, 0)),
    (279, 15, 40, S, 0, (3, 3, 512, 0)), (184, 24, 40, S, 1, (3, 3, 512, 0)), (102, 100, 40, S, 0, (3, 1, 512, 0)),
    (1, 1073, 40, S, 0, (3, 2, 1024, 0)), (2, 1074, 40, S, 0, (3, 2, 1024, 0)), (259, 11, 40, S, 0, (3, 3, 1024, 0)),
    (260, 12, 40, S, 1, (3, 3, 1024, 0)), (261, 13, 40, S, 0, (3, 3, 1024, 0)), (262, 14, 40, S, 0, (3, 1, 1024, 0)),
    (263, 15, 40, S, 0, (3, 3, 1024, 0)), (40, 104, 40, S, 1, (3, 3, 1024, 0)), (75, 70, 40, S, 0, (3, 3, 1024, 0)),
    # ---- whole-frame (kernel 4): rm = 8 only, both workgroup sizes, every dm
    (96, 96, 40, S, 0, (4, 0, 256, 1)), (40, 104, 40, S, 0, (4, 1, 256, 0)), (520, 64, 40, S, 0, (4, 1, 512, 1)),
    (200, 168, 40, S, 0, (4, 1, 512, 0)),
    (128, 98, 40, S, 0, (4, 0, 256, 1)), (128, 100, 40, S, 0, (4, 0, 256, 1)), (128, 102, 40, S, 0, (4, 0, 256, 1)),
    (128, 97, 40, S, 0, (4, 0, 256, 1)), (128, 99, 40, S, 0, (4, 0, 256, 1)), (128, 101, 40, S, 0, (4, 0, 256, 1)),
    (128, 103, 40, S, 0, (4, 0, 256, 1)),
    (528, 66, 20, S, 0, (4, 0, 512, 0)), (528, 69, 20, S, 0, (4, 0, 512, 0)),
    # ---- group (kernel 5): whole 16-byte blocks (rm 8), rows of 4-byte multiples (rm 4 and 8), every dm
    (64, 64, 40, S, 0, (5, 0, 256, 1)), (16, 16, 40, S, 4, (5, 1, 256, 1)), (12, 12, 40, S, 0, (5, 2, 256, 1)),
    (100, 100, 40, S, 0, (5, 1, 256, 0)), (72, 72, 40, S, 0, (5, 1, 256, 0)),
    (16, 9, 40, S, 0, (5, 0, 256, 1)), (16, 10, 40, S, 0, (5, 0, 256, 1)), (16, 11, 40, S, 0, (5, 0, 256, 1)),
    (32, 13, 40, S, 0, (5, 0, 256, 1)), (20, 13, 40, S, 4, (5, 1, 256, 0)), (20, 14, 40, S, 8, (5, 1, 256, 0)),
    (20, 15, 40, S, 0, (5, 1, 256, 0)), (24, 9, 40, S, 8, (5, 1, 256, 0)), (24, 14, 40, S, 4, (5, 1, 256, 0)),
]

FORM_KEYS = ("kernel", "input_mode", "threads", "aligned_out")


def plan_of(W, H, n, layout, residue, image_base=0, out_base=0):
    return dv.encode_plan(W, H, n, image_base + residue, out_base, slot_stride(layout, W, H))


def form_of(plan):
    return tuple(plan[k] for k in FORM_KEYS)


def group_instance(W, H, residue):
    """launch_encode_group: the instance without the shifted image where rows are 8-byte multiples and frames and
    base are whole 16-byte blocks."""
    return "blocks16" if W % 8 == 0 and (W * H) % 16 == 0 and residue % 16 == 0 else "rows4"


def cell_of(W, H, residue, form):
    kernel, input_mode, threads, _ = form
    rm = W % 8 or 8
    if kernel in (PERSISTENT, SMALL):
        return kernel, input_mode, rm
    if kernel == GROUP:
        return kernel, group_instance(W, H, residue), rm
    return kernel, threads, rm


def case_id(case):
    W, H, n, layout, residue, form = case
    return f"{W}x{H}x{n}-{layout}-r{residue}-k{form[0]}m{form[1]}t{form[2]}a{form[3]}"


def test_rows_are_distinct():
    assert len({c[:5] for c in ENCODE_CASES}) == len(ENCODE_CASES)
    assert len({case_id(c) for c in ENCODE_CASES}) == len(ENCODE_CASES)


@pytest.mark.parametrize("case", ENCODE_CASES, ids=case_id)
def test_every_case_runs_its_stated_form(case):
    W, H, n, layout, residue, form = case
    plan = plan_of(W, H, n, layout, residue)
    assert form_of(plan) == form, f"encode_plan {plan} is not {form}"
    # the GPU test places the image at a 256-byte aligned base plus the residue: the same form there
    assert form_of(plan_of(W, H, n, layout, residue, image_base=1 << 20, out_base=1 << 21)) == form
    if form[0] == PERSISTENT:   # with a margin against a device that holds a few more or fewer workgroups than 513
        assert plan["n_chunks"] >= 540, plan
    if form[0] == SMALL:
        assert plan["n_chunks"] <= 450, plan


SCAN_W = list(range(1, 301)) + list(range(505, 531)) + list(range(1000, 1032)) + list(range(1913, 1940)) + list(range(4089, 4100))
SCAN_H = (1, 5, 8, 9, 17, 64, 70, 100, 123, 1081)
SCAN_N = (1, 3, 64, 2048)
SCAN_RESIDUES = (0, 1, 2, 4, 8)


def test_the_table_lacks_no_cell_the_planner_offers():
    have = {cell_of(c[0], c[1], c[4], c[5]) for c in ENCODE_CASES}
    found = {}
    for W in SCAN_W:
        for H in SCAN_H:
            for layout in (P, S):
                stride = slot_stride(layout, W, H)
                for n in SCAN_N:
                    for residue in SCAN_RESIDUES:
                        plan = dv.encode_plan(W, H, n, residue, 0, stride)
                        found.setdefault(cell_of(W, H, residue, form_of(plan)), (W, H, n, layout, residue))
    missing = {c: at for c, at in found.items() if c not in have}
    assert not missing, f"cells without a row in ENCODE_CASES (cell: first place seen): {missing}"
    # what the scan is known to offer, so that a scan that went blind fails too
    for kernel in (PERSISTENT, SMALL):
        assert {c[2] for c in found if c[:2] == (kernel, 0)} == {8}
        assert {c[2] for c in found if c[:2] == (kernel, 1)} == {2, 4, 6, 7, 8}
        for mode in (2, 3, 4):
            assert {c[2] for c in found if c[:2] == (kernel, mode)} == set(range(1, 9)), (kernel, mode)
    assert {c[2] for c in found if c[0] == TINY} == set(range(1, 9))
    for threads in (256, 512, 1024):
        assert {c[2] for c in found if c[:2] == (MID, threads)} == set(range(1, 9))
    assert {c[1:] for c in found if c[0] == FRAMES} == {(256, 8), (512, 8)}
    assert {c[1:] for c in found if c[0] == GROUP} == {("blocks16", 8), ("rows4", 4), ("rows4", 8)}
    # a table row outside the scan's cells would be a row that tests nothing the planner offers
    assert have <= set(found), have - set(found)


def test_bottom_margins_workgroup_sizes_and_output_alignment():
    for kernel in (PERSISTENT, SMALL, TINY, MID, FRAMES, GROUP):
        dms = {c[1] % 8 or 8 for c in ENCODE_CASES if c[5][0] == kernel}
        assert dms == set(range(1, 9)), f"kernel {kernel}: bottom margins {sorted(dms)}"
    assert {c[5][2] for c in ENCODE_CASES if c[5][0] == FRAMES} == {256, 512}
    assert {c[5][2] for c in ENCODE_CASES if c[5][0] == MID} == {256, 512, 1024}
    # the chunk kernels are also instantiated on the output's alignment
    for kernel in (PERSISTENT, SMALL):
        for mode in range(5):
            assert {c[5][3] for c in ENCODE_CASES if c[5][:2] == (kernel, mode)} == {0, 1}, (kernel, mode)
    for kernel in (PERSISTENT, SMALL):
        assert {c[3] for c in ENCODE_CASES if c[5][0] == kernel} == {P, S}
