"""CPU, compile only: the gfx950 listing of the pair projection kernels (`make asm`, dbde_pairs_kernels.s; no GPU).

dbde_hip_project_pairs (PIX = 1) and dbde16_hip_project_pairs (PIX = 2) launch pairs_kernel<MASK, PIX> with MASK the
instance that serves the requested offsets -- 1 (RIGHT alone), 3 (RIGHT, DOWN) or 15 (all four) -- followed with several
segments by pairs_combine_kernel<partial type, ACC>.  Every instance keeps its sums in registers on top of
project_kernel's pipeline (twice over where it also decodes the row below) and the decoded band in LDS: no scratch, no
dynamic stack, the LDS the plan reports, and the VGPR count of DESIGN.md 4.20's table, within the 256 architectural
VGPRs of a 256-lane workgroup.  Only `.amdhsa_*` fields are read.
"""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dbde-video-cpp_amd", "csrc")
sys.path.insert(0, ROOT)

INSTANCES = (1, 3, 15)
# next_free_vgpr of pairs_kernel<MASK, PIX>
VGPRS = {(1, 1): 80, (3, 1): 138, (15, 1): 154, (1, 2): 90, (3, 2): 145, (15, 2): 163}
COMBINE_LDS = 16      # write_count's wave counts


@pytest.fixture(scope="module")
def kernels():
    r = subprocess.run(["make", "-s", "-C", CSRC, "asm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    meta = open(os.path.join(CSRC, "dbde_pairs_kernels.s")).read()
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", meta, re.S):
        fields = dict(re.findall(r"\.amdhsa_(\w+) (\d+)", m.group(2)))
        out[m.group(1)] = {k: int(v) for k, v in fields.items()}
    return out


def name(mask, pix):
    return f"_ZN4dbde12pairs_kernelILj{mask}ELj{pix}EEEvNS_11PairsParamsE"


COMBINE = {f"_ZN4dbde20pairs_combine_kernelI{t}Lb{a}EEEvNS_11PairsParamsE" for t in "jm" for a in (0, 1)}


def test_six_instances_and_four_combine_kernels(kernels):
    assert set(kernels) == {name(m, pix) for m in INSTANCES for pix in (1, 2)} | COMBINE


def test_no_scratch_and_no_dynamic_stack(kernels):
    for k, f in kernels.items():
        assert f["private_segment_fixed_size"] == 0, (k, "scratch")
        assert not f.get("uses_dynamic_stack", 0), k
        assert not f.get("enable_private_segment", 0), k


@pytest.mark.parametrize("pix", (1, 2))
def test_lds_matches_plan_for_every_mask(kernels, pix):
    import dbde_video_cpp_amd as dv
    if not os.path.exists(dv.LIB_PATH):
        dv.build()
    plan = dv.pairs_plan if pix == 1 else dv.pairs16_plan
    for mask in range(1, 16):
        p = plan(64, 64, 10, pairs=mask)
        assert p["instance"] in INSTANCES and p["instance"] & mask == mask      # a superset of the request
        assert kernels[name(p["instance"], pix)]["group_segment_fixed_size"] == p["lds_bytes"], mask
    assert plan(64, 64, 10, pairs=1)["lds_bytes"] == 2 * 4 * 8 * 288 + 2 * 4 * 1 * 32 + 16
    assert plan(64, 64, 10, pairs=15)["lds_bytes"] == 2 * 4 * 9 * 288 + 2 * 4 * 2 * 32 + 16
    for k in COMBINE:
        assert kernels[k]["group_segment_fixed_size"] == COMBINE_LDS


@pytest.mark.parametrize("pix", (1, 2))
def test_vgprs_are_pinned_and_spill_free(kernels, pix):
    for mask in INSTANCES:
        f = kernels[name(mask, pix)]
        assert f["next_free_vgpr"] == VGPRS[(mask, pix)], (mask, pix, f["next_free_vgpr"])
        assert f["next_free_vgpr"] <= 256
