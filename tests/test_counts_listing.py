"""CPU, compile only: the gfx950 listing of the count projection kernels (`make asm`, dbde_counts_kernels.s; no GPU).

dbde_hip_project_counts (PIX = 1) and dbde16_hip_project_counts (PIX = 2) launch one counts_kernel<K, PIX> instance per
level count K = 1..8, followed with several segments by counts_combine_kernel<ACC> (ACC: the planes' prior content is
added).  Every instance keeps its K x 8 (PIX 2: K x 4) U32 counters and K x 2 registers of packed thresholds on top of
project_kernel's pipeline: no scratch, no dynamic stack, the LDS the plan reports, and the VGPR count of DESIGN.md
4.19's table, within the 256 architectural VGPRs of a 256-lane workgroup.  Only `.amdhsa_*` fields are read.
"""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dbde-video-cpp_amd", "csrc")
sys.path.insert(0, ROOT)

# next_free_vgpr of counts_kernel<K, PIX>, K = 1..8
VGPRS = {1: (89, 99, 109, 119, 129, 139, 149, 159), 2: (94, 100, 106, 112, 118, 124, 130, 136)}
COMBINE_LDS = 16      # write_count's wave counts


@pytest.fixture(scope="module")
def kernels():
    r = subprocess.run(["make", "-s", "-C", CSRC, "asm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    meta = open(os.path.join(CSRC, "dbde_counts_kernels.s")).read()
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", meta, re.S):
        fields = dict(re.findall(r"\.amdhsa_(\w+) (\d+)", m.group(2)))
        out[m.group(1)] = {k: int(v) for k, v in fields.items()}
    return out


def name(K, pix):
    return f"_ZN4dbde13counts_kernelILj{K}ELj{pix}EEEvNS_12CountsParamsE"


COMBINE = {f"_ZN4dbde21counts_combine_kernelILb{a}EEEvNS_12CountsParamsE" for a in (0, 1)}


def test_sixteen_instances_and_two_combine_kernels(kernels):
    assert set(kernels) == {name(K, pix) for K in range(1, 9) for pix in (1, 2)} | COMBINE


def test_no_scratch_and_no_dynamic_stack(kernels):
    for k, f in kernels.items():
        assert f["private_segment_fixed_size"] == 0, (k, "scratch")
        assert not f.get("uses_dynamic_stack", 0), k
        assert not f.get("enable_private_segment", 0), k


@pytest.mark.parametrize("pix", (1, 2))
def test_lds_matches_plan(kernels, pix):
    import dbde_video_cpp_amd as dv
    if not os.path.exists(dv.LIB_PATH):
        dv.build()
    plan = dv.counts_plan if pix == 1 else dv.counts16_plan
    for K in range(1, 9):
        assert kernels[name(K, pix)]["group_segment_fixed_size"] == plan(64, 64, 10, levels=K)["lds_bytes"]
    for k in COMBINE:
        assert kernels[k]["group_segment_fixed_size"] == COMBINE_LDS


@pytest.mark.parametrize("pix", (1, 2))
def test_vgprs_are_pinned_and_spill_free(kernels, pix):
    for K in range(1, 9):
        f = kernels[name(K, pix)]
        assert f["next_free_vgpr"] == VGPRS[pix][K - 1], (K, pix, f["next_free_vgpr"])
        assert f["next_free_vgpr"] <= 256


@pytest.mark.parametrize("pix", (1, 2))
def test_each_level_costs_its_counters_and_thresholds_at_most(kernels, pix):
    """K + 1 levels need at most 8 / pix counters and 2 threshold registers more than K, and never fewer."""
    v = [kernels[name(K, pix)]["next_free_vgpr"] for K in range(1, 9)]
    for a, b in zip(v, v[1:]):
        assert 0 < b - a <= 8 // pix + 2
