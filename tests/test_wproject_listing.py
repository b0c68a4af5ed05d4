"""CPU, compile only: the gfx950 listing of the weighted projection kernels (`make asm`, dbde_wproject_kernels.s; no
GPU).

dbde_hip_project_weighted (PIX = 1) and dbde16_hip_project_weighted (PIX = 2) launch one wproject_kernel<R, PIX>
instance per regressor count R = 1..8, followed with several segments by wproject_combine_kernel<ACC> (ACC: the planes'
prior content is the first operand).  Every instance keeps its R x 8 (PIX 2: R x 4) F32 accumulators in registers on
top of project_kernel's pipeline: no scratch, no dynamic stack, the LDS the plan reports, and the VGPR count of
DESIGN.md 4.17's table, within the 256 architectural VGPRs of a 256-lane workgroup.  Only `.amdhsa_*` fields are read.
"""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dbde-video-cpp_amd", "csrc")
sys.path.insert(0, ROOT)

# next_free_vgpr of wproject_kernel<R, PIX>, R = 1..8
VGPRS = {1: (90, 100, 108, 116, 124, 132, 140, 148), 2: (94, 100, 104, 108, 112, 116, 120, 124)}
COMBINE_LDS = 16      # write_count's wave counts


@pytest.fixture(scope="module")
def kernels():
    r = subprocess.run(["make", "-s", "-C", CSRC, "asm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    meta = open(os.path.join(CSRC, "dbde_wproject_kernels.s")).read()
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", meta, re.S):
        fields = dict(re.findall(r"\.amdhsa_(\w+) (\d+)", m.group(2)))
        out[m.group(1)] = {k: int(v) for k, v in fields.items()}
    return out


def name(R, pix):
    return f"_ZN4dbde15wproject_kernelILj{R}ELj{pix}EEEvNS_11WProjParamsE"


COMBINE = {f"_ZN4dbde23wproject_combine_kernelILb{a}EEEvNS_11WProjParamsE" for a in (0, 1)}


def test_sixteen_instances_and_two_combine_kernels(kernels):
    assert set(kernels) == {name(R, pix) for R in range(1, 9) for pix in (1, 2)} | COMBINE


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
    plan = dv.wproject_plan if pix == 1 else dv.wproject16_plan
    for R in range(1, 9):
        assert kernels[name(R, pix)]["group_segment_fixed_size"] == plan(64, 64, 10, regressors=R)["lds_bytes"]
    for k in COMBINE:
        assert kernels[k]["group_segment_fixed_size"] == COMBINE_LDS


@pytest.mark.parametrize("pix", (1, 2))
def test_vgprs_are_pinned_and_spill_free(kernels, pix):
    for R in range(1, 9):
        f = kernels[name(R, pix)]
        assert f["next_free_vgpr"] == VGPRS[pix][R - 1], (R, pix, f["next_free_vgpr"])
        assert f["next_free_vgpr"] <= 256
        assert f["float_denorm_mode_32"] == 3, "F32 denormals are kept (the defined value's gradual underflow)"


@pytest.mark.parametrize("pix", (1, 2))
def test_each_regressor_costs_its_accumulators_at_most(kernels, pix):
    """R + 1 regressors need at most 8 / pix more VGPRs than R (beyond R = 1: the first few also free pipeline
    temporaries), and never fewer."""
    v = [kernels[name(R, pix)]["next_free_vgpr"] for R in range(1, 9)]
    for a, b in zip(v[1:], v[2:]):
        assert 0 < b - a <= 8 // pix
