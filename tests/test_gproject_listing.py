"""CPU, compile only: the gfx950 listing of the grouped projection kernels (`make asm`, dbde_gproject_kernels.s; no GPU).

dbde_hip_project_groups (PIX = 1) and dbde16_hip_project_groups (PIX = 2) launch one gproject_kernel<STATS, PIX>
instance per statistics set (every non-empty subset of max, min, sum and sumsq: 15); there is no finishing kernel (the
counts are written by each run's first workgroup).  The resource budget is project_kernel's: no
scratch, no dynamic stack, LDS within 512 bytes and at most 128 VGPRs, so that 4 workgroups of 256 threads per CU stay
resident.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dbde-video-cpp_amd", "csrc")

LDS_BUDGET = 512      # bytes per workgroup
VGPR_BUDGET = 128     # per lane: 4 waves per SIMD
PIXES = (1, 2)        # DBDE, DBDE16


@pytest.fixture(scope="module")
def kernels():
    r = subprocess.run(["make", "-s", "-C", CSRC, "asm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    meta = open(os.path.join(CSRC, "dbde_gproject_kernels.s")).read()
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", meta, re.S):
        fields = dict(re.findall(r"\.amdhsa_(\w+) (\d+)", m.group(2)))
        out[m.group(1)] = {k: int(v) for k, v in fields.items()}
    return out


def expected(pix):
    return {f"_ZN4dbde15gproject_kernelILj{s}ELj{pix}EEEvNS_11GProjParamsE" for s in range(1, 16)}


def instances(kernels, pix):
    got = {}
    for name, f in kernels.items():
        m = re.match(r"_ZN4dbde15gproject_kernelILj(\d+)ELj(\d+)EEEvNS_11GProjParamsE$", name)
        if m and int(m.group(2)) == pix:
            got[int(m.group(1))] = f
    return got


@pytest.mark.parametrize("pix", PIXES)
def test_one_instance_per_statistics_set(kernels, pix):
    assert sorted(instances(kernels, pix)) == list(range(1, 16))


def test_no_other_kernels(kernels):
    assert set(kernels) == expected(1) | expected(2)


@pytest.mark.parametrize("pix", PIXES)
def test_no_scratch_and_within_budget(kernels, pix):
    for name in sorted(expected(pix)):
        f = kernels[name]
        assert f["private_segment_fixed_size"] == 0, (name, "scratch")
        assert not f.get("uses_dynamic_stack", 0), name
        assert f["group_segment_fixed_size"] <= LDS_BUDGET, (name, f["group_segment_fixed_size"])
        assert f["next_free_vgpr"] <= VGPR_BUDGET, (name, f["next_free_vgpr"])


@pytest.mark.parametrize("pix", PIXES)
def test_fewer_statistics_cost_fewer_registers(kernels, pix):
    """An unrequested statistic has no accumulators: max + min alone needs fewer VGPRs than all four."""
    inst = instances(kernels, pix)
    assert inst[3]["next_free_vgpr"] < inst[15]["next_free_vgpr"]
