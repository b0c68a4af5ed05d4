"""CPU, compile only: the gfx950 listing of the DBDE16 projection kernels (`make asm`, dbde_project_kernels.s; no GPU).

dbde16_hip_project launches one project16_kernel instance per statistics set (15) and project16_combine_kernel.  They
keep the 8-bit kernels' budget: no scratch, no dynamic stack, at most 512 bytes of LDS and 128 VGPRs
(at least 4 waves per SIMD).
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dbde-video-cpp_amd", "csrc")

LDS_BUDGET = 512      # bytes per workgroup
VGPR_BUDGET = 128     # per lane: 4 waves per SIMD
COMBINE16 = "_ZN4dbde24project16_combine_kernelENS_10ProjParamsE"


@pytest.fixture(scope="module")
def kernels():
    r = subprocess.run(["make", "-s", "-C", CSRC, "asm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    meta = open(os.path.join(CSRC, "dbde_project_kernels.s")).read()
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", meta, re.S):
        fields = dict(re.findall(r"\.amdhsa_(\w+) (\d+)", m.group(2)))
        out[m.group(1)] = {k: int(v) for k, v in fields.items()}
    return out


def instances16(kernels):
    got = {}
    for name, f in kernels.items():
        m = re.match(r"_ZN4dbde16project16_kernelILj(\d+)EEEvNS_10ProjParamsE$", name)
        if m:
            got[int(m.group(1))] = f
    return got


def test_one_instance_per_statistics_set(kernels):
    assert sorted(instances16(kernels)) == list(range(1, 16))
    assert COMBINE16 in kernels
    assert len([k for k in kernels if "project16" in k]) == 16


def test_no_scratch_and_within_budget(kernels):
    names = [k for k in kernels if "project16" in k]
    for name in names:
        f = kernels[name]
        assert f["private_segment_fixed_size"] == 0, (name, "scratch")
        assert not f.get("uses_dynamic_stack", 0), name
        assert f["group_segment_fixed_size"] <= LDS_BUDGET, (name, f["group_segment_fixed_size"])
        assert f["next_free_vgpr"] <= VGPR_BUDGET, (name, f["next_free_vgpr"])


def test_fewer_statistics_cost_fewer_registers(kernels):
    """An unrequested statistic has no accumulators: max + min alone needs fewer VGPRs than all four (whose U64 sums
    of squares take 8)."""
    inst = instances16(kernels)
    assert inst[3]["next_free_vgpr"] < inst[15]["next_free_vgpr"]
