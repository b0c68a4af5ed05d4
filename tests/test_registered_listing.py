"""CPU, compile only: the gfx950 listing of the registered projection kernels (`make asm`, dbde_rproject_kernels.s; no
GPU).

dbde_hip_project_registered (PIX = 1) and dbde16_hip_project_registered (PIX = 2) launch rproject_kernel<STATS, PIX>
with STATS the instance that serves the requested statistics -- 3 (max, min), 12 (sum, sumsq) or 15 (all four) --
followed with several segments by project's combine kernel (dbde_project_kernels.s).  Every instance keeps its
accumulators in registers and the re-aligning band in LDS: no scratch, no dynamic stack, the LDS the plan reports, and
the VGPR count of DESIGN.md 4.22's table, within the 256 architectural VGPRs of a 256-lane workgroup.  Only `.amdhsa_*`
fields are read.
"""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dbde-video-cpp_amd", "csrc")
sys.path.insert(0, ROOT)

INSTANCES = (3, 12, 15)
# next_free_vgpr of rproject_kernel<STATS, PIX>
VGPRS = {(3, 1): 102, (12, 1): 110, (15, 1): 118, (3, 2): 105, (12, 2): 112, (15, 2): 116}


@pytest.fixture(scope="module")
def kernels():
    r = subprocess.run(["make", "-s", "-C", CSRC, "asm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    meta = open(os.path.join(CSRC, "dbde_rproject_kernels.s")).read()
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", meta, re.S):
        fields = dict(re.findall(r"\.amdhsa_(\w+) (\d+)", m.group(2)))
        out[m.group(1)] = {k: int(v) for k, v in fields.items()}
    return out


def name(stats, pix):
    return f"_ZN4dbde15rproject_kernelILj{stats}ELj{pix}EEEvNS_11RProjParamsE"


def test_six_instances(kernels):
    assert set(kernels) == {name(m, pix) for m in INSTANCES for pix in (1, 2)}


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
    plan = dv.registered_plan if pix == 1 else dv.registered16_plan
    for mask in range(1, 16):
        p = plan(64, 64, 10, 40, 40, stats=mask)
        assert p["instance"] in INSTANCES and p["instance"] & mask == mask      # a superset of the request
        assert kernels[name(p["instance"], pix)]["group_segment_fixed_size"] == p["lds_bytes"], mask
    # the band (two groups of four frames, 8 rows of 68 dwords), the wave totals of two tile rows, the count's
    assert plan(64, 64, 10, 40, 40)["lds_bytes"] == 2 * 4 * 8 * 68 * 4 + 2 * 4 * 2 * 32 + 16


@pytest.mark.parametrize("pix", (1, 2))
def test_vgprs_are_pinned_and_spill_free(kernels, pix):
    for stats in INSTANCES:
        f = kernels[name(stats, pix)]
        assert f["next_free_vgpr"] == VGPRS[(stats, pix)], (stats, pix, f["next_free_vgpr"])
        assert f["next_free_vgpr"] <= 256
