"""CPU, compile only: the gfx950 listing of the lag projection kernels (`make asm`, dbde_lag_kernels.s; no GPU).

dbde_hip_project_lag (PIX = 1) and dbde16_hip_project_lag (PIX = 2) launch lag_kernel<STATS, PIX> with STATS the instance
that serves the requested statistics -- 3 (product, pairsum), 28 (absdiff, sqdiff, maxdiff) or 31 (all five) -- followed
with several segments by lag_combine_kernel<PIX, ACC>.  Every instance keeps its sums in registers on top of
project_kernel's pipeline and the history ring in LDS: no scratch, no dynamic stack, the LDS the plan reports, and the
VGPR count of DESIGN.md 4.21's table, within the 256 architectural VGPRs of a 256-lane workgroup.  Only `.amdhsa_*`
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

INSTANCES = (3, 28, 31)
# next_free_vgpr of lag_kernel<STATS, PIX>
VGPRS = {(3, 1): 103, (28, 1): 115, (31, 1): 131, (3, 2): 112, (28, 2): 112, (31, 2): 129}
COMBINE_LDS = 32      # write_scalars' wave counts


@pytest.fixture(scope="module")
def kernels():
    r = subprocess.run(["make", "-s", "-C", CSRC, "asm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    meta = open(os.path.join(CSRC, "dbde_lag_kernels.s")).read()
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", meta, re.S):
        fields = dict(re.findall(r"\.amdhsa_(\w+) (\d+)", m.group(2)))
        out[m.group(1)] = {k: int(v) for k, v in fields.items()}
    return out


def name(stats, pix):
    return f"_ZN4dbde10lag_kernelILj{stats}ELj{pix}EEEvNS_9LagParamsE"


COMBINE = {f"_ZN4dbde18lag_combine_kernelILj{pix}ELb{a}EEEvNS_9LagParamsE" for pix in (1, 2) for a in (0, 1)}


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
    plan = dv.lag_plan if pix == 1 else dv.lag16_plan
    for mask in range(1, 32):
        p = plan(64, 64, 10, stats=mask)
        assert p["instance"] in INSTANCES and p["instance"] & mask == mask      # a superset of the request
        assert kernels[name(p["instance"], pix)]["group_segment_fixed_size"] == p["lds_bytes"], mask
    assert plan(64, 64, 10)["lds_bytes"] == 8 * 256 * 8 + 2 * 4 * 2 * 16 + 32      # the ring, the wave totals, the scalars'
    for k in COMBINE:
        assert kernels[k]["group_segment_fixed_size"] == COMBINE_LDS


@pytest.mark.parametrize("pix", (1, 2))
def test_vgprs_are_pinned_and_spill_free(kernels, pix):
    for stats in INSTANCES:
        f = kernels[name(stats, pix)]
        assert f["next_free_vgpr"] == VGPRS[(stats, pix)], (stats, pix, f["next_free_vgpr"])
        assert f["next_free_vgpr"] <= 256
