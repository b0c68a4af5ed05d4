"""CPU, compile only: the gfx950 listing of the patch moments' kernels (`make asm`, dbde_moment_kernels.s; no GPU).

dbde_hip_patch_moments launches patch_moments_kernel<1>, dbde16_hip_patch_moments patch_moments_kernel<2>: 64-lane
workgroups, one tile per lane.  Their resources are part of the design: no scratch, no dynamic stack,
the LDS the plan reports (the rows' payload ranges: 4096 bytes per pixel byte plus 32 for each of up to 64 tile rows),
and the VGPR figure of each instance pinned at the listing's: 72 for DBDE, 97 for DBDE16 (92 registers and the
accumulation offset).

What that means for occupancy: 72 allocated VGPRs admit 512 / 72 = 7 waves per SIMD, the 6,144 bytes of LDS 26 one-wave
workgroups per CU = 6.5 per SIMD; 104 allocated VGPRs admit 4 waves per SIMD, the 10,240 bytes 16 workgroups per CU = 4
per SIMD.  In both instances the registers admit at least what the LDS admits.
"""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dbde-video-cpp_amd", "csrc")
sys.path.insert(0, ROOT)

VGPRS = {1: 72, 2: 97}        # next_free_vgpr of the listing, pinned
LDS = {1: 6144, 2: 10240}


def name(pix):
    return f"_ZN4dbde20patch_moments_kernelILj{pix}EEEvNS_12MomentParamsE"


@pytest.fixture(scope="module")
def kernels():
    r = subprocess.run(["make", "-s", "-C", CSRC, "asm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    listing = open(os.path.join(CSRC, "dbde_moment_kernels.s")).read()
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", listing, re.S):
        fields = dict(re.findall(r"\.amdhsa_(\w+) (\d+)", m.group(2)))
        out[m.group(1)] = {k: int(v) for k, v in fields.items()}
    return out


def test_expected_instances_only(kernels):
    assert set(kernels) == {name(1), name(2)}


@pytest.mark.parametrize("pix", (1, 2))
def test_no_scratch_plan_lds_and_pinned_vgprs(kernels, pix):
    f = kernels[name(pix)]
    assert f["private_segment_fixed_size"] == 0, "scratch"
    assert not f.get("uses_dynamic_stack", 0)
    assert f["group_segment_fixed_size"] == LDS[pix]
    assert f["next_free_vgpr"] == VGPRS[pix], f["next_free_vgpr"]   # a drift either way is looked at
    by_vgpr = min(8, 512 // ((VGPRS[pix] + 7) // 8 * 8))             # waves per SIMD the registers admit
    by_lds = (160 * 1024 // LDS[pix]) / 4                            # ... and the LDS (one-wave workgroups, 4 SIMDs per CU)
    assert by_vgpr >= min(8, by_lds), (by_vgpr, by_lds)


def test_plan_reports_the_listing_lds():
    import dbde_video_cpp_amd as dv
    if not os.path.exists(dv.LIB_PATH):
        dv.build()
    assert dv.patch_moments_plan(4096, 3072, 2, 32, 32, 8)["lds_bytes"] == LDS[1]
    assert dv.patch_moments16_plan(4096, 3072, 2, 32, 32, 8)["lds_bytes"] == LDS[2]
