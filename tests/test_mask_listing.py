"""CPU, compile only: the gfx950 listing of the threshold mask decode's kernels (`make asm`, dbde_mask_kernels.s; no GPU).

dbde_hip_decode_mask (PIX = 1) and dbde16_hip_decode_mask (PIX = 2) launch mask_init_kernel (when counts or boxes are
asked for) and one decode_mask_kernel<THREADS, PIX> instance: THREADS = 64 for windows of at most 7 mask words, 256
(DBDE16: 128) for wider ones -- four instances.  Their resources are part of the design: no scratch, no
dynamic stack, the LDS the plan reports, and the VGPR number of every instance pinned at the listing's figure (30 and 32
for DBDE, 81 for both DBDE16 instances), within the budgets the occupancy argument needs: 32 for DBDE, 88 for DBDE16
(the compiler declares 81 for both 16-bit instances, as it does for decode_roi_kernel<T, 2>: 46 registers and an
accumulation offset of 48).

What the budgets buy: 512 VGPRs per SIMD lane give 8 waves per SIMD (the most the hardware holds) up to 64 VGPRs, so the
8-bit kernel is bound by its LDS alone: the wide form's 16,704 bytes admit 160 KiB / 16,704 = 9 workgroups of 4 waves per
CU = 9 waves per SIMD, more than 8, and the narrow form's 4,240 bytes 38 one-wave workgroups = 9.5 waves per SIMD.  88
VGPRs give 5 waves per SIMD, more than the 4.5 that the 16-bit wide form's 16,608 bytes per 2-wave workgroup admit (9
workgroups = 18 waves per CU) and the 4.75 of the narrow form's 8,336 bytes (19 one-wave workgroups).  In every form the
register file is not what limits the occupancy that hides the kernel's one dependent load chain;
test_no_scratch_plan_lds_and_within_budget restates the comparison.
"""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dbde-video-cpp_amd", "csrc")
sys.path.insert(0, ROOT)

VGPR_BUDGET = {1: 32, 2: 88}   # what the occupancy argument needs
VGPRS = {(64, 1): 30, (256, 1): 32, (64, 2): 81, (128, 2): 81}   # next_free_vgpr of the listing, pinned
INSTANCES = [(64, 1), (256, 1), (64, 2), (128, 2)]
LDS = {(64, 1): 4240, (256, 1): 16704, (64, 2): 8336, (128, 2): 16608}
INIT = "_ZN4dbde16mask_init_kernelEPjPijii"


def name(threads, pix):
    return f"_ZN4dbde18decode_mask_kernelILj{threads}ELj{pix}EEEvNS_10MaskParamsE"


@pytest.fixture(scope="module")
def kernels():
    r = subprocess.run(["make", "-s", "-C", CSRC, "asm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    listing = open(os.path.join(CSRC, "dbde_mask_kernels.s")).read()
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", listing, re.S):
        fields = dict(re.findall(r"\.amdhsa_(\w+) (\d+)", m.group(2)))
        out[m.group(1)] = {k: int(v) for k, v in fields.items()}
    return out


def test_expected_instances_only(kernels):
    assert set(kernels) == {name(*i) for i in INSTANCES} | {INIT}


@pytest.mark.parametrize("threads,pix", INSTANCES)
def test_no_scratch_plan_lds_and_within_budget(kernels, threads, pix):
    f = kernels[name(threads, pix)]
    assert f["private_segment_fixed_size"] == 0, "scratch"
    assert not f.get("uses_dynamic_stack", 0)
    assert f["group_segment_fixed_size"] == LDS[(threads, pix)]
    assert f["next_free_vgpr"] == VGPRS[(threads, pix)], f["next_free_vgpr"]   # a drift either way is looked at
    assert VGPRS[(threads, pix)] <= VGPR_BUDGET[pix]
    by_vgpr = min(8, 512 // ((VGPR_BUDGET[pix] + 7) // 8 * 8))                       # waves per SIMD the registers admit
    by_lds = (160 * 1024 // LDS[(threads, pix)]) * (threads // 64) / 4               # ... and the LDS (4 SIMDs per CU)
    assert by_vgpr >= min(8, by_lds), (by_vgpr, by_lds)


def test_init_kernel_is_trivial(kernels):
    f = kernels[INIT]
    assert f["private_segment_fixed_size"] == 0 and f["group_segment_fixed_size"] == 0
    assert not f.get("uses_dynamic_stack", 0)


def test_plan_reports_the_listing_lds():
    import dbde_video_cpp_amd as dv
    if not os.path.exists(dv.LIB_PATH):
        dv.build()
    assert dv.mask_plan(64, 48, 2)["lds_bytes"] == LDS[(64, 1)]
    assert dv.mask_plan(4096, 3072, 2)["lds_bytes"] == LDS[(256, 1)]
    assert dv.mask16_plan(64, 48, 2)["lds_bytes"] == LDS[(64, 2)]
    assert dv.mask16_plan(4096, 3072, 2)["lds_bytes"] == LDS[(128, 2)]
