"""CPU, compile only: the gfx950 listing of the scaled float decode's kernel (`make asm`, dbde_scaled_kernels.s; no GPU).

dbde_hip_decode_scaled (PIX = 1) and dbde16_hip_decode_scaled (PIX = 2) launch one decode_scaled_kernel<THREADS, PIX,
OUT> instance: THREADS = 64 tiles per workgroup for windows of at most 64 tiles across, 256 (DBDE16: 128) for wider
ones, OUT = 0, 1, 2 (F32, F16, BF16) -- twelve instances.  Their resources are part of the design: no
scratch, no dynamic stack, the LDS the plan reports (the window decoder's: the band stays in the pixel type), and at
most 40 VGPRs for DBDE (the listing: 30 for F32, 36 for F16 / BF16) and 88 for DBDE16 (the compiler declares 81 for every
16-bit instance, as it does for decode_roi_kernel<T, 2>).

What the budgets buy: 512 VGPRs per SIMD lane give 8 waves per SIMD (the most the hardware holds) up to 64 VGPRs, so 40
leaves the 8-bit kernel bound by its LDS alone: 160 KiB per CU / 16,480 bytes = 9 workgroups of 4 waves = 9 waves per
SIMD of LDS room, more than 8.  88 VGPRs give 5 waves per SIMD, more than the 4.5 that the 16-bit kernel's 16,432 bytes
per 2-wave workgroup admit (9 workgroups = 18 waves per CU).  In both the register file is not what limits the
occupancy that hides the kernel's one dependent load chain.
"""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dbde-video-cpp_amd", "csrc")
sys.path.insert(0, ROOT)

VGPR_BUDGET = {1: 40, 2: 88}
INSTANCES = [(t, pix, o) for pix, ts in ((1, (64, 256)), (2, (64, 128))) for t in ts for o in (0, 1, 2)]
LDS = {(64, 1): 4168, (256, 1): 16480, (64, 2): 8232, (128, 2): 16432}


def name(threads, pix, out):
    return f"_ZN4dbde20decode_scaled_kernelILj{threads}ELj{pix}ELj{out}EEEvNS_12ScaledParamsE"


@pytest.fixture(scope="module")
def listing():
    r = subprocess.run(["make", "-s", "-C", CSRC, "asm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(os.path.join(CSRC, "dbde_scaled_kernels.s")).read()


@pytest.fixture(scope="module")
def kernels(listing):
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", listing, re.S):
        fields = dict(re.findall(r"\.amdhsa_(\w+) (\d+)", m.group(2)))
        out[m.group(1)] = {k: int(v) for k, v in fields.items()}
    return out


def test_expected_instances_only(kernels):
    assert set(kernels) == {name(*i) for i in INSTANCES}


@pytest.mark.parametrize("threads,pix,out", INSTANCES)
def test_no_scratch_and_within_budget(kernels, threads, pix, out):
    f = kernels[name(threads, pix, out)]
    assert f["private_segment_fixed_size"] == 0, "scratch"
    assert not f.get("uses_dynamic_stack", 0)
    assert f["group_segment_fixed_size"] == LDS[(threads, pix)]
    assert f["next_free_vgpr"] <= VGPR_BUDGET[pix], f["next_free_vgpr"]


def test_plan_reports_the_listing_lds():
    import dbde_video_cpp_amd as dv
    if not os.path.exists(dv.LIB_PATH):
        dv.build()
    for t in (0, 1, 2):
        assert dv.scaled_plan(64, 48, 2, dtype=t)["lds_bytes"] == LDS[(64, 1)]
        assert dv.scaled_plan(4096, 3072, 2, dtype=t)["lds_bytes"] == LDS[(256, 1)]
        assert dv.scaled16_plan(64, 48, 2, dtype=t)["lds_bytes"] == LDS[(64, 2)]
        assert dv.scaled16_plan(4096, 3072, 2, dtype=t)["lds_bytes"] == LDS[(128, 2)]


def test_packed_bf16_conversion_and_nontemporal_block_stores(listing):
    """BF16 results are rounded by gfx950's packed conversion, and the output leaves as nontemporal 16-byte vector
    stores (flat ones, as decode_roi_kernel's: the block addresses are computed as integers)."""
    assert "v_cvt_pk_bf16_f32" in listing
    assert re.search(r"(flat|global)_store_dwordx4 .* nt", listing)
