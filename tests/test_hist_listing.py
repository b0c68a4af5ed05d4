"""CPU, compile only: the gfx950 listing of the histogram kernels (`make asm`, dbde_hist_kernels.s; no GPU).

dbde_hip_histogram (PIX = 1) and dbde16_hip_histogram (PIX = 2) launch hist_init_kernel and one hist_kernel<PIX, NB>
instance: NB = 256 bins (one LDS copy per wave) for DBDE and for DBDE16 up to 256 bins, NB = 4096 (one shared copy)
for DBDE16 above.  Their resources are part of the design: no scratch, no dynamic stack, the LDS the
plan reports (4,352 / 16,640 bytes) and at most 96 VGPRs, so that 5 waves per SIMD stay resident.
"""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dbde-video-cpp_amd", "csrc")
sys.path.insert(0, ROOT)

VGPR_BUDGET = 96
INIT = "_ZN4dbde16hist_init_kernelENS_10HistParamsE"
LDS = {(1, 256): 4352, (2, 256): 4352, (2, 4096): 16640}


def name(pix, nb):
    return f"_ZN4dbde11hist_kernelILj{pix}ELj{nb}EEEvNS_10HistParamsE"


@pytest.fixture(scope="module")
def kernels():
    r = subprocess.run(["make", "-s", "-C", CSRC, "asm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    meta = open(os.path.join(CSRC, "dbde_hist_kernels.s")).read()
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", meta, re.S):
        fields = dict(re.findall(r"\.amdhsa_(\w+) (\d+)", m.group(2)))
        out[m.group(1)] = {k: int(v) for k, v in fields.items()}
    return out


def test_expected_instances_only(kernels):
    assert set(kernels) == {INIT} | {name(pix, nb) for pix, nb in LDS}


@pytest.mark.parametrize("pix,nb", sorted(LDS))
def test_no_scratch_and_within_budget(kernels, pix, nb):
    f = kernels[name(pix, nb)]
    assert f["private_segment_fixed_size"] == 0, "scratch"
    assert not f.get("uses_dynamic_stack", 0)
    assert f["group_segment_fixed_size"] == LDS[(pix, nb)]
    assert f["next_free_vgpr"] <= VGPR_BUDGET, f["next_free_vgpr"]


def test_init_kernel(kernels):
    f = kernels[INIT]
    assert f["private_segment_fixed_size"] == 0 and f["group_segment_fixed_size"] == 0
    assert not f.get("uses_dynamic_stack", 0)


def test_plan_reports_the_listing_lds():
    import dbde_video_cpp_amd as dv
    if not os.path.exists(dv.LIB_PATH):
        dv.build()
    assert dv.histogram_plan(64, 48, 2)["lds_bytes"] == LDS[(1, 256)]
    assert dv.histogram16_plan(64, 48, 2, bins=256)["lds_bytes"] == LDS[(2, 256)]
    assert dv.histogram16_plan(64, 48, 2)["lds_bytes"] == LDS[(2, 4096)]


def test_lds_and_global_atomics_without_compare_and_swap():
    """Counts go to LDS with ds_add_u32, out with U32 / U64 global atomic adds: no compare-and-swap loop."""
    text = open(os.path.join(CSRC, "dbde_hist_kernels.s")).read()
    assert "ds_add_u32" in text and "global_atomic_add_x2" in text and "global_atomic_add " in text
    assert "cmpswap" not in text
