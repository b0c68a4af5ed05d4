"""CPU, compile only: the gfx950 listing of the binned decode's kernel (`make asm`, dbde_binned_kernels.s; no GPU).

dbde_hip_decode_binned (PIX = 1) and dbde16_hip_decode_binned (PIX = 2) launch one binned_kernel<THREADS, PIX, B>
instance: THREADS = 64 tiles per workgroup for windows of at most 64 tiles across, 256 (DBDE16: 128) for wider ones,
B = 2, 4, 8 -- twelve instances.  Their resources are part of the design: no scratch, no dynamic
stack, the LDS the plan reports, and at most 64 VGPRs for DBDE (8 waves per SIMD; the B = 4 and B = 8 instances stay
within 48 and 40) and 88 for DBDE16 (5 waves per SIMD, more than the 4.5 its LDS admits; the compiler declares 81 for
every 16-bit instance, as it does for decode_roi_kernel<T, 2>, while using 68, 50 and 39).
"""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dbde-video-cpp_amd", "csrc")
sys.path.insert(0, ROOT)

VGPR_BUDGET = {1: 64, 2: 88}
BY_BIN = {(1, 4): 48, (1, 8): 40}   # the larger bins hold fewer results
INSTANCES = [(t, pix, b) for pix, ts in ((1, (64, 256)), (2, (64, 128))) for t in ts for b in (2, 4, 8)]
LDS = {(64, 1): 4168, (256, 1): 16480, (64, 2): 8232, (128, 2): 16432}


def name(threads, pix, b):
    return f"_ZN4dbde13binned_kernelILj{threads}ELj{pix}ELj{b}EEEvNS_12BinnedParamsE"


@pytest.fixture(scope="module")
def kernels():
    r = subprocess.run(["make", "-s", "-C", CSRC, "asm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    meta = open(os.path.join(CSRC, "dbde_binned_kernels.s")).read()
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", meta, re.S):
        fields = dict(re.findall(r"\.amdhsa_(\w+) (\d+)", m.group(2)))
        out[m.group(1)] = {k: int(v) for k, v in fields.items()}
    return out


def test_expected_instances_only(kernels):
    assert set(kernels) == {name(*i) for i in INSTANCES}


@pytest.mark.parametrize("threads,pix,b", INSTANCES)
def test_no_scratch_and_within_budget(kernels, threads, pix, b):
    f = kernels[name(threads, pix, b)]
    assert f["private_segment_fixed_size"] == 0, "scratch"
    assert not f.get("uses_dynamic_stack", 0)
    assert f["group_segment_fixed_size"] == LDS[(threads, pix)]
    assert f["next_free_vgpr"] <= BY_BIN.get((pix, b), VGPR_BUDGET[pix]), f["next_free_vgpr"]


def test_plan_reports_the_listing_lds():
    import dbde_video_cpp_amd as dv
    if not os.path.exists(dv.LIB_PATH):
        dv.build()
    for b in (2, 4, 8):
        assert dv.binned_plan(64, 48, 2, b)["lds_bytes"] == LDS[(64, 1)]
        assert dv.binned_plan(4096, 3072, 2, b)["lds_bytes"] == LDS[(256, 1)]
        assert dv.binned16_plan(64, 48, 2, b)["lds_bytes"] == LDS[(64, 2)]
        assert dv.binned16_plan(4096, 3072, 2, b)["lds_bytes"] == LDS[(128, 2)]


def test_byte_sums_by_sad_and_no_memory_writes_but_vector_stores():
    """The 4 x 4 and 8 x 8 byte sums are v_sad_u8 against zero; maxima / minima are packed 16-bit instructions; the
    planes leave as nontemporal 16-byte vector stores (flat ones, as decode_roi_kernel's: the block addresses are
    computed as integers); nothing is written through the scalar unit."""
    text = open(os.path.join(CSRC, "dbde_binned_kernels.s")).read()
    assert "v_sad_u8" in text and "v_pk_max_u16" in text and "v_pk_min_u16" in text
    assert re.search(r"(flat|global)_store_dwordx4 .* nt", text)
    assert not re.search(r"^\s*s_(buffer_|scratch_)?(store|atomic)", text, re.M)
