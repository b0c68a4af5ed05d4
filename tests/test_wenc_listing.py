"""CPU, compile only: the gfx950 listing of the window encoder's kernel (`make asm`, dbde_wenc_kernels.s; no GPU).

dbde_hip_encode_window and dbde16_hip_encode_window launch encode_window_kernel<1> and <2>: exactly these two
instances, no scratch, no dynamic stack, the LDS the plan reports (the chunk's worst-case payload image, 4,096 words,
plus the trash word and the few words of workgroup state), and at most 128 VGPRs (the listing: 97 allocated for both).

What the budget buys: the 32,824 bytes of LDS admit 4 workgroups of 4 waves per CU (160 KiB / 32,824 = 4.99), that is
4 waves per SIMD, and 512 VGPRs per SIMD lane hold 4 waves up to 128 VGPRs each: within the budget the register file
never lowers the occupancy below what the LDS already fixes, and the launch bound of 4 waves per SIMD holds.

The pixel fetches are 16-byte nontemporal loads (8 per instance: one per image row of a lane's tile pair / tile); the
byte loads in the listing belong to the path taken within 16 bytes of the end of the readable extent and by windows
narrower than 16 bytes.
"""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dbde-video-cpp_amd", "csrc")
sys.path.insert(0, ROOT)

VGPR_BUDGET = 128
LDS = 32824


def name(pix):
    return f"_ZN4dbde20encode_window_kernelILi{pix}EEEvNS_10WencParamsE"


@pytest.fixture(scope="module")
def listing():
    r = subprocess.run(["make", "-s", "-C", CSRC, "asm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(os.path.join(CSRC, "dbde_wenc_kernels.s")).read()


@pytest.fixture(scope="module")
def kernels(listing):
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", listing, re.S):
        fields = dict(re.findall(r"\.amdhsa_(\w+) (\d+)", m.group(2)))
        out[m.group(1)] = {k: int(v) for k, v in fields.items()}
    return out


def test_exactly_the_two_instances(kernels):
    assert set(kernels) == {name(1), name(2)}


@pytest.mark.parametrize("pix", [1, 2])
def test_no_scratch_lds_and_vgpr_budget(kernels, pix):
    f = kernels[name(pix)]
    assert f["private_segment_fixed_size"] == 0, "scratch"
    assert not f.get("uses_dynamic_stack", 0)
    assert f["group_segment_fixed_size"] == LDS
    assert f["next_free_vgpr"] <= VGPR_BUDGET, f["next_free_vgpr"]


def test_plan_reports_the_listing_lds():
    import dbde_video_cpp_amd as dv
    if not os.path.exists(dv.LIB_PATH):
        dv.build()
    assert dv.window_encode_plan(1500, 1460, 3, 31, 7, 1456, 1448)["lds_bytes"] == LDS
    assert dv.window_encode16_plan(1500, 1460, 3, 31, 7, 1456, 1448)["lds_bytes"] == LDS
    assert dv.window_encode_plan(40, 29, 3, 5, 3, 1, 9)["lds_bytes"] == LDS


def body(listing, pix):
    m = re.search(rf"^{re.escape(name(pix))}:[^\n]*\n(.*?)\n\.Lfunc_end\d+:", listing, re.S | re.M)
    assert m, "kernel body not found"
    return m.group(1)


@pytest.mark.parametrize("pix", [1, 2])
def test_pixel_fetches_are_16_byte_nontemporal_loads(listing, pix):
    loads = re.findall(r"global_load_dwordx4 .* nt", body(listing, pix))
    assert len(loads) == 8, len(loads)
