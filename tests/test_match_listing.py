"""CPU, compile only: the gfx950 listing of the patch match's kernels (`make asm`, dbde_match_kernels.s; no GPU).

dbde_hip_match_patches launches match_patches_kernel<1>, dbde16_hip_match_patches match_patches_kernel<2>: 256-lane
workgroups.  Their resources are part of the design: no scratch, no dynamic stack, no static LDS (all
of it is dynamic and sized per launch: static plus dynamic equals the plan's lds_bytes), and the VGPR figure of each
instance pinned at the listing's: 122 for DBDE, 127 for DBDE16.  Both admit 4 waves per SIMD, which is 4 workgroups per
CU; a 48 x 48 search patch takes under 16 KiB of LDS, so the registers, not the LDS, set the occupancy there.

The 8-bit instance must hold v_dot4_u32_u8 (the three surfaces' inner step), the 16-bit instance v_mad_u64_u32 (one
16-bit product pair can pass 32 bits, so it accumulates in 64).
"""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dbde-video-cpp_amd", "csrc")
sys.path.insert(0, ROOT)

VGPRS = {1: 122, 2: 127}        # next_free_vgpr of the listing, pinned


def name(pix):
    return f"_ZN4dbde20match_patches_kernelILj{pix}EEEvNS_11MatchParamsE"


@pytest.fixture(scope="module")
def listing():
    r = subprocess.run(["make", "-s", "-C", CSRC, "asm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return open(os.path.join(CSRC, "dbde_match_kernels.s")).read()


@pytest.fixture(scope="module")
def kernels(listing):
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", listing, re.S):
        fields = dict(re.findall(r"\.amdhsa_(\w+) (\d+)", m.group(2)))
        out[m.group(1)] = {k: int(v) for k, v in fields.items()}
    return out


def body(listing, pix):
    """The instructions of one instance: from its label to its s_endpgm-terminated end marker."""
    m = re.search(rf"^{re.escape(name(pix))}:[^\n]*\n(.*?)^\.Lfunc_end\d+:", listing, re.S | re.M)
    assert m, "kernel body not found"
    return m.group(1)


def test_expected_instances_only(kernels):
    assert set(kernels) == {name(1), name(2)}


@pytest.mark.parametrize("pix", (1, 2))
def test_no_scratch_no_static_lds_and_pinned_vgprs(kernels, pix):
    f = kernels[name(pix)]
    assert f["private_segment_fixed_size"] == 0, "scratch"
    assert not f.get("uses_dynamic_stack", 0)
    assert f["group_segment_fixed_size"] == 0, "the LDS is dynamic: the plan's lds_bytes is all of it"
    assert f["next_free_vgpr"] == VGPRS[pix], f["next_free_vgpr"]   # a drift either way is looked at
    assert 512 // ((VGPRS[pix] + 7) // 8 * 8) >= 4                   # 4 waves per SIMD: 4 workgroups of 4 waves per CU


def test_inner_steps_are_in_the_bodies(listing):
    b1, b2 = body(listing, 1), body(listing, 2)
    assert b1.count("v_dot4_u32_u8") >= 3, "prod, sum and sq of 8-bit pixels are one v_dot4_u32_u8 each"
    assert "v_mad_u64_u32" in b2, "16-bit products are accumulated in 64 bits"
    assert "v_dot4_u32_u8" not in b2
    for b in (b1, b2):
        assert "v_alignbyte_b32" in b and "scratch_" not in b


def test_plan_lds_is_the_launch_lds():
    """All of the kernel's LDS is dynamic, and the launch passes the plan's figure (the call and the plan share
    plan_match): largest and a usual size, both pixel sizes, within what one workgroup may declare."""
    import dbde_video_cpp_amd as dv
    if not os.path.exists(dv.LIB_PATH):
        dv.build()
    for fn in (dv.match_plan, dv.match16_plan):
        assert 0 < fn(4096, 3072, 2, 32, 32, 8, 8)["lds_bytes"] < fn(4096, 3072, 2, 128, 128, 16, 8)["lds_bytes"] <= 163840
