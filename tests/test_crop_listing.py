"""CPU, compile only: the gfx950 listing of the compressed-domain crop's kernels (`make asm`, dbde_crop_kernels.s).

dbde_hip_crop_frames (PIX = 1) and dbde16_hip_crop_frames (PIX = 2) launch crop_size_kernel<PIX>,
crop_repack_kernel<PIX>, crop_rows_kernel<PIX>, crop_place_kernel and crop_copy_kernel<PIX>: nine instances.  Their
resources are part of the design: no scratch, no dynamic stack, the LDS the plan reports.  The copy
kernel, the one that moves the bytes, and the sizing and scan kernels stay within 32 VGPRs (8 waves per SIMD, the most
there is: each is one dependent chain of loads per workgroup, hidden by occupancy alone); the re-pack kernel holds a
tile's 64 pixels in 32 registers while it pads and packs them and stays within 80 (6 waves per SIMD; the listing has
72), which is no limit to it: a call has at most tiles_x + tiles_y - 1 such threads a frame.
"""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dbde-video-cpp_amd", "csrc")
sys.path.insert(0, ROOT)

KERNELS = {  # mangled name -> (LDS bytes, VGPR budget, the plan's field)
    "_ZN4dbde16crop_size_kernelILj1EEEvNS_10CropParamsE": (48, 32, "size"),
    "_ZN4dbde16crop_size_kernelILj2EEEvNS_10CropParamsE": (48, 32, "size"),
    "_ZN4dbde18crop_repack_kernelILj1EEEvNS_10CropParamsE": (0, 80, "repack"),
    "_ZN4dbde18crop_repack_kernelILj2EEEvNS_10CropParamsE": (0, 80, "repack"),
    "_ZN4dbde16crop_rows_kernelILj1EEEvNS_10CropParamsE": (16, 32, "rows"),
    "_ZN4dbde16crop_rows_kernelILj2EEEvNS_10CropParamsE": (16, 32, "rows"),
    "_ZN4dbde17crop_place_kernelENS_10CropParamsE": (4096, 32, "place"),
    "_ZN4dbde16crop_copy_kernelILj1EEEvNS_10CropParamsE": (0, 32, "copy"),
    "_ZN4dbde16crop_copy_kernelILj2EEEvNS_10CropParamsE": (0, 32, "copy"),
}


@pytest.fixture(scope="module")
def kernels():
    r = subprocess.run(["make", "-s", "-C", CSRC, "asm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    meta = open(os.path.join(CSRC, "dbde_crop_kernels.s")).read()
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", meta, re.S):
        fields = dict(re.findall(r"\.amdhsa_(\w+) (\d+)", m.group(2)))
        out[m.group(1)] = {k: int(v) for k, v in fields.items()}
    return out


def test_expected_instances_only(kernels):
    assert set(kernels) == set(KERNELS)


@pytest.mark.parametrize("name", sorted(KERNELS))
def test_no_scratch_and_within_budget(kernels, name):
    f = kernels[name]
    lds, vgprs, _ = KERNELS[name]
    assert f["private_segment_fixed_size"] == 0, "scratch"
    assert not f.get("uses_dynamic_stack", 0)
    assert f["group_segment_fixed_size"] == lds
    assert f["next_free_vgpr"] <= vgprs, f["next_free_vgpr"]


def test_plan_reports_the_listing_lds():
    import dbde_video_cpp_amd as dv
    if not os.path.exists(dv.LIB_PATH):
        dv.build()
    for plan in (dv.crop_plan(4096, 3072, 2, 1000, 696, 2045, 2043), dv.crop16_plan(64, 48, 2)):
        for lds, _, field in KERNELS.values():
            assert plan[field + "_lds_bytes"] == lds and plan[field + "_threads"] == 256


def test_payload_leaves_as_16_byte_vector_stores_and_nothing_through_the_scalar_unit():
    """The copied payload leaves as nontemporal 16-byte vector stores (flat ones, as decode_roi_kernel's: the block
    addresses are computed as integers); the byte shift between the two alignments is v_alignbyte; no kernel writes
    memory through the scalar unit."""
    text = open(os.path.join(CSRC, "dbde_crop_kernels.s")).read()
    assert re.search(r"(flat|global)_store_dwordx4 .* nt", text)
    assert "v_alignbyte_b32" in text
    assert not re.search(r"^\s*s_(buffer_|scratch_)?(store|atomic)", text, re.M)
