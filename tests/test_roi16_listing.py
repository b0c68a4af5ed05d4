"""CPU, compile only: the gfx950 listing of the DBDE16 window kernel (`make asm`, dbde_roi_kernels.s; no GPU).

decode_roi16_kernel hides its latency by occupancy alone, so its resources are part of its design:
no instance may use scratch, and each stays within the LDS budget that keeps at least 9 workgroups per CU (160 KiB of
LDS per CU): 64-tile pieces in 8.25 KiB, 128-tile pieces in 16.25 KiB.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dbde-video-cpp_amd", "csrc")

LDS_BUDGET = {64: 8448, 128: 16640}   # bytes per workgroup
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def kernels():
    r = subprocess.run(["make", "-s", "-C", CSRC, "asm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    meta = open(os.path.join(CSRC, "dbde_roi_kernels.s")).read()
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", meta, re.S):
        fields = dict(re.findall(r"\.amdhsa_(\w+) (\d+)", m.group(2)))
        out[m.group(1)] = {k: int(v) for k, v in fields.items()}
    return out


def instances(kernels):
    got = {}
    for name, f in kernels.items():
        m = re.match(r"_ZN4dbde19decode_roi16_kernelILj(\d+)EEEvNS_9RoiParamsE$", name)
        if m:
            got[int(m.group(1))] = f
    return got


def test_roi16_instances_are_built(kernels):
    assert sorted(instances(kernels)) == [64, 128]


def test_roi16_uses_no_scratch_and_fits_its_lds_budget(kernels):
    for threads, f in instances(kernels).items():
        assert f["private_segment_fixed_size"] == 0, (threads, "scratch")
        assert not f.get("uses_dynamic_stack", 0), threads
        lds = f["group_segment_fixed_size"]
        assert lds >= threads * 128, (threads, lds)            # a whole piece of depth-16 tiles fits
        assert lds <= LDS_BUDGET[threads], (threads, lds)
        assert LDS_PER_CU // lds >= 9, (threads, lds)
