"""CPU, compile only: the gfx950 listing of the window kernel (`make asm`, dbde_roi_kernels.s; no GPU).

decode_roi_kernel<THREADS, PIX> hides its latency by occupancy alone, so its resources are part of its
design: no instance may use scratch or a dynamic stack.  The DBDE16 instances (PIX = 2) each stay within the LDS budget
that keeps at least 9 workgroups per CU (160 KiB of LDS per CU): 64-tile pieces in 8.25 KiB, 128-tile pieces in
16.25 KiB.  The 8-bit instances (PIX = 1) use no more LDS than they did as a kernel of their own: 4,168 / 16,480 bytes.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dbde-video-cpp_amd", "csrc")

LDS_BUDGET = {64: 8448, 128: 16640}   # bytes per workgroup
LDS_BUDGET_8 = {64: 4168, 256: 16480}
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


def instances(kernels, pix=2):
    got = {}
    for name, f in kernels.items():
        m = re.match(r"_ZN4dbde17decode_roi_kernelILj(\d+)ELj(\d)EEEvNS_9RoiParamsE$", name)
        if m and int(m.group(2)) == pix:
            got[int(m.group(1))] = f
    return got


def test_window_instances_are_built(kernels):
    assert sorted(instances(kernels, pix=1)) == [64, 256]
    assert sorted(instances(kernels, pix=2)) == [64, 128]


def test_roi16_uses_no_scratch_and_fits_its_lds_budget(kernels):
    got = instances(kernels, pix=2)
    assert got
    for threads, f in got.items():
        assert f["private_segment_fixed_size"] == 0, (threads, "scratch")
        assert not f.get("uses_dynamic_stack", 0), threads
        lds = f["group_segment_fixed_size"]
        assert lds >= threads * 128, (threads, lds)            # a whole piece of depth-16 tiles fits
        assert lds <= LDS_BUDGET[threads], (threads, lds)
        assert LDS_PER_CU // lds >= 9, (threads, lds)


def test_roi8_uses_no_scratch_and_keeps_its_lds(kernels):
    got = instances(kernels, pix=1)
    assert got
    for threads, f in got.items():
        assert f["private_segment_fixed_size"] == 0, (threads, "scratch")
        assert not f.get("uses_dynamic_stack", 0), threads
        lds = f["group_segment_fixed_size"]
        assert lds >= threads * 64, (threads, lds)             # a whole piece of depth-8 tiles fits
        assert lds <= LDS_BUDGET_8[threads], (threads, lds)
