"""CPU, compile only: the gfx950 listing of the region trace kernels (`make asm`, dbde_trace_kernels.s; no GPU).

dbde_hip_traces (PIX = 1) and dbde16_hip_traces (PIX = 2) launch trace_init_kernel, one trace_kernel<STATS, PIX>
instance per statistics set (every non-empty subset of max, min, sum and sumsq: 15) and, for max or min,
trace_finish_kernel<PIX>.  Their resources are part of the design: no instance may use scratch or a
dynamic stack, each keeps its LDS within 1,024 bytes (the offsets and run exchanges, the span's tile words) and its
VGPRs within 128, so that at least 4 waves per SIMD -- 4 workgroups of 256 threads per CU -- stay resident.
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dbde-video-cpp_amd", "csrc")

LDS_BUDGET = 1024     # bytes per workgroup
VGPR_BUDGET = 128     # per lane: 4 waves per SIMD
PIXES = (1, 2)        # DBDE, DBDE16
INIT = "_ZN4dbde17trace_init_kernelENS_11TraceParamsE"


@pytest.fixture(scope="module")
def kernels():
    r = subprocess.run(["make", "-s", "-C", CSRC, "asm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    meta = open(os.path.join(CSRC, "dbde_trace_kernels.s")).read()
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", meta, re.S):
        fields = dict(re.findall(r"\.amdhsa_(\w+) (\d+)", m.group(2)))
        out[m.group(1)] = {k: int(v) for k, v in fields.items()}
    return out


def finish(pix):
    return f"_ZN4dbde19trace_finish_kernelILj{pix}EEEvNS_11TraceParamsE"


def expected(pix):
    return {finish(pix)} | {f"_ZN4dbde12trace_kernelILj{s}ELj{pix}EEEvNS_11TraceParamsE" for s in range(1, 16)}


def instances(kernels, pix):
    got = {}
    for name, f in kernels.items():
        m = re.match(r"_ZN4dbde12trace_kernelILj(\d+)ELj(\d+)EEEvNS_11TraceParamsE$", name)
        if m and int(m.group(2)) == pix:
            got[int(m.group(1))] = f
    return got


@pytest.mark.parametrize("pix", PIXES)
def test_one_instance_per_statistics_set(kernels, pix):
    assert sorted(instances(kernels, pix)) == list(range(1, 16))
    assert finish(pix) in kernels


def test_no_other_trace_kernels(kernels):
    assert set(kernels) == expected(1) | expected(2) | {INIT}


@pytest.mark.parametrize("pix", PIXES)
def test_no_scratch_and_within_budget(kernels, pix):
    for name in sorted(expected(pix) | {INIT}):
        f = kernels[name]
        assert f["private_segment_fixed_size"] == 0, (name, "scratch")
        assert not f.get("uses_dynamic_stack", 0), name
        assert f["group_segment_fixed_size"] <= LDS_BUDGET, (name, f["group_segment_fixed_size"])
        assert f["next_free_vgpr"] <= VGPR_BUDGET, (name, f["next_free_vgpr"])


def test_integer_atomics_without_compare_and_swap(kernels):
    """Sums go out as U64 global atomic adds, max / min as U32 umax / umin: no compare-and-swap loop."""
    text = open(os.path.join(CSRC, "dbde_trace_kernels.s")).read()
    assert "global_atomic_add_x2" in text and "global_atomic_umax" in text and "global_atomic_umin" in text
    assert "cmpswap" not in text
