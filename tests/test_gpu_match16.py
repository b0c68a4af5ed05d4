"""GPU: patch match of DBDE16 streams -- dbde16_hip_match_patches (Codec.match_patches16).

As tests/test_gpu_match.py over U16 pixels: the same cases of tests/match_cases.py with 16-bit noise, exact equality with
tests/match_ref.py.  The all-65535 witness pins the 64-bit accumulation: one product pair already passes 32 bits.
"""
import pytest

import match_cases as mc
import match_gpu as mg

pytestmark = pytest.mark.gpu

BITS = 16


@pytest.fixture(scope="module")
def dv():
    import dbde_video_cpp_amd as m
    return m


@pytest.fixture(scope="module")
def codec(dv):
    c = dv.Codec(0)
    assert c.arch.startswith("gfx950")
    yield c
    c.close()


@pytest.mark.parametrize("c", mc.CASES, ids=mc.IDS)
def test_cases16_match_match_ref(codec, c):
    mg.run_case(codec, c, BITS)


def test_rejected_and_truncated_frames16_stay_untouched(codec):
    mg.run_rejected(codec, BITS)


def test_overflow_witness_all_65535(codec):
    mg.run_overflow_witness(codec, BITS)


def test_decode_patches16_plus_torch_agree(codec):
    mg.run_cross_check(codec, BITS)
