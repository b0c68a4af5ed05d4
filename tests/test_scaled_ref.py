"""CPU: tests/scaled_ref.py, the numpy definition of the scaled float decode, against torch on the CPU.

The helper's bit patterns equal ((p.float() - dark) * gain).to(dtype) of torch for U8 and U16 pixels in all three
output types; its BF16 rounding is round-to-nearest-even on crafted ties; and the standard maps stay inside the range
that keeps the reference independent of denormal modes while still producing +-0, F16 infinities and F16 subnormals.
"""
import numpy as np
import pytest
import torch

import scaled_ref as sr

N = 1 << 20
SHAPE = (1024, 1024)


def torch_bits(p, dark, gain, t):
    # (uint16 has no .float() in every torch build: widen on the numpy side, exactly)
    x = torch.from_numpy(p.astype(np.int32)).float()
    v = ((x - torch.from_numpy(dark)) * torch.from_numpy(gain)).to(sr.torch_dtype(t))
    return v.view(torch.int32 if t == "f32" else torch.int16).numpy().view(sr.BITS[t])


@pytest.fixture(scope="module", params=[8, 16])
def sample(request):
    bits = request.param
    rng = np.random.default_rng(2024 + bits)
    p = rng.integers(0, 1 << bits, SHAPE).astype(np.uint8 if bits == 8 else np.uint16)
    if bits == 16:   # values around the dark level too, so that small differences occur
        p[::2] = rng.integers(0, 320, (SHAPE[0] // 2, SHAPE[1]))
    dark, gain = sr.maps(7 + bits, SHAPE[1], SHAPE[0], pixels=p)
    return p, dark, gain


@pytest.mark.parametrize("t", sr.TYPES)
def test_numpy_and_torch_agree_bit_for_bit(sample, t):
    p, dark, gain = sample
    assert p.size == N
    got, want = sr.scaled_bits(p, dark, gain, t), torch_bits(p, dark, gain, t)
    assert got.dtype == want.dtype and np.array_equal(got, want)


def test_scalars_agree_too(sample):
    p = sample[0]
    for d0, g0 in ((0.0, 1.0 / 255.0), (12.5, -3.0), (0.0, 1.0)):
        for t in sr.TYPES:
            d = np.full(SHAPE, d0, np.float32)
            g = np.full(SHAPE, g0, np.float32)
            assert np.array_equal(sr.scaled_bits(p, np.float32(d0), np.float32(g0), t), torch_bits(p, d, g, t))


def test_standard_maps_stay_in_range_and_reach_the_edge_cases(sample):
    p, dark, gain = sample
    assert dark.dtype == np.float32 and gain.dtype == np.float32
    assert dark.min() >= 0.0 and (dark.max() < 300.0 or p.dtype == np.uint16)
    assert (dark != np.floor(dark)).any()
    a = np.abs(gain)
    assert a.min() >= 2.0 ** -8 and a.max() <= 2.0 ** 8 and (gain > 0).any() and (gain < 0).any()
    d = np.subtract(p.astype(np.float32), dark, dtype=np.float32)
    v = sr.value(p, dark, gain)
    for x in (d, v):   # no subnormal binary32 intermediate
        nz = np.abs(x[x != 0])
        assert nz.min() >= sr.F32_MIN_NORMAL
    zero = sr.scaled_bits(p, dark, gain, "f32")[d == 0]
    assert (zero == 0).any() and (zero == 0x80000000).any(), "+0 and -0 both occur"
    h = sr.scaled_bits(p, dark, gain, "f16")
    assert ((h & 0x7FFF) == 0x7C00).any(), "F16 overflow to inf occurs"
    assert (((h & 0x7C00) == 0) & ((h & 0x03FF) != 0)).any(), "F16 subnormals occur"
    assert not ((h & 0x7FFF) > 0x7C00).any(), "no NaN"


def test_bf16_rounding_ties_to_even():
    cases = {
        0x3F800000: 0x3F80,   # exact
        0x3F808000: 0x3F80,   # tie, even below: stays
        0x3F818000: 0x3F82,   # tie, odd below: up to even
        0x3F808001: 0x3F81,   # above the tie: up
        0x3F807FFF: 0x3F80,   # below the tie: down
        0xBF818000: 0xBF82,   # the same with the sign set
        0x7F7F8000: 0x7F80,   # tie at the largest finite value: to inf
        0x7F7FFFFF: 0x7F80,
        0x00008000: 0x0000,   # subnormal tie to even (zero)
        0x00018000: 0x0002,   # subnormal tie, odd below
        0x80000000: 0x8000,   # -0
        0x7F800000: 0x7F80,   # inf
    }
    bits = np.array(list(cases), np.uint32)
    got = sr.bf16_bits(bits.view(np.float32))
    assert got.tolist() == list(cases.values())
    want = torch.from_numpy(bits.view(np.float32).copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(got, want)
    nan = sr.bf16_bits(np.array([np.nan], np.float32))
    assert (nan & 0x7F80) == 0x7F80 and (nan & 0x007F) != 0


def test_expected_takes_the_maps_at_clamped_frame_coordinates():
    rng = np.random.default_rng(3)
    W, H, n, rw, rh = 23, 17, 4, 7, 5
    img = rng.integers(0, 256, (n, H, W)).astype(np.uint8)
    dark, gain = sr.maps(1, W, H)
    org = np.array([[-5, 2], [3, 100], [16, 12], [40, -1]])
    cl = sr.clamp_origins(org, W, H, rw, rh)
    assert cl.tolist() == [[0, 2], [3, 12], [16, 12], [16, 0]]
    got = sr.expected(img, 0, 0, rw, rh, dark, gain, "f32", origins=org)
    for f, (x, y) in enumerate(cl):
        for j in range(rh):
            for i in range(rw):
                v = (np.float32(img[f, y + j, x + i]) - dark[y + j, x + i]) * gain[y + j, x + i]
                assert got[f, j, i] == np.float32(v).view(np.uint32)
