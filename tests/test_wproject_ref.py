"""CPU: the reference of the weighted projections (tests/wproject_ref.py) -- its fused multiply-add is a true
single-rounding one, a multiply-then-add kernel is told apart from it, and the segment order of the defined value
matters.  No GPU, no library."""
import numpy as np

import wproject_ref as wr


def f32(bits):
    return np.array(bits, np.uint32).view(np.float32)


def check_against_libm(w, p, acc):
    got = wr.fma32(w, p, acc)
    w, p, acc = np.broadcast_arrays(np.asarray(w, np.float32), np.asarray(p), np.asarray(acc, np.float32))
    for i in range(w.size):
        want = wr.fmaf_libm(w.flat[i], p.flat[i], acc.flat[i])
        g = got.flat[i]
        if np.isnan(want):
            assert np.isnan(g), (w.flat[i], p.flat[i], acc.flat[i])
        else:
            assert g.view(np.int32) == want.view(np.int32), (w.flat[i].hex(), int(p.flat[i]), acc.flat[i].hex(), g, want)


def test_fma_equals_libm_on_random_operands():
    rng = np.random.default_rng(1)
    n = 4000
    w = f32(rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32))      # any bit pattern: NaN, inf, subnormal
    acc = f32(rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32))
    p = rng.integers(0, 65536, n)
    check_against_libm(w, p, acc)
    w = rng.standard_normal(n).astype(np.float32)
    acc = (rng.standard_normal(n) * 300).astype(np.float32)
    check_against_libm(w, rng.integers(0, 256, n), acc)


def test_fma_equals_libm_in_the_subnormal_range():
    rng = np.random.default_rng(2)
    n = 3000
    w = (f32(rng.integers(1, 1 << 12, n).astype(np.uint32)) * rng.choice([-1, 1], n)).astype(np.float32)   # subnormal weights
    acc = (f32(rng.integers(0, 1 << 24, n).astype(np.uint32)) * rng.choice([-1, 1], n)).astype(np.float32)
    check_against_libm(w, rng.integers(0, 65536, n), acc)
    check_against_libm(np.float32(1e-42), np.arange(0, 65536, 257), np.float32(0.0))
    check_against_libm(np.float32(1e-42), 65535, f32(rng.integers(0, 1 << 23, 500).astype(np.uint32)))


def test_fma_equals_libm_on_huge_operands():
    big = np.array([1e30, -1e30, 3.4028235e38, 1e35, -3e37], np.float32)
    for p in (0, 1, 2, 255, 256, 65535):
        for acc in (0.0, 1e38, -1e38, 3.4028235e38, -3.4028235e38, np.inf, -np.inf):
            check_against_libm(big, p, np.float32(acc))
    check_against_libm(np.array([np.inf, -np.inf, np.nan], np.float32), np.array([[0], [3]]), np.float32(1.0))


def test_fma_equals_libm_on_ties_and_signed_zeros():
    """Products that land exactly half way between two float32 values of the sum, and sums that cancel to zero."""
    rng = np.random.default_rng(3)
    n = 3000
    # acc = 2^k * odd-ish, w * p = half an ulp of acc (+/- one float64-invisible bit via the product's tail)
    e = rng.integers(-20, 20, n)
    acc = np.ldexp(1.0 + rng.integers(0, 1 << 23, n) * 2.0 ** -23, e).astype(np.float32)
    half_ulp = np.ldexp(1.0, e - 24)
    for p in (1, 3, 255, 4097, 65535):
        for tail in (0.0, 2.0 ** -23, -2.0 ** -23):
            w = (half_ulp / p * (1.0 + tail)).astype(np.float32)
            check_against_libm(w, p, acc)
            check_against_libm(-w, p, acc)
    z = np.array([0.0, -0.0], np.float32)
    check_against_libm(z[:, None], np.array([0, 5]), z[None, :, None])
    check_against_libm(np.float32(2.0), 5, np.float32(-10.0))      # exact cancellation: +0.0
    check_against_libm(np.float32(-2.0), 5, np.float32(10.0))


def test_a_search_finds_witnesses_against_multiply_then_add():
    """For p <= 255 and for p <= 65535 there are (w, p, acc) where round(w * p) + acc differs from the FMA: a kernel that
    multiplies and then adds is told apart.  The named witnesses the GPU tests place are of that kind."""
    rng = np.random.default_rng(4)
    for pmax in (255, 65535):
        w = rng.standard_normal(20000).astype(np.float32)
        p = rng.integers(1, pmax + 1, 20000)
        acc = (-(w.astype(np.float64) * p) * (1.0 + rng.standard_normal(20000) * 1e-3)).astype(np.float32)
        differ = wr.fma32(w, p, acc).view(np.int32) != wr.mul_then_add(w, p, acc).view(np.int32)
        assert differ.any(), pmax
        i = int(np.flatnonzero(differ)[0])
        assert wr.fmaf_libm(w[i], p[i], acc[i]).view(np.int32) == wr.fma32(w[i], p[i], acc[i]).view(np.int32)
    for (w, p, acc), pmax in ((wr.WITNESS_U8, 255), (wr.WITNESS_U16, 65535)):
        assert 0 < p <= pmax
        fused = wr.fmaf_libm(w, p, acc)
        assert fused.view(np.int32) == wr.fma32(w, p, acc).view(np.int32)
        assert fused.view(np.int32) != wr.mul_then_add(w, p, acc).view(np.int32), (w, p, acc)


def test_segment_order_matters():
    """((P_0 + P_1) + P_2) is not (P_0 + (P_1 + P_2)) for a crafted case: the ordering rule is not vacuous, and the
    reference follows the ascending one."""
    img = lambda v: np.full((8, 8), v, np.uint8)   # noqa: E731
    images = [img(1), img(1), img(1)]
    w = np.array([[2.0 ** 24, 1.0, 1.0]], np.float32)
    s3, _ = wr.wproject(images, w, 0, 0, 8, 8, segments=3, fps=1)
    s1, _ = wr.wproject(images, w, 0, 0, 8, 8, segments=1, fps=3)
    assert (s3 == np.float32(2.0 ** 24)).all() and (s1 == s3).all()          # each +1 is lost in turn
    other = np.float32(2.0 ** 24) + (np.float32(1.0) + np.float32(1.0))       # P_0 + (P_1 + P_2)
    assert other == np.float32(2.0 ** 24 + 2) and other != s3[0, 0, 0]
    # and the segmentation itself shows: two segments [2^24, 1 | 1] against [2^24 | 1, 1]
    a, _ = wr.wproject(images, w, 0, 0, 8, 8, segments=2, fps=2)
    b, _ = wr.wproject(images, w[:, ::-1].copy(), 0, 0, 8, 8, segments=2, fps=2)   # [1, 1 | 2^24]: (1 + 1) + 2^24
    assert a[0, 0, 0] == np.float32(2.0 ** 24) and b[0, 0, 0] == np.float32(2.0 ** 24 + 2)


def test_chain_skips_rejected_frames_and_counts():
    rng = np.random.default_rng(5)
    images = [rng.integers(0, 256, (16, 24)).astype(np.uint8) for _ in range(5)]
    images[2] = None
    w = rng.standard_normal((2, 7)).astype(np.float32)
    w[:, 2] = np.nan
    out, count = wr.wproject(images, w, 3, 5, 9, 7)
    assert count == 4 and np.isfinite(out).all() and out.shape == (2, 7, 9)
    for r in range(2):
        acc = np.float32(0.0)
        for f in (0, 1, 3, 4):
            acc = wr.fmaf_libm(w[r, f], images[f][5 + 2, 3 + 4], acc)
        assert acc.view(np.int32) == out[r, 2, 4].view(np.int32)
    prior = rng.standard_normal((2, 7, 9)).astype(np.float32)
    acc2, _ = wr.wproject(images, w, 3, 5, 9, 7, segments=2, fps=3, accumulate=True, prior=prior)
    p0, _ = wr.wproject(images[:3], w, 3, 5, 9, 7)
    p1, _ = wr.wproject(images[3:], w[:, 3:], 3, 5, 9, 7)
    assert np.array_equal(wr.bits(acc2), wr.bits((prior + p0) + p1))
    same, c0 = wr.wproject([], w, 3, 5, 9, 7, accumulate=True, prior=prior)
    assert c0 == 0 and np.array_equal(wr.bits(same), wr.bits(prior))
    empty, _ = wr.wproject([None, None], w, 3, 5, 9, 7)
    assert np.array_equal(wr.bits(empty), np.zeros((2, 7, 9), np.int32))    # +0.0 planes
