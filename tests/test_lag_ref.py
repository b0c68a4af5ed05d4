"""CPU: the lag projections' reference (tests/lag_ref.py) against a second formulation, the header's split rule on the
reference, and the cap (tests/lag_gpu.cap) on every stream the GPU tests use, with the same seeds -- so the content is
judged on the reference alone, before any GPU run."""
import numpy as np
import pytest

import lag_cases as lc
import lag_gpu as lg
import lag_ref as lr


@pytest.mark.parametrize("bits", (8, 16))
def test_two_formulations_agree(bits):
    """The loop from the definition against stacks with sqdiff = sum a^2 + sum b^2 - 2 sum a b in Python integers."""
    for spec in (lc.noise(bits, 13), lc.crafted(bits, 13, bad=(2, 7)), ("alternating", 0, 72, 40, 13, bits, ())):
        images = lg.host_images(*spec)
        W, H = spec[2], spec[3]
        for lag in lg.LAGS:
            for lead in (0, 3, 13):
                for win in ((0, 0, W, H), (3, 5, 41, 27)):
                    a = lr.lag(images, lag, *win, lead=lead, bits=bits)
                    b = lr.lag_expanded(images, lag, *win, lead=lead, bits=bits)
                    for k in lr.STATS:
                        assert np.array_equal(a[k].astype(object), b[k]), (spec[0], lag, lead, win, k)
                    assert a["pairs"] == b["pairs"] == len(lr.counted(images, lag, lead))
    # the extremes, by hand: 13 alternating frames, lag 1: 12 pairs of (0, max) or (max, 0); lag 2: 11 pairs, 5 of (max, max)
    top = (1 << bits) - 1
    images = lg.host_images("alternating", 0, 72, 40, 13, bits)
    one, two = lr.lag(images, 1, 0, 0, 72, 40, bits=bits), lr.lag(images, 2, 0, 0, 72, 40, bits=bits)
    assert (one["product"] == 0).all() and (one["sqdiff"] == 12 * top * top).all() and (one["maxdiff"] == top).all()
    assert (one["pairsum"] == 12 * top).all() and (one["absdiff"] == 12 * top).all()
    assert (two["product"] == 5 * top * top).all() and (two["pairsum"] == 10 * top).all() and not two["sqdiff"].any()


def test_counted_pairs():
    """A rejected frame is not skipped over: it voids the up to two pairs it is a member of."""
    im = [0, 0, None, 0, 0, 0, None, None, 0, 0]
    assert lr.counted(im, 1) == [1, 4, 5, 9] and lr.counted(im, 2) == [3, 5]
    assert lr.counted(im, 3) == [3, 4, 8] and lr.counted(im, 3, lead=4) == [4, 8] and lr.counted(im, 1, lead=10) == []
    assert lr.counted(im[:3], 3) == [] and lr.counted(im, 8) == [8, 9]


@pytest.mark.parametrize("bits", (8, 16))
@pytest.mark.parametrize("lag", lg.LAGS)
def test_split_rule_on_the_reference(bits, lag):
    """Frames [0, N) in one call equal the calls on [0, B) with lead 0 and on [kB - lag, (k + 1)B) with lead = lag,
    accumulated: every plane, pairs, and count = the accepted frames of [0, N)."""
    images = lg.host_images(*lc.splits(bits, lag)[0][0])
    win = lg.SMALL
    one = lr.lag(images, lag, *win, bits=bits)
    assert one["pairs"] > 3 and one["count"] == 63
    for B in sorted({lag, lag + 1, 7, 32}):
        if B < lag:
            continue
        got = lr.lag_split(images, lag, *win, B, bits=bits)
        for k in lr.STATS + ("pairs", "count"):
            assert np.array_equal(got[k], one[k]), (lag, B, k)
    assert lr.split_calls(70, 3, 32) == [(0, 32, 0), (29, 35, 3), (61, 9, 3)]


@pytest.mark.parametrize("bits", (8, 16))
def test_the_cap_holds_on_every_gpu_case(bits):
    seen = 0
    for spec, n, lag, win, lead, mask, cap in lc.every(bits):
        if cap:
            images = lg.host_images(*spec)[:n]
            try:
                want = lg.cap(images, lag, win, lead, bits)
            except AssertionError as e:
                raise AssertionError(f"{spec} n={n} lag={lag} {win} lead={lead}: {e}") from None
            seen += want["pairs"] >= 3
    assert seen >= 150     # n = 11 and 13 of the sweep alone are 64 cases of at least 3 pairs: the cap is no formality


def test_autocorrelation_two_pass_on_a_known_series():
    """A square wave of period 4 at one pixel: r(2) = -1 and r(4) = +1 up to the end effect of the finite series; a
    constant pixel gives 0."""
    n = 64
    images = [np.array([[10 + 5 * ((f // 2) % 2), 7]], np.uint8) for f in range(n)]
    r2 = lr.autocorrelation_two_pass(images, 2, 0, 0, 2, 1)
    r4 = lr.autocorrelation_two_pass(images, 4, 0, 0, 2, 1)
    assert abs(r2[0, 0] + 1) < 1e-12 and abs(r4[0, 0] - 1) < 1e-12 and r2[0, 1] == 0 and r4[0, 1] == 0
    assert not lr.autocorrelation_two_pass(images[:2], 2, 0, 0, 2, 1).any()
