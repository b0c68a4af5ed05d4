"""The cases of the lag projections' GPU tests as data (test infrastructure; not a test module), so that
tests/test_lag_ref.py can hold the cap on the reference of every one of them, with the same seeds, before any GPU run,
and tests/test_gpu_lag.py / test_gpu_lag16.py run the same lists at their pixel size.

A case is (stream, n, lag, window, lead, mask, cap): `stream` the arguments of lag_gpu.stream, n the leading frames of
it the call takes, cap whether lag_gpu.cap is asserted on its reference (it applies from 3 counted pairs on)."""
import lag_gpu as lg

FPS33 = 17   # frames per segment of n = 33 on a device of 256 compute units: 2 segments of 17 (tests/test_lag_plan.py)


def noise(bits, n, W=lg.FRAME[0], H=lg.FRAME[1], bad=()):
    return ("noise", lg.seed_of(W, H, bits) + 1, W, H, n, bits, tuple(bad))


def crafted(bits, n, W=lg.FRAME[0], H=lg.FRAME[1], bad=()):
    return ("crafted", lg.seed_of(W, H, bits) + 2, W, H, n, bits, tuple(bad))


def counts_of(lag):
    """1, lag, lag + 1, lag + 2 (no pair, no pair, one, two) and 11 and 13 (around the pipeline's group of 4)."""
    return sorted({1, lag, lag + 1, lag + 2, 11, 13})


def sweep(bits, lag):
    """Every window of the 200 x 123 frame at every frame count, all five statistics."""
    return [(noise(bits, 13), n, lag, win, 0, 31, True) for n in counts_of(lag) for win in lg.WINDOWS]


def wide(bits):
    """300 x 20: two pieces at 8 bits (three at 16); the full frame and windows across the pieces' seams."""
    W, H = lg.WIDE
    return [(noise(bits, 13, W, H), 13, lag, win, 0, 31, True)
            for lag in (1, 4, 8) for win in [(0, 0, W, H), (250, 3, 20, 15), (120, 0, 20, 20)]]


def segments(bits):
    """n = 33 and n = 70 on the small windows: 2 and 3 segments on a 256-CU part, each after the first with lag history
    frames of its own."""
    return [(noise(bits, 70), n, lag, win, 0, mask, True)
            for n in (33, 70) for lag in (1, 3, 8) for win in (lg.SMALL, lg.WINDOWS[3]) for mask in (31, 3, 28)]


def bad_sets(lag, n=13):
    """Rejected frames that each hit a different branch: frame 0, frame lag, the last frame, two frames exactly lag
    apart, two adjacent frames, all frames."""
    return [(0,), (lag,), (n - 1,), (2, 2 + lag), (4, 5), tuple(range(n))]


def rejected(bits, lag):
    out = [(crafted(bits, 13, bad=bad), 13, lag, win, 0, 31, True)
           for bad in bad_sets(lag) for win in (lg.WINDOWS[0], lg.SMALL)]
    # the last frame of segment 0 and the first frame of segment 1
    out += [(crafted(bits, 33, bad=(FPS33 - 1, FPS33)), 33, lag, win, 0, 31, True) for win in (lg.WINDOWS[0], lg.SMALL)]
    return out


def leads(bits):
    """lead in {0, 1, lag, lag + 3, n}, with a rejected frame inside the history frames (frame 1)."""
    return [(crafted(bits, 13, bad=(1,)), 13, lag, win, lead, 31, True)
            for lag in (2, 5) for lead in (0, 1, lag, lag + 3, 13) for win in (lg.WINDOWS[0], lg.SMALL)]


def masks(bits):
    return [(noise(bits, 13), 13, 3, lg.SMALL, 0, mask, True) for mask in lg.MASKS]


def extremes(bits):
    """Frames of constant 0 and constant 255 / 65,535 alternating: the extreme products (even lags: a = b, so half the
    pairs hold the largest product) and differences (odd lags: every pair holds the largest difference).  No cap: either
    the products or the differences are all zero by construction."""
    return [(("alternating", 0, 72, 40, n, bits, ()), n, lag, (0, 0, 72, 40), 0, 31, False)
            for n in (13, 70) for lag in (1, 2, 7, 8)]


SPLIT_BAD = (0, 6, 7, 31, 32, 40, 69)


def splits(bits, lag):
    """The one call of the split-rule test: 70 noise frames (crafted ones saturate maxdiff at every lag by then), 7 of
    them rejected, at two windows."""
    return [(noise(bits, 70, bad=SPLIT_BAD), 70, lag, win, 0, 31, True) for win in (lg.SMALL, lg.WINDOWS[0])]


def every(bits):
    out = []
    for lag in lg.LAGS:
        out += sweep(bits, lag)
    for lag in (1, 3, 8):
        out += rejected(bits, lag)
    for lag in (1, 3, 7, 8):
        out += splits(bits, lag)
    return out + wide(bits) + segments(bits) + leads(bits) + masks(bits) + extremes(bits)


def run(codec, cases, bits, what=""):
    """Every case through lag_gpu.check; the results rows are project's for the same frames."""
    import torch
    rows = {}
    for spec, n, lag, win, lead, mask, cap in cases:
        s = lg.stream(*spec).first(n)
        out, res = lg.check(codec, s, lag, win, mask, lead, bits, what=f"{what} {spec[0]} bad={spec[6]}", use_cap=cap)
        if (spec, n) not in rows:
            project = codec.project if bits == 8 else codec.project16
            rows[(spec, n)] = project(s.buf, s.lead, s.total, s.offs, s.W, s.H, n, stats=("sum",))[1]
            codec.sync()
        assert torch.equal(res, rows[(spec, n)]), (what, spec, n, "results rows")
