"""CPU: quantiles.refine -- the radix refinement that turns per-pixel counts into an exact order statistic -- with a
numpy-backed count function, against np.sort.  No GPU, no library: torch on the CPU only."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = (6, 9)


def frames_of(bits, N, seed):
    """(N, 6, 9) samples: noise, a narrow band, and pixels constant at 0, at the maximum and at one value."""
    rng = np.random.default_rng(seed)
    top = (1 << bits) - 1
    f = rng.integers(0, top + 1, (N,) + SHAPE).astype(np.uint16 if bits == 16 else np.uint8)
    f[:, 0, 0] = 0
    f[:, 0, 1] = top
    f[:, 0, 2] = top // 3
    f[:, 1, :] = (top // 2 + rng.integers(-2, 3, (N, SHAPE[1]))).astype(f.dtype)     # many ties
    f[:, 2, 0] = np.where(np.arange(N) % 2 == 0, 0, top)                             # only the two extremes
    return f


class NumpyCounts:
    """count_fn over numpy samples; records every call's threshold shape."""

    def __init__(self, frames):
        self.frames, self.calls = frames.astype(np.int64), []

    def __call__(self, thr):
        assert thr.dtype == torch.int64
        self.calls.append(tuple(thr.shape))
        t = thr.numpy()
        assert t.min() >= 0
        t = t.reshape(t.shape[0], 1, 1) if t.ndim == 1 else t
        return torch.from_numpy((self.frames[None] <= t[:, None]).sum(1))


@pytest.mark.parametrize("bits", (8, 16))
@pytest.mark.parametrize("N", (1, 2, 13, 70))
@pytest.mark.parametrize("q", (0, 0.08, 0.5, 1))
def test_refine_is_the_order_statistic(bits, N, q):
    from dbde_video_cpp_amd import quantiles as qt
    frames = frames_of(bits, N, 100 * bits + N)
    r = int(np.floor(q * (N - 1)))
    want = np.sort(frames, 0)[r].astype(np.int64)
    for rank in (r, torch.tensor(r)):
        fn = NumpyCounts(frames)
        got = qt.refine(fn, rank, bits, SHAPE, "cpu")
        assert got.dtype == torch.int64 and tuple(got.shape) == SHAPE
        assert np.array_equal(got.numpy(), want), (bits, N, q)
        # 3 passes for 8 bits, 6 for 16; the first in scalars, the rest in maps; at most 7 levels each
        assert len(fn.calls) == qt.passes(bits) == {8: 3, 16: 6}[bits]
        assert len(fn.calls[0]) == 1 and all(len(c) == 3 and c[1:] == SHAPE for c in fn.calls[1:])
        assert all(c[0] <= 7 for c in fn.calls)
        assert [c[0] for c in fn.calls] == ([7, 7, 3] if bits == 8 else [7, 7, 7, 7, 7, 1])


@pytest.mark.parametrize("bits", (8, 16))
def test_thresholds_stay_in_the_pixel_range(bits):
    from dbde_video_cpp_amd import quantiles as qt
    frames = frames_of(bits, 5, 7)
    top = (1 << bits) - 1
    seen = []

    def fn(thr):
        seen.append((int(thr.min()), int(thr.max())))
        return NumpyCounts(frames)(thr)

    qt.refine(fn, 4, bits, SHAPE, "cpu")
    assert all(0 <= lo and hi <= top for lo, hi in seen)
    assert tuple(qt.first_thresholds(bits, "cpu").tolist()) == tuple((j + 1) * ((top + 1) >> 3) - 1 for j in range(7))


def test_per_pixel_ranks():
    from dbde_video_cpp_amd import quantiles as qt
    frames = frames_of(8, 13, 3)
    ranks = np.random.default_rng(5).integers(0, 13, SHAPE)
    want = np.take_along_axis(np.sort(frames, 0), ranks[None], 0)[0]
    got = qt.refine(NumpyCounts(frames), torch.from_numpy(ranks), 8, SHAPE, "cpu")
    assert np.array_equal(got.numpy(), want)
