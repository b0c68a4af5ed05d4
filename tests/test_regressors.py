"""CPU: the weight builders of dbde_video_cpp_amd.regressors -- their values, and that a batch's slice (first=, total=) is
exactly the columns of the whole sequence.  No GPU."""
import math
import os
import sys
from importlib import import_module

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.fixture(scope="module")
def reg():
    import dbde_video_cpp_amd   # noqa: F401
    return import_module("dbde_video_cpp_amd.regressors")


def test_fourier_values(reg):
    import torch
    n, period = 50, 12.5
    w = reg.fourier(n, period, harmonics=2)
    assert w.dtype == torch.float32 and tuple(w.shape) == (4, n)
    f = np.arange(n, dtype=np.float64)
    for h in (1, 2):
        a = 2 * math.pi * h * f / period
        assert np.allclose(w[2 * h - 2].numpy(), np.cos(a), rtol=0, atol=1.2e-7)
        assert np.allclose(w[2 * h - 1].numpy(), np.sin(a), rtol=0, atol=1.2e-7)
    assert w[0, 0] == 1.0 and w[1, 0] == 0.0
    # a pure tone at the period projects onto its own pair and not onto the second harmonic (whole periods)
    tone = np.cos(2 * math.pi * np.arange(100) / 25.0 + 0.3)
    c = reg.fourier(100, 25.0, 2).numpy().astype(np.float64) @ tone
    assert abs(math.hypot(c[0], c[1]) * 2 / 100 - 1.0) < 1e-6 and abs(math.atan2(-c[1], c[0]) - 0.3) < 1e-6
    assert abs(c[2]) < 1e-4 and abs(c[3]) < 1e-4


def test_trend_is_centred_and_of_unit_norm(reg):
    for n in (2, 7, 100):
        t = reg.trend(n).numpy().astype(np.float64)
        assert t.shape == (1, n)
        assert abs(t.sum()) < 1e-5 and abs((t * t).sum() - 1.0) < 1e-5
        assert (np.diff(t[0]) > 0).all()
        line = 3.0 + 0.25 * np.arange(n)
        assert abs((t[0] * line).sum() - 0.25 * math.sqrt(((np.arange(n) - (n - 1) / 2) ** 2).sum())) < 1e-4
    assert reg.trend(1).numpy().tolist() == [[0.0]]


def test_ema_values(reg):
    n, alpha = 40, 0.125
    w = reg.ema(n, alpha).numpy()
    want = alpha * (1 - alpha) ** (n - 1 - np.arange(n, dtype=np.float64))
    assert np.allclose(w[0], want, rtol=1.2e-7, atol=0)
    assert w[0, -1] == np.float32(alpha) and abs(w.astype(np.float64).sum() - (1 - (1 - alpha) ** n)) < 1e-6
    assert reg.ema(3, 1.0).numpy().tolist() == [[0.0, 0.0, 1.0]]


def test_slices_are_the_columns_of_the_whole(reg):
    import torch
    total = 37
    makers = (lambda **k: reg.fourier(period=9.3, harmonics=3, **k), lambda **k: reg.trend(**k),
              lambda **k: reg.ema(alpha=0.07, **k))
    for make in makers:
        whole = make(n=total)
        for first, n in ((0, 37), (0, 10), (10, 13), (23, 14), (36, 1), (5, 0)):
            part = make(n=n, first=first, total=total)
            assert torch.equal(part, whole[:, first:first + n]), (first, n)
    # without total= a slice of trend / ema describes a shorter sequence: total matters and is checked
    assert not torch.equal(reg.trend(10), reg.trend(10, first=0, total=37))
    for bad in (dict(n=5, first=35, total=37), dict(n=-1), dict(n=3, first=-1)):
        with pytest.raises(ValueError):
            reg.trend(**bad)
    with pytest.raises(ValueError):
        reg.ema(5, 0.0)
    with pytest.raises(ValueError):
        reg.fourier(5, 0.0)
