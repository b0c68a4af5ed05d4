"""Weights for Codec.project_weighted, and what to do with its planes.

Every builder returns a float32 tensor (R, n): row r holds regressor r's weight for frames first .. first + n - 1 of a
sequence of `total` frames (total defaults to first + n), so a batch can ask for its slice of a longer sequence and the
slices of consecutive batches are exactly the columns of the whole.  The values are computed in float64 and rounded to
float32 once.

pearson() turns the planes of a weighted projection and the sum / sum of squares of Codec.project into per-pixel
correlation maps; regress_file() streams a .dbde file through project_weighted batch by batch.
"""
import math

import numpy as np
import torch

from . import WeightedProjection, accepted_frames, max_frame_bytes, tiles, unpack_video_header


def _frames(n, first, total):
    n, first = int(n), int(first)
    total = first + n if total is None else int(total)
    if n < 0 or first < 0 or first + n > total:
        raise ValueError(f"frames [{first}, {first + n}) do not lie in a sequence of {total}")
    return range(first, first + n), total


def _rows(rows, device):
    """float64 values, one Python float per element (so that a frame's weight never depends on the slice it is asked
    in), rounded to float32 once."""
    return torch.tensor(rows, dtype=torch.float64).reshape(len(rows), -1).to(torch.float32).to(device)


def fourier(n, period, harmonics=1, first=0, total=None, device=None):
    """cos and sin rows at the frequencies h / period (in cycles per frame), h = 1 .. harmonics: rows 2(h-1) and
    2(h-1) + 1 are cos(2 pi h f / period) and sin(2 pi h f / period).  Plane pair (c, s) of the projection gives the
    amplitude hypot(c, s) * 2 / count and the phase atan2(-s, c) of the component."""
    frames, _ = _frames(n, first, total)
    if not period > 0 or int(harmonics) < 1:
        raise ValueError("period must be positive and harmonics at least 1")
    rows = []
    for h in range(1, int(harmonics) + 1):
        k = 2.0 * math.pi * h / float(period)
        rows += [[math.cos(k * f) for f in frames], [math.sin(k * f) for f in frames]]
    return _rows(rows, device)


def trend(n, first=0, total=None, device=None):
    """One row: the linear trend over the whole sequence, centred and of unit norm, t_f = (f - (total - 1) / 2) / |.|.
    The projection's plane is then the per-pixel slope times the norm (a constant pixel gives 0)."""
    frames, total = _frames(n, first, total)
    c = (total - 1) / 2.0
    norm = math.sqrt(total * (total * total - 1) / 12.0) if total > 1 else 1.0   # sqrt(sum (k - c)^2)
    return _rows([[(f - c) / norm for f in frames]], device)


def ema(n, alpha, first=0, total=None, device=None):
    """One row: the weights alpha * (1 - alpha)^(total - 1 - f) of an exponentially weighted background that ends at the
    sequence's last frame."""
    frames, total = _frames(n, first, total)
    if not 0.0 < alpha <= 1.0:
        raise ValueError("alpha must lie in (0, 1]")
    return _rows([[float(alpha) * (1.0 - float(alpha)) ** (total - 1 - f) for f in frames]], device)


def pearson(weighted, projection, weights, results):
    """Pearson correlation of every regressor with every pixel over the accepted frames: float64 (R, rh, rw) on the
    planes' device, NaN where a variance is 0 (or no frame was accepted).  weighted: the WeightedProjection of `weights`;
    projection: a Projection of the same frames and window with sum and sumsq (Codec.project); results: the (n, 4)
    tensor either call returned.  A float64 host formula on the device tensors, not a kernel:
        r = (Swx - Sw Sx / N) / sqrt((Sww - Sw^2 / N) (Sxx - Sx^2 / N))."""
    w = weights if weights.dim() == 2 else weights.view(1, -1)
    n = results.shape[0]
    dev = weighted.out.device
    ok = accepted_frames(results).to(dev).view(1, -1)
    w64 = w[:, :n].to(dev).to(torch.float64)
    w64 = torch.where(ok, w64, torch.zeros_like(w64))
    N = projection.count.to(torch.float64).view(1, 1, 1)
    Sw = w64.sum(1).view(-1, 1, 1)
    Sww = (w64 * w64).sum(1).view(-1, 1, 1)
    Sx = projection.sum.to(torch.float64).unsqueeze(0)
    Sxx = projection.sumsq.to(torch.float64).unsqueeze(0)
    cov = weighted.out.to(torch.float64) - Sw * Sx / N
    var_w = Sww - Sw * Sw / N
    var_x = Sxx - Sx * Sx / N
    den = var_w * var_x
    nan = torch.full_like(cov, float("nan"))
    return torch.where(den > 0.0, cov / den.clamp(min=0.0).sqrt(), nan)


def regress_file(codec, path, weights, batch=64, window=None):
    """Streams the 8-bit .dbde file `path` through Codec.project_weighted, `batch` frames at a time: the file is read in
    pieces that hold a batch, each piece is indexed on the device, and batch k covering frames [a, b) calls
    project_weighted(..., weights[:, a:b], accumulate=True) on planes that start at +0.0, so the value is the defined
    chain with those batch boundaries (include/dbde_hip.h) and only one batch of compressed bytes is resident.  weights:
    float32 device tensor (R, >= frames in the file).  window: (x, y, rw, rh), by default the whole frame.  Returns
    (WeightedProjection, results (frames, 4) int64)."""
    batch = int(batch)
    if batch < 1:
        raise ValueError("batch must be at least 1")
    if weights.dim() == 1:
        weights = weights.view(1, -1)
    all_results = []
    with open(path, "rb") as src:
        _, (_, H, W, _) = unpack_video_header(np.frombuffer(src.read(28), np.uint8))
        W, H = int(W), int(H)
        x, y, rw, rh = (0, 0, W, H) if window is None else window
        T = tiles(W, H)
        piece = batch * max_frame_bytes(W, H)          # always holds `batch` whole frames, unless the file ends
        out = WeightedProjection.empty(weights.shape[0], rh, rw, codec.device)
        out.out.zero_()
        carry, a = b"", 0
        while True:
            data = carry + src.read(max(piece - len(carry), 0))
            if len(data) < 32 + 2 * T:
                break   # the end, or a cut frame behind the last whole one
            buf = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(codec.device)
            offs, n = codec.index_stream(buf, 0, len(data), W, H, batch + 1)
            m = min(n, batch)
            if m == 0:
                break
            if a + m > weights.shape[1]:
                raise ValueError(f"the file holds more than the {weights.shape[1]} frames the weights have columns for")
            _, res = codec.project_weighted(buf, 0, len(data), offs, W, H, m, weights[:, a:a + m], x, y, rw, rh,
                                            out=out, accumulate=True)
            all_results.append(res)
            if m < n:
                end = int(offs[m].item())
            else:
                last = int(offs[m - 1].item())
                n64 = int.from_bytes(data[last + 28 + 2 * T: last + 32 + 2 * T], "little")
                end = last + 32 + 2 * T + 8 * n64
            codec.sync()   # the piece's buffer is released below
            carry, a = data[end:], a + m
    results = torch.cat(all_results) if all_results else torch.empty((0, 4), dtype=torch.int64, device=codec.device)
    return out, results
