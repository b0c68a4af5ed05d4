"""Per-pixel noise, motion and autocorrelation images from Codec.project_lag and Codec.project.

project_lag folds, per pixel, the pairs (a, b) = (p[f - lag], p[f]) of frames `lag` apart into exact integer planes:
product = sum a b, pairsum = sum (a + b), absdiff = sum |b - a|, sqdiff = sum (b - a)^2, maxdiff = max |b - a|, with
pairs = the number P of counted pairs.  From them, without a decoded frame ever being held:

    noise_image          sqrt(sqdiff / (2 P)): the noise level from successive differences, which a slow signal does
                         not inflate (the standard deviation does)
    mean_abs_difference  absdiff / P: a motion / activity map
    autocorrelation      with project's sum S, sumsq Q and count N of the same frames,
                         r = (N^2 Sab - N S Spair + P S^2) / (P (N Q - S^2)):
                         the mean over the pairs of (a - mu)(b - mu), mu = S / N, over the population variance
    peak_to_noise        (peak - baseline) / noise: the factor the local correlation image is multiplied by to seed
                         cell detection

Everything here is torch on the codec's device with float64 arithmetic from the exact integers, and nothing
synchronises.

Exactness.  float64 represents every integer below 2^53 exactly.  sqdiff, product <= P (2^bits - 1)^2 and pairsum
<= 2 P (2^bits - 1), so the planes convert exactly for P < 2^53 / 255^2 = 1.3e11 pairs of 8-bit data and
P < 2^53 / 65,535^2 = 2^21 = 2,097,152 pairs of 16-bit data; noise_image and mean_abs_difference then round twice (the
division and the root).  In autocorrelation the three terms of the numerator are each at most N^2 P (2^bits - 1)^2 and
are exact below 2^53 while N^3 (2^bits - 1)^2 < 2^53: N < 5,170 frames (8 bit) or N < 128 frames (16 bit); beyond that
each is rounded once to 53 bits before they are combined, a relative error of 2^-53 of terms whose combination may be
much smaller than they are (nearly constant pixels of long 16-bit recordings lose the most).  The zero-variance test
N Q == S^2 is made on the int64 planes where N Q < 2^63 and is then exact.
"""
import numpy as np
import torch

from . import max_frame_bytes, tiles, unpack_video_header


def _pairs(lp):
    return lp.pairs.view(-1)[0].to(torch.float64)


def _need(lp, name):
    t = getattr(lp, name)
    if t is None:
        raise ValueError(f"the lag projection needs the statistic {name}")
    return t.to(torch.float64)


def _zero(like):
    return torch.zeros((), dtype=torch.float64, device=like.device)


def noise_image(lp):
    """float64 (rh, rw): sqrt(sqdiff / (2 pairs)), the per-pixel noise level from the differences of frames lp.lag
    apart; 0 everywhere when no pair was counted."""
    P = _pairs(lp)
    return torch.where(P > 0, torch.sqrt(_need(lp, "sqdiff") / (2.0 * P.clamp(min=1.0))), _zero(P))


def mean_abs_difference(lp):
    """float64 (rh, rw): absdiff / pairs, the mean |p[f] - p[f - lag]| per pixel; 0 when no pair was counted."""
    P = _pairs(lp)
    return torch.where(P > 0, _need(lp, "absdiff") / P.clamp(min=1.0), _zero(P))


def autocorrelation(lp, projection):
    """float64 (rh, rw): the autocorrelation at lp.lag, r = (N^2 Sab - N S Spair + P S^2) / (P (N Q - S^2)), from the
    lag projection's product and pairsum and Codec.project's sum, sumsq and count over the same frames and window.  It
    is the mean over the counted pairs of (a - mu)(b - mu) divided by the population variance over the accepted frames.
    0 where the variance is 0 (N Q == S^2, an integer test) and everywhere when no pair was counted."""
    if projection.sum is None or projection.sumsq is None:
        raise ValueError("projection needs the statistics sum and sumsq")
    Sab, Spair = _need(lp, "product"), _need(lp, "pairsum")
    if tuple(projection.sum.shape) != tuple(lp.product.shape):
        raise ValueError("the projection and the lag projection cover different windows")
    Ni = projection.count.view(-1)[0]
    flat = Ni * projection.sumsq == projection.sum * projection.sum          # int64: exact while N Q < 2^63
    N, P = Ni.to(torch.float64), _pairs(lp)
    S, Q = projection.sum.to(torch.float64), projection.sumsq.to(torch.float64)
    num = N * N * Sab - N * S * Spair + P * S * S
    ok = ~flat & (P > 0)
    den = torch.where(ok, P * (N * Q - S * S), torch.ones_like(num))
    return torch.where(ok, num / den, torch.zeros_like(num))


def peak_to_noise(peak, baseline, lp):
    """float64 (rh, rw): (peak - baseline) / noise_image(lp), 0 where the noise is 0.  peak and baseline: tensors of the
    window's shape (or scalars), e.g. project's max and quantiles.temporal_median."""
    noise = noise_image(lp)
    diff = (torch.as_tensor(peak, device=noise.device).to(torch.float64)
            - torch.as_tensor(baseline, device=noise.device).to(torch.float64))
    return torch.where(noise > 0, diff / torch.where(noise > 0, noise, torch.ones_like(noise)), torch.zeros_like(noise))


def _call(codec, bits):
    if bits not in (8, 16):
        raise ValueError("bits must be 8 or 16")
    return codec.project_lag if bits == 8 else codec.project_lag16


def lag_image(codec, stream, stream_offset, stream_bytes, offsets, W, H, n, lag=1, stats=("sqdiff",), x=0, y=0, rw=None,
              rh=None, bits=8):
    """One project_lag over n frames of the stream: the one-call driver.  bits: 8 for DBDE streams, 16 for DBDE16.
    Returns (LagProjection, results (n, 4) int64)."""
    return _call(codec, bits)(stream, stream_offset, stream_bytes, offsets, W, H, n, lag, stats, 0, x, y, rw, rh)


def lag_file(codec, path, lag=1, stats=("sqdiff",), batch=64, window=None):
    """lag_image of a .dbde file that need not fit in device memory: the file is read once in pieces that hold `batch`
    new frames (correlation.correlation_file's reading loop); the bytes of the last `lag` frames of each piece stay in
    the carry and lead the next piece as history (lead = lag), and every piece is folded into the same integer planes
    with accumulate=True -- the header's split rule, so the planes equal the one-call planes bit for bit.  batch must
    be at least lag.  window: (x, y, rw, rh), by default the whole frame.  Returns (LagProjection, results), the results
    covering every frame of the file once."""
    batch, lag = int(batch), int(lag)
    if batch < max(lag, 1):
        raise ValueError("batch must be at least lag (and at least 1)")
    all_results = []
    with open(path, "rb") as src:
        _, (_, H, W, _) = unpack_video_header(np.frombuffer(src.read(28), np.uint8))
        W, H = int(W), int(H)
        x, y, rw, rh = (0, 0, W, H) if window is None else window
        T = tiles(W, H)
        piece = (batch + lag) * max_frame_bytes(W, H)   # holds the history and `batch` whole frames, unless the file ends
        lp = None
        carry, lead = b"", 0
        while True:
            data = carry + src.read(max(piece - len(carry), 0))
            if len(data) < 32 + 2 * T:
                break   # the end, or a cut frame behind the last whole one
            buf = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(codec.device)
            offs, n = codec.index_stream(buf, 0, len(data), W, H, lead + batch + 1)
            m = min(n, lead + batch)
            if m <= lead:
                break   # nothing behind the history frames
            lp, res = codec.project_lag(buf, 0, len(data), offs, W, H, m, lag, stats, lead, x, y, rw, rh, out=lp,
                                        accumulate=lp is not None)
            all_results.append(res[lead:])
            keep = min(lag, m)                              # the history of the next piece: this one's last frames
            start = int(offs[m - keep].item())
            codec.sync()   # the piece's buffer is released below
            carry, lead = data[start:], keep
    results = torch.cat(all_results) if all_results else torch.empty((0, 4), dtype=torch.int64, device=codec.device)
    if lp is None:   # no frame in the file
        from . import LagProjection
        lp = LagProjection.empty(stats, rh, rw, codec.device, lag=lag)
        for k in lp.stats:
            getattr(lp, k).zero_()
    return lp, results
