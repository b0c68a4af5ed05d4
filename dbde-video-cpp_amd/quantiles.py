"""Exact per-pixel temporal order statistics from Codec.project_counts.

project_counts gives, per pixel, how many accepted frames lie at or below each of up to 8 thresholds.  refine() turns
that into an exact order statistic by radix refinement: every pass cuts each pixel's interval of candidate values into
8 (3 bits; the last pass of an 8-bit search into 4), so an 8-bit statistic takes 3 passes over the compressed bytes and a
16-bit one 6, and no decoded frame is ever held.  Everything here is torch on the codec's device: the thresholds of a
pass are computed from the counts of the pass before without leaving the device, and nothing synchronises.

temporal_quantile() / temporal_median() run the passes on a stream in device memory; quantile_file() streams a .dbde file
once per pass, batch by batch.  The value is the order statistic sorted[r] of the accepted frames of each pixel with
r = floor(q * (N - 1)): numpy's quantile(..., method="lower").
"""
import numpy as np
import torch

from . import CountProjection, max_frame_bytes, tiles, unpack_video_header

PASS_BITS = 3   # bits settled per pass: 2^3 - 1 = 7 thresholds, one launch of at most 8 levels


def passes(bits):
    """Passes over the data that refine() makes for `bits`-wide values: 3 for 8 bits, 6 for 16."""
    return (int(bits) + PASS_BITS - 1) // PASS_BITS


def first_thresholds(bits, device):
    """The first pass's thresholds, int64 (7,) (fewer where bits < 3): they do not depend on the data."""
    b = min(PASS_BITS, int(bits))
    step = (1 << int(bits)) >> b
    return (torch.arange((1 << b) - 1, dtype=torch.int64, device=device) + 1) * step - 1


def refine(count_fn, rank, bits, shape, device):
    """The value v of rank `rank` (0-based, ascending) per pixel, from counts alone: the smallest v with
    count(<= v) >= rank + 1.  int64 tensor of `shape`.

    count_fn(thr) -> integer tensor (K, *shape): per pixel, how many samples are <= each threshold.  thr is int64, (K,)
    on the first pass (the same thresholds for every pixel: first_thresholds) and (K, *shape) afterwards.  rank: an int
    or a device tensor broadcastable to `shape`.  State is a per-pixel `lo`, from 0, and an interval width, from
    2^bits; per pass b = min(3, bits left), step = width >> b, thresholds lo + (j + 1) * step - 1 for j < 2^b - 1,
    s = the number of levels whose count is < rank + 1, lo += s * step.  A pixel with fewer than rank + 1 samples ends
    at the largest value."""
    shape = tuple(shape)
    lo = torch.zeros(shape, dtype=torch.int64, device=device)
    need = (rank if torch.is_tensor(rank) else torch.tensor(int(rank), device=device)).to(torch.int64) + 1
    width, left = 1 << int(bits), int(bits)
    while left > 0:
        b = min(PASS_BITS, left)
        step = width >> b
        offs = (torch.arange((1 << b) - 1, dtype=torch.int64, device=device) + 1) * step - 1
        thr = offs if left == int(bits) else lo.unsqueeze(0) + offs.view((-1,) + (1,) * len(shape))
        c = count_fn(thr)
        s = (c.to(torch.int64) < need).sum(0)
        lo = lo + s * step
        width, left = step, left - b
    return lo


def _codec_dtype(thr, bits):
    """int64 thresholds -> what project_counts / project_counts16 take: uint8, or int16 holding the U16 bits."""
    if bits == 8:
        return thr.to(torch.uint8)
    return torch.where(thr >= 32768, thr - 65536, thr).to(torch.int16)


def _values(lo, count, bits):
    """refine()'s int64 values in the pixel dtype of the package, zero where no frame was accepted."""
    lo = torch.where(count.view(-1)[0] > 0, lo, torch.zeros_like(lo))
    return _codec_dtype(lo, bits)


def _rank(q, count):
    """floor(q * (N - 1)) on the device (numpy's method="lower"), 0 for N = 0."""
    q = float(q)
    if not 0.0 <= q <= 1.0:
        raise ValueError("q must lie in [0, 1]")
    return torch.floor(q * (count.view(-1)[0] - 1).to(torch.float64)).clamp(min=0).to(torch.int64)


def _quantiles(count_fn, q, bits, shape, device):
    """Shared by temporal_quantile and quantile_file.  count_fn(thr int64) -> (CountProjection, results); the first
    pass, whose thresholds do not depend on q, is run once and serves every q."""
    if bits not in (8, 16):
        raise ValueError("bits must be 8 or 16")
    qs = [q] if np.isscalar(q) else list(q)
    first, results = count_fn(first_thresholds(bits, device))

    def cached(thr):
        return first.out if thr.dim() == 1 else count_fn(thr)[0].out

    vals = [_values(refine(cached, _rank(qq, first.count), bits, shape, device), first.count, bits) for qq in qs]
    return (vals[0] if np.isscalar(q) else torch.stack(vals)), first.count, results


def temporal_quantile(codec, stream, stream_offset, stream_bytes, offsets, W, H, n, q, x=0, y=0, rw=None, rh=None,
                      bits=8):
    """The exact temporal quantile of every pixel of the rw x rh window at (x, y) over n frames, straight from the
    compressed stream: sorted[floor(q * (N - 1))] of the N accepted frames of each pixel (numpy's method="lower").
    bits: 8 for DBDE streams (3 passes of project_counts), 16 for DBDE16 streams (6 passes of project_counts16).  q: a
    float in [0, 1] or a sequence of them; several q share the first pass.  No frame accepted gives zeros and count 0.
    Returns (values, count int64 (1,), results (n, 4) int64): values uint8 (rh, rw), or int16 holding the U16 bits, with
    a leading axis over q when q is a sequence."""
    rw = W - x if rw is None else rw
    rh = H - y if rh is None else rh
    call = codec.project_counts if bits == 8 else codec.project_counts16

    def count_fn(thr):
        return call(stream, stream_offset, stream_bytes, offsets, W, H, n, _codec_dtype(thr, bits), x, y, rw, rh)

    return _quantiles(count_fn, q, bits, (rh, rw), codec.device)


def temporal_median(codec, stream, stream_offset, stream_bytes, offsets, W, H, n, x=0, y=0, rw=None, rh=None, bits=8):
    """temporal_quantile at q = 0.5: the lower median (sorted[(N - 1) // 2]) of every pixel, the background image that
    decode_mask's band_from_background expects."""
    return temporal_quantile(codec, stream, stream_offset, stream_bytes, offsets, W, H, n, 0.5, x, y, rw, rh, bits)


def count_file(codec, path, thresholds, batch=64, window=None):
    """Streams the 8-bit .dbde file `path` through Codec.project_counts, `batch` frames at a time, with regress_file's
    reading loop: the file is read in pieces that hold a batch, each piece is indexed on the device and counted into
    the same planes with accumulate=True, so only one batch of compressed bytes is resident.  thresholds: what
    project_counts takes (maps in the window's coordinates).  window: (x, y, rw, rh), by default the whole frame.
    Returns (CountProjection, results (frames, 4) int64)."""
    batch = int(batch)
    if batch < 1:
        raise ValueError("batch must be at least 1")
    all_results = []
    with open(path, "rb") as src:
        _, (_, H, W, _) = unpack_video_header(np.frombuffer(src.read(28), np.uint8))
        W, H = int(W), int(H)
        x, y, rw, rh = (0, 0, W, H) if window is None else window
        T = tiles(W, H)
        piece = batch * max_frame_bytes(W, H)          # always holds `batch` whole frames, unless the file ends
        out = None
        carry = b""
        while True:
            data = carry + src.read(max(piece - len(carry), 0))
            if len(data) < 32 + 2 * T:
                break   # the end, or a cut frame behind the last whole one
            buf = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(codec.device)
            offs, n = codec.index_stream(buf, 0, len(data), W, H, batch + 1)
            m = min(n, batch)
            if m == 0:
                break
            out, res = codec.project_counts(buf, 0, len(data), offs, W, H, m, thresholds, x, y, rw, rh, out=out,
                                            accumulate=out is not None)
            all_results.append(res)
            if m < n:
                end = int(offs[m].item())
            else:
                last = int(offs[m - 1].item())
                n64 = int.from_bytes(data[last + 28 + 2 * T: last + 32 + 2 * T], "little")
                end = last + 32 + 2 * T + 8 * n64
            codec.sync()   # the piece's buffer is released below
            carry = data[end:]
    if out is None:   # no frame in the file: zero planes, count 0
        K = thresholds.shape[0] if torch.is_tensor(thresholds) else np.atleast_1d(np.asarray(thresholds)).size
        out = CountProjection.empty(K, rh, rw, codec.device)
        out.out.zero_()
    results = torch.cat(all_results) if all_results else torch.empty((0, 4), dtype=torch.int64, device=codec.device)
    return out, results


def file_window(path, window=None):
    """(x, y, rw, rh) of `window` in the .dbde file `path`, by default its whole frame."""
    with open(path, "rb") as src:
        _, (_, H, W, _) = unpack_video_header(np.frombuffer(src.read(28), np.uint8))
    return (0, 0, int(W), int(H)) if window is None else tuple(window)


def quantile_file(codec, path, q, batch=64, window=None, bits=8):
    """temporal_quantile of a .dbde file that need not fit in device memory: one read of the file per pass (3 for 8
    bits), each pass accumulating the counts batch by batch (count_file), so only one batch of compressed bytes and the
    window-sized count planes are resident.  .dbde files hold 8-bit frames, so bits must be 8.  Returns (values, count,
    results) as temporal_quantile does, the results covering every frame of the file."""
    if bits != 8:
        raise ValueError("a .dbde file holds 8-bit frames: bits must be 8")
    x, y, rw, rh = file_window(path, window)

    def count_fn(thr):
        return count_file(codec, path, _codec_dtype(thr, bits), batch, (x, y, rw, rh))

    return _quantiles(count_fn, q, bits, (rh, rw), codec.device)
