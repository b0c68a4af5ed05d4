"""The local correlation image from Codec.project_pairs and Codec.project.

For every pixel, the mean Pearson correlation of its time course with those of its 4 or 8 neighbours: the summary image
that cell detection draws candidates from.  project_pairs gives the sums of neighbour products Sab per forward offset,
project gives Sa, Saa and the frame count N, and

    r = (N Sab - Sa Sb) / sqrt((N Saa - Sa^2) (N Sbb - Sb^2))

follows per pair without a decoded frame ever being held.  Everything here is torch on the codec's device and nothing
synchronises.

Exactness.  The planes are exact integers.  local_correlation evaluates r in float64, which represents every integer
below 2^53 exactly: Sab, Saa <= N * (2^bits - 1)^2, so the inputs are exact for N < 2^53 / 255^2 = 1.3e11 frames of 8-bit
data and N < 2^53 / 65,535^2 = 2^21 = 2,097,152 frames of 16-bit data.  The products N * Sab and Sa * Sb are exact below
2^53 as well while N^2 * (2^bits - 1)^2 < 2^53: N < 372,000 frames (8 bit) or N < 1,448 frames (16 bit); beyond that each
is rounded once to 53 bits before the subtraction, a relative error of 2^-53 of terms whose difference may be much
smaller than they are (nearly constant pixels of long 16-bit recordings lose the most).
"""
import numpy as np
import torch

from . import max_frame_bytes, tiles, unpack_video_header


def _spans(dx, dy, rw, rh):
    """(first, partner) index tuples of a (rh, rw) plane for the offset (dx, dy), dy >= 0."""
    xa = slice(max(0, -dx), rw - max(0, dx))
    xb = slice(max(0, dx), rw - max(0, -dx))
    return (slice(0, rh - dy), xa), (slice(dy, rh), xb)


def local_correlation(pair_projection, projection):
    """float64 (rh, rw) device tensor: for every pixel the mean of r over the neighbours present in the window along
    pair_projection.offsets (both directions of each pair).  projection: Codec.project's result for the same frames and
    window, with sum, sumsq and count.  A pair with a zero-variance member (N Saa == Sa^2, an integer test) is left out
    of the mean; a pixel with no pair left, and every pixel when no frame was accepted, gives 0."""
    if projection.sum is None or projection.sumsq is None:
        raise ValueError("projection needs the statistics sum and sumsq")
    out = pair_projection.out
    rh, rw = out.shape[1:]
    if tuple(projection.sum.shape) != (rh, rw) or tuple(projection.sumsq.shape) != (rh, rw):
        raise ValueError("the projection and the pair projection cover different windows")
    N = projection.count.view(-1)[0].to(torch.float64)
    S = projection.sum.to(torch.float64)
    var = N * projection.sumsq.to(torch.float64) - S * S          # N^2 times the population variance, >= 0
    total = torch.zeros((rh, rw), dtype=torch.float64, device=out.device)
    number = torch.zeros((rh, rw), dtype=torch.float64, device=out.device)
    for j, (dx, dy) in enumerate(pair_projection.offsets):
        a, b = _spans(dx, dy, rw, rh)
        cov = N * out[j][a].to(torch.float64) - S[a] * S[b]
        ok = (var[a] > 0) & (var[b] > 0)
        r = torch.where(ok, cov / torch.sqrt(torch.where(ok, var[a] * var[b], torch.ones_like(cov))),
                        torch.zeros_like(cov))
        okf = ok.to(torch.float64)
        total[a] += r
        total[b] += r
        number[a] += okf
        number[b] += okf
    return torch.where(number > 0, total / number.clamp(min=1.0), torch.zeros_like(total))


def _calls(codec, bits):
    if bits not in (8, 16):
        raise ValueError("bits must be 8 or 16")
    return (codec.project, codec.project_pairs) if bits == 8 else (codec.project16, codec.project_pairs16)


def _pairs_of(neighbours):
    if neighbours not in (4, 8):
        raise ValueError("neighbours must be 4 or 8")
    return neighbours


def correlation_image(codec, stream, stream_offset, stream_bytes, offsets, W, H, n, x=0, y=0, rw=None, rh=None,
                      neighbours=8, bits=8):
    """The local correlation image of the rw x rh window at (x, y) over n frames, straight from the compressed stream:
    one project (sum, sumsq) and one project_pairs.  neighbours: 4 or 8.  bits: 8 for DBDE streams, 16 for DBDE16.
    Returns (image float64 (rh, rw), count int64 (1,), results (n, 4) int64)."""
    project, project_pairs = _calls(codec, bits)
    pr, results = project(stream, stream_offset, stream_bytes, offsets, W, H, n, x, y, rw, rh, stats=("sum", "sumsq"))
    pp, _ = project_pairs(stream, stream_offset, stream_bytes, offsets, W, H, n, _pairs_of(neighbours), x, y, rw, rh)
    return local_correlation(pp, pr), pr.count, results


def correlation_file(codec, path, neighbours=8, batch=64, window=None, bits=8):
    """correlation_image of a .dbde file that need not fit in device memory: the file is read once in pieces that hold
    `batch` frames (quantiles.count_file's reading loop), each piece is indexed on the device and folded into the same
    integer planes with accumulate=True, so only one batch of compressed bytes and the window-sized planes are
    resident; the planes are integers, so the image equals the one-call image bit for bit.  .dbde files hold 8-bit
    frames, so bits must be 8.  window: (x, y, rw, rh), by default the whole frame.  Returns (image, count, results)
    as correlation_image does, the results covering every frame of the file."""
    if bits != 8:
        raise ValueError("a .dbde file holds 8-bit frames: bits must be 8")
    pairs = _pairs_of(neighbours)
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
        pr = pp = None
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
            pr, res = codec.project(buf, 0, len(data), offs, W, H, m, x, y, rw, rh, stats=("sum", "sumsq"), out=pr,
                                    accumulate=pr is not None)
            pp, _ = codec.project_pairs(buf, 0, len(data), offs, W, H, m, pairs, x, y, rw, rh, out=pp,
                                        accumulate=pp is not None)
            all_results.append(res)
            if m < n:
                end = int(offs[m].item())
            else:
                last = int(offs[m - 1].item())
                n64 = int.from_bytes(data[last + 28 + 2 * T: last + 32 + 2 * T], "little")
                end = last + 32 + 2 * T + 8 * n64
            codec.sync()   # the piece's buffer is released below
            carry = data[end:]
    results = torch.cat(all_results) if all_results else torch.empty((0, 4), dtype=torch.int64, device=codec.device)
    if pp is None:   # no frame in the file
        return (torch.zeros((rh, rw), dtype=torch.float64, device=codec.device),
                torch.zeros(1, dtype=torch.int64, device=codec.device), results)
    return local_correlation(pp, pr), pr.count, results
