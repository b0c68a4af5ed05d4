"""Registered summary images from Codec.project_registered: rigid integer shifts -> per-frame window
origins -> max / min / sum / sumsq images in the template's coordinates, straight from the compressed stream.

The shifts come from a registration tool's one integer (dx, dy) per frame, from tracking.follow's fiducial centres
(shifts_from_centres), or from estimate_shifts / estimate_file below: block matching of a few templates of a reference
image over a search radius (Codec.match_patches).  The convention is

    registered[Y][X] = frame_f[Y + dy_f][X + dx_f]

so (dx_f, dy_f) is where the template's pixel (0, 0) lies in frame f.  origins_from_shifts turns the shifts into the
window every frame can serve and its per-frame origins; registered_image and registered_file reduce over it.

Out of scope here: applying sub-pixel or piecewise-rigid shifts (estimate_shifts reports the per-patch field and
PatchMatch.refine the sub-pixel offsets, project_registered takes one integer origin per frame), FFT correlation of
whole frames, rotation and scale, and a fill mode for pixels that leave the frame (the common window holds only pixels
every frame has).
"""
import numpy as np
import torch

from . import max_frame_bytes, tiles, unpack_video_header


def _as_shifts(shifts, device=None):
    s = torch.as_tensor(shifts, device=device)
    if s.dim() != 2 or s.shape[1] != 2:
        raise ValueError("shifts must have shape (n, 2)")
    if s.dtype.is_floating_point or s.dtype == torch.bool or s.dtype.is_complex:
        raise ValueError("shifts must be integers (shifts_from_centres rounds centres)")
    return s.to(torch.int64)


def origins_from_shifts(shifts, W, H, max_shift=None, device=None):
    """Per-frame window origins for Codec.project_registered from (n, 2) integer (dx, dy) shifts.

    max_shift=None: the common window, in template coordinates X0 = max(0, -min dx), X1 = min(W, W - max dx), likewise
    in y; every origin (X0 + dx_f, Y0 + dy_f) lies inside the frame, so nothing is clamped.  One host synchronisation
    (the extrema).  max_shift=m: the window [m, W - m) x [m, H - m) without looking at the shifts; a frame that moved
    further is clamped by the kernel, which origins_used= of project_registered shows.
    Returns (origins int32 (n, 2) on the shifts' device (or `device`), rw, rh, (X0, Y0)); raises ValueError if the
    window is empty."""
    s = _as_shifts(shifts, device)
    if max_shift is None:
        if s.shape[0] == 0:
            X0 = Y0 = 0
            X1, Y1 = W, H
        else:
            lo, hi = s.amin(0).tolist(), s.amax(0).tolist()   # the host synchronisation
            X0, Y0 = max(0, -lo[0]), max(0, -lo[1])
            X1, Y1 = min(W, W - hi[0]), min(H, H - hi[1])
    else:
        m = int(max_shift)
        if m < 0:
            raise ValueError("max_shift must be >= 0")
        X0 = Y0 = m
        X1, Y1 = W - m, H - m
    rw, rh = X1 - X0, Y1 - Y0
    if rw < 1 or rh < 1:
        raise ValueError(f"the shifts leave no common window in a {W} x {H} frame ({rw} x {rh})")
    base = torch.empty(2, dtype=torch.int64, device=s.device)
    base[:1].fill_(X0)
    base[1:].fill_(Y0)
    origins = (s + base).clamp(-2 ** 31, 2 ** 31 - 1).to(torch.int32).contiguous()
    return origins, rw, rh, (X0, Y0)


def shifts_from_centres(centres, reference=None):
    """tracking.follow's centres (n, K, 2) -> integer shifts int64 (n, 2), on the centres' device: the mean over the K
    fiducials, less `reference` (an (x, y), by default frame 0's mean), rounded to nearest (halves up, as
    origins_from_centres rounds)."""
    c = torch.as_tensor(centres)
    if c.dim() != 3 or c.shape[2] != 2 or c.shape[1] < 1:
        raise ValueError("centres must have shape (n, K, 2) with K >= 1")
    mean = c.to(torch.float64).mean(1)
    if reference is None:
        if mean.shape[0] == 0:
            return torch.empty((0, 2), dtype=torch.int64, device=mean.device)
        ref = mean[:1]
    else:
        ref = torch.as_tensor(reference, dtype=torch.float64, device=mean.device).reshape(1, 2)
    return torch.floor(mean - ref + 0.5).to(torch.int64)


def _call(codec, bits):
    if bits not in (8, 16):
        raise ValueError("bits must be 8 or 16")
    return codec.project_registered if bits == 8 else codec.project_registered16


def registered_image(codec, stream, stream_offset, stream_bytes, offsets, W, H, n, shifts,
                     stats=("max", "min", "sum", "sumsq"), bits=8, max_shift=None, origins_used=None):
    """The registered projection of n frames in one call: origins_from_shifts(shifts[:n]) and project_registered.
    Returns (Projection of the rw x rh common window, (X0, Y0) its place in the template, results (n, 4))."""
    s = _as_shifts(shifts, codec.device)[:n]
    if s.shape[0] < n:
        raise ValueError(f"{n} frames need {n} shifts, not {s.shape[0]}")
    origins, rw, rh, at = origins_from_shifts(s, W, H, max_shift)
    pr, results = _call(codec, bits)(stream, stream_offset, stream_bytes, offsets, W, H, n, rw, rh, origins, stats=stats,
                                     origins_used=origins_used)
    return pr, at, results


def registered_file(codec, path, shifts, stats=("max", "min", "sum", "sumsq"), batch=64, bits=8, max_shift=None):
    """registered_image of a .dbde file that need not fit in device memory: the file is read once in pieces that hold
    `batch` frames (correlation.correlation_file's reading loop), each piece is indexed on the device and folded into
    the same planes with accumulate=True and its rows of the origins.  The planes are integers, so the result equals
    the one-call result bit for bit.  shifts: one row per frame of the file (the window is the common one of all rows; fewer rows than frames raise).
    .dbde files hold 8-bit frames, so bits must be 8.  Returns (Projection, (X0, Y0), results) as registered_image
    does, the results covering every frame of the file."""
    if bits != 8:
        raise ValueError("a .dbde file holds 8-bit frames: bits must be 8")
    batch = int(batch)
    if batch < 1:
        raise ValueError("batch must be at least 1")
    s = _as_shifts(shifts, codec.device)
    all_results = []
    done = 0
    with open(path, "rb") as src:
        _, (_, H, W, _) = unpack_video_header(np.frombuffer(src.read(28), np.uint8))
        W, H = int(W), int(H)
        origins, rw, rh, at = origins_from_shifts(s, W, H, max_shift)
        T = tiles(W, H)
        piece = batch * max_frame_bytes(W, H)          # always holds `batch` whole frames, unless the file ends
        pr = None
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
            if done + m > origins.shape[0]:
                raise ValueError(f"the file holds more than the {origins.shape[0]} frames the shifts cover")
            pr, res = codec.project_registered(buf, 0, len(data), offs, W, H, m, rw, rh, origins[done:done + m],
                                               stats=stats, out=pr, accumulate=pr is not None)
            done += m
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
    if pr is None:   # no frame in the file: the empty projection
        from . import Projection
        pr = Projection.empty(rh, rw, stats, codec.device)
        for plane, fill in ((pr.max, 0), (pr.min, 255), (pr.sum, 0), (pr.sumsq, 0)):
            if plane is not None:
                plane.fill_(fill)
    return pr, at, results


def _as_positions(positions, device=None):
    p = torch.as_tensor(positions, device=device)
    if p.dim() != 2 or p.shape[1] != 2 or p.shape[0] < 1:
        raise ValueError("positions must have shape (K, 2) with K >= 1")
    if p.dtype.is_floating_point or p.dtype == torch.bool or p.dtype.is_complex:
        raise ValueError("positions must be integers")
    return p.to(torch.int64)


def templates_from_image(image, positions, tw, th):
    """(K, th, tw) slices of a reference image (H, W) at the (x, y) `positions` (K, 2), on the image's device and in its
    type: a decoded frame, or project's rounded mean.  A slice must lie inside the image."""
    if not torch.is_tensor(image) or image.dim() != 2:
        raise ValueError("image must be a 2-D tensor")
    H, W = image.shape
    pos = _as_positions(positions).tolist()
    for x, y in pos:
        if not (0 <= x <= W - tw and 0 <= y <= H - th):
            raise ValueError(f"a {tw} x {th} template at ({x}, {y}) leaves the {W} x {H} image")
    return torch.stack([image[y:y + th, x:x + tw] for x, y in pos]).contiguous()


def search_origins(positions, S, n, device=None):
    """The search patches' origins for Codec.match_patches: positions (K, 2) - S, for each of n frames, int32 (n, K, 2)
    on the positions' device (or `device`)."""
    p = _as_positions(positions, device)
    return (p - int(S)).clamp(-2 ** 31, 2 ** 31 - 1).to(torch.int32)[None].expand(int(n), -1, -1).contiguous()


def _shifts_of(pm, results):
    """PatchMatch of a batch -> (shifts int32 (n, 2), score (n,), per-patch shifts int32 (n, K, 2))."""
    from . import accepted_frames, best_shift
    z = pm.zncc()
    ok = accepted_frames(results).to(torch.bool)
    z = torch.where(ok.view(-1, 1, 1, 1), z, torch.full_like(z, float("nan")))   # a rejected frame's surfaces are not written
    per_patch, _ = best_shift(z, pm.S)
    mean = torch.nanmean(z, dim=1)   # over the patches; NaN where every patch is NaN
    shifts, score = best_shift(mean, pm.S)
    return shifts.to(torch.int32), score, per_patch.to(torch.int32)


def _match(codec, bits):
    if bits not in (8, 16):
        raise ValueError("bits must be 8 or 16")
    return codec.match_patches if bits == 8 else codec.match_patches16


def estimate_shifts(codec, stream, stream_offset, stream_bytes, offsets, W, H, n, reference, positions, tw, th, S, bits=8,
                    edge="clamp"):
    """Rigid integer shifts of n frames against a reference image, by block matching straight from the compressed
    stream: K templates of tw x th are cut out of `reference` (H, W; uint8, or int16 holding U16 bits for bits=16) at
    `positions` (K, 2) and searched over -S..S in x and y in every frame (Codec.match_patches).
    Returns (shifts int32 (n, 2), score (n,), per-patch shifts int32 (n, K, 2)).  The per-frame shift is the arg-max,
    under PatchMatch.best's tie rule, of the mean over the patches of zncc(), NaNs ignored; a frame whose every entry
    is NaN gets (0, 0) and score NaN, as does a rejected frame.  The per-patch shifts are each patch's own best: the
    piecewise-rigid field.  Sign: a template cut at (X, Y) of the reference and found at (X + dx, Y + dy) of frame f
    means registered[Y][X] = frame[Y + dy][X + dx], so the shifts feed origins_from_shifts unchanged."""
    templates = templates_from_image(reference, positions, tw, th)
    origins = search_origins(positions, S, n, codec.device)
    pm, results = _match(codec, bits)(stream, stream_offset, stream_bytes, offsets, W, H, n, templates, S, origins, edge=edge)
    return _shifts_of(pm, results)


def estimate_file(codec, path, reference, positions, tw, th, S, batch=64, edge="clamp"):
    """estimate_shifts of a .dbde file that need not fit in device memory: the file is read once in pieces that hold
    `batch` frames (registered_file's reading loop), each piece is indexed on the device and matched.  Every frame is
    matched on its own, so the result equals the one-call result.  .dbde files hold 8-bit frames.
    Returns (shifts int32 (N, 2), score (N,), per-patch shifts (N, K, 2)) over the N frames of the file."""
    batch = int(batch)
    if batch < 1:
        raise ValueError("batch must be at least 1")
    parts = []
    K = _as_positions(positions).shape[0]
    with open(path, "rb") as src:
        _, (_, H, W, _) = unpack_video_header(np.frombuffer(src.read(28), np.uint8))
        W, H = int(W), int(H)
        templates = templates_from_image(reference, positions, tw, th)
        T = tiles(W, H)
        piece = batch * max_frame_bytes(W, H)          # always holds `batch` whole frames, unless the file ends
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
            pm, res = codec.match_patches(buf, 0, len(data), offs, W, H, m, templates, S,
                                          search_origins(positions, S, m, codec.device), edge=edge)
            parts.append(_shifts_of(pm, res))
            if m < n:
                end = int(offs[m].item())
            else:
                last = int(offs[m - 1].item())
                n64 = int.from_bytes(data[last + 28 + 2 * T: last + 32 + 2 * T], "little")
                end = last + 32 + 2 * T + 8 * n64
            codec.sync()   # the piece's buffer is released below
            carry = data[end:]
    if not parts:
        dev = codec.device
        return (torch.empty((0, 2), dtype=torch.int32, device=dev), torch.empty((0,), dtype=torch.float64, device=dev),
                torch.empty((0, K, 2), dtype=torch.int32, device=dev))
    return tuple(torch.cat([p[i] for p in parts]) for i in range(3))
