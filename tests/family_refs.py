"""The numpy / torch references of the projection, trace and histogram families, shared by their GPU tests and by
tests/sequences.py (test infrastructure, like binned_ref.py; not a test module).

reduce_numpy / reduce16: exact int64 max / min / sum / sumsq of a window over a list of decoded images (DBDE / DBDE16).
map_discs, reduce_labels: a label map of random discs, and the per-frame, per-label reductions of images over a map.
hist_expect / hist_expect16: per-frame counts of min(v >> shift, bins - 1) over a window.
"""
import numpy as np


def reduce_numpy(images, x, y, rw, rh):
    """Exact int64 reductions of the window over a list of (H, W) uint8 numpy images; the empty projection for none."""
    if not images:
        z = np.zeros((rh, rw), np.int64)
        return dict(max=z, min=z + 255, sum=z, sumsq=z, count=0)
    w = np.stack([im[y:y + rh, x:x + rw] for im in images]).astype(np.int64)
    return dict(max=w.max(0), min=w.min(0), sum=w.sum(0), sumsq=(w * w).sum(0), count=len(images))


def reduce16(images, x, y, rw, rh):
    """reduce_numpy for DBDE16: a list (or array) of (H, W) uint16 images."""
    if len(images) == 0:
        z = np.zeros((rh, rw), np.int64)
        return dict(max=z, min=z + 65535, sum=z, sumsq=z, count=0)
    w = np.stack([np.asarray(im)[y:y + rh, x:x + rw] for im in images]).astype(np.int64)
    return dict(max=w.max(0), min=w.min(0), sum=w.sum(0), sumsq=(w * w).sum(0), count=len(images))


def map_discs(W, H, seed=1, count=None):
    """Random discs (later ones over earlier ones): whole and mixed tiles."""
    rng = np.random.default_rng(seed)
    lab = np.zeros((H, W), np.int32)
    count = count or max(2, min(300, W * H // 400))
    yy, xx = np.mgrid[0:H, 0:W]
    r_max = max(2, min(W, H) // 6)
    for k in range(count):
        cx, cy, r = rng.integers(0, W), rng.integers(0, H), rng.integers(1, r_max + 1)
        y0, y1, x0, x1 = max(0, cy - r), min(H, cy + r + 1), max(0, cx - r), min(W, cx + r + 1)
        sub = (yy[y0:y1, x0:x1] - cy) ** 2 + (xx[y0:y1, x0:x1] - cx) ** 2 <= r * r
        lab[y0:y1, x0:x1][sub] = k + 1
    return lab, count


def reduce_labels(images, labels, L, pix_max=255):
    """int64 reductions of (n, H, W) images (torch, any integer type holding the values) over the label map:
    dict of (n, L) int64 tensors on the images' device.  The empty reduction where a label has no pixels."""
    import torch
    dev = images.device
    n = images.shape[0]
    lab = torch.from_numpy(np.ascontiguousarray(labels, np.int64)).to(dev).reshape(-1)
    keep = lab > 0
    idx = (lab[keep] - 1).unsqueeze(0)
    out = dict(max=torch.zeros((n, L), dtype=torch.int64, device=dev),
               min=torch.full((n, L), pix_max, dtype=torch.int64, device=dev),
               sum=torch.zeros((n, L), dtype=torch.int64, device=dev),
               sumsq=torch.zeros((n, L), dtype=torch.int64, device=dev))
    for f0 in range(0, n, 4):   # a few frames at a time: 4096 x 3072 int64 images are large
        v = images[f0:f0 + 4].reshape(min(4, n - f0), -1)[:, keep].to(torch.int64)
        ix = idx.expand(v.shape[0], -1)
        sl = slice(f0, f0 + v.shape[0])
        out["max"][sl] = out["max"][sl].scatter_reduce(1, ix, v, "amax", include_self=True)
        out["min"][sl] = out["min"][sl].scatter_reduce(1, ix, v, "amin", include_self=True)
        out["sum"][sl] = out["sum"][sl].scatter_add(1, ix, v)
        out["sumsq"][sl] = out["sumsq"][sl].scatter_add(1, ix, v * v)
    return out


def hist_expect(images, x, y, rw, rh, shift, bins, keep=None):
    """int64 (n, bins): the counts of each frame's window (torch images (n, H, W) or a list of numpy images)."""
    import torch
    if isinstance(images, list):
        images = torch.from_numpy(np.stack(images)) if images else torch.zeros((0, y + rh, x + rw), dtype=torch.uint8)
    win = images[:, y:y + rh, x:x + rw].to(torch.int64)
    b = (win >> shift).clamp(max=bins - 1).reshape(win.shape[0], -1)
    out = torch.zeros((win.shape[0], bins), dtype=torch.int64, device=win.device)
    for f in range(win.shape[0]):
        if keep is None or keep[f]:
            out[f] = torch.bincount(b[f], minlength=bins)
    return out


def hist_expect16(images, x, y, rw, rh, shift, bins, keep=None):
    """int64 (n, bins) from uint16 numpy images (n, H, W)."""
    import torch
    w = torch.from_numpy(np.ascontiguousarray(np.asarray(images)[:, y:y + rh, x:x + rw]).astype(np.int64))
    b = (w >> shift).clamp(max=bins - 1).reshape(w.shape[0], -1)
    out = torch.zeros((w.shape[0], bins), dtype=torch.int64)
    for f in range(w.shape[0]):
        if keep is None or keep[f]:
            out[f] = torch.bincount(b[f], minlength=bins)
    return out
