"""The expected planes of a binned decode (dbde_hip_decode_binned), straight from the definition, two ways.

Element (i, j) of a frame reduces rows [y + i b, min(y + i b + b, y + rh)) and columns [x + j b, min(x + j b + b,
x + rw)) of the decoded image.  binned_reduceat does it with numpy's reduceat over the window, binned_loop with a plain
loop over the bins; tests/test_binned_ref.py requires the two to agree.  Not a test module.
"""
import numpy as np

STATS = ("sum", "max", "min")
UFUNC = {"sum": np.add, "max": np.maximum, "min": np.minimum}


def out_shape(rw, rh, b):
    return -(-rh // b), -(-rw // b)


def binned_reduceat(images, x, y, rw, rh, b):
    """images: (n, H, W) or (H, W) integers -> {"sum", "max", "min"}: int64 (n, oh, ow) (or (oh, ow))."""
    win = np.asarray(images)[..., y:y + rh, x:x + rw].astype(np.int64)
    rows, cols = np.arange(0, rh, b), np.arange(0, rw, b)
    return {s: UFUNC[s].reduceat(UFUNC[s].reduceat(win, rows, axis=-2), cols, axis=-1) for s in STATS}


def binned_loop(image, x, y, rw, rh, b):
    """One (H, W) image, bin by bin."""
    oh, ow = out_shape(rw, rh, b)
    out = {s: np.zeros((oh, ow), np.int64) for s in STATS}
    for i in range(oh):
        for j in range(ow):
            blk = image[y + i * b: min(y + i * b + b, y + rh), x + j * b: min(x + j * b + b, x + rw)].astype(np.int64)
            out["sum"][i, j], out["max"][i, j], out["min"][i, j] = blk.sum(), blk.max(), blk.min()
    return out


def bin_pixels(rw, rh, b):
    """int64 (oh, ow): the pixels of each bin."""
    ny = np.minimum(b, rh - np.arange(0, rh, b))
    nx = np.minimum(b, rw - np.arange(0, rw, b))
    return ny[:, None] * nx[None, :]


def windows(W, H, b):
    """The windows every shape is checked with: the full frame; an odd-sized window at a multiple of b (for b < 8 not
    of 8) where the frame has room for one; 1 x 1 at the last multiple of b inside the frame; a full-width window one
    pixel high; a full-height window one pixel wide."""
    out = [(0, 0, W, H)]
    x0, y0 = b + 8 * (W // 56), b + 8 * (H // 40)   # b mod 8
    if W - x0 >= 3 and H - y0 >= 3:
        rw, rh = (W - x0) * 3 // 4, (H - y0) * 3 // 4
        out.append((x0, y0, rw - 1 + rw % 2, rh - 1 + rh % 2))
    out.append(((W - 1) // b * b, (H - 1) // b * b, 1, 1))
    out.append((0, (H // 3) // b * b, W, 1))
    out.append(((W // 2) // b * b, 0, 1, H))
    return out
