"""The count projection's reference (test infrastructure; not a test module): numpy on decoded images.

counts(images, thr, x, y, rw, rh) -> (planes uint32 (K, rh, rw), count): plane k holds, per window pixel, the number of
accepted frames (images[f] is not None) whose pixel is <= thr[k], an unsigned compare in the pixel type.  thr is (K,)
scalars or (K, rh, rw) maps in window coordinates."""
import numpy as np


def counts(images, thr, x, y, rw, rh):
    ok = [np.asarray(im) for im in images if im is not None]
    thr = np.asarray(thr)
    assert thr.dtype in (np.uint8, np.uint16), thr.dtype
    K = thr.shape[0]
    t = thr.reshape(K, 1, 1) if thr.ndim == 1 else thr
    assert t.shape in ((K, 1, 1), (K, rh, rw)), t.shape
    if not ok:
        return np.zeros((K, rh, rw), np.uint32), 0
    win = np.stack([im[y:y + rh, x:x + rw] for im in ok])
    assert win.dtype == thr.dtype, (win.dtype, thr.dtype)
    return (win[None] <= t[:, None]).sum(1).astype(np.uint32), len(ok)


def order_statistic(images, q, x, y, rw, rh):
    """sorted[floor(q * (N - 1))] of the accepted frames per window pixel (numpy's method="lower"); zeros for N = 0."""
    ok = [np.asarray(im)[y:y + rh, x:x + rw] for im in images if im is not None]
    if not ok:
        return np.zeros((rh, rw), np.uint8), 0
    r = int(np.floor(q * (len(ok) - 1)))
    return np.sort(np.stack(ok), 0)[r], len(ok)
