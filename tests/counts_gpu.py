"""What the GPU tests of the count projections share (test infrastructure, like wproject_gpu.py; not a test module):
threshold families drawn with tests/counts_ref.py on the CPU so that no case can pass by counting nothing, device
thresholds in the package's dtypes, and the one check every case runs -- the call against counts_ref, by equality."""
import numpy as np

import counts_ref as cref


def np_dtype(bits):
    return np.uint8 if bits == 8 else np.uint16


def device(thr):
    """numpy uint8 / uint16 thresholds -> the device tensor the package takes (uint8, or int16 holding the U16 bits)."""
    import torch
    thr = np.ascontiguousarray(thr)
    return torch.from_numpy(thr if thr.dtype == np.uint8 else thr.view(np.int16)).cuda()


def planes(out):
    """CountProjection.out (int32) as the U32 planes it holds, on the host."""
    return out.out.cpu().numpy().view(np.uint32)


def window_stack(images, win):
    x, y, rw, rh = win
    return np.stack([im[y:y + rh, x:x + rw] for im in images if im is not None])


def capped(want, N):
    """The cap: every level's expected plane has a pixel with 0 < count < N (N = 1: the plane holds both 0 and 1)."""
    if N == 1:
        return all((p == 0).any() and (p == 1).any() for p in want)
    return all(((p > 0) & (p < N)).any() for p in want)


def draw(rng, images, win, K, bits, maps, over_data=False, tries=400):
    """Uniform random thresholds, (K,) or (K, rh, rw), redrawn (on the CPU, with counts_ref) until the cap holds.  A
    one-pixel window draws from the range of its own values, where a uniform draw over the whole pixel range would
    almost never cut all K levels through one pixel's few samples (over_data=True does the same for content that
    fills a small part of the pixel range); with one frame and one pixel no plane can hold both 0 and 1, and the K
    levels together must (K > 1) -- K = 1 is then returned as drawn.  Where half the tries over the whole range find
    nothing (a small window whose few tiles fill a narrow band), the rest draw over the data's range as well."""
    x, y, rw, rh = win
    st = window_stack(images, win)
    N, top = st.shape[0], (1 << bits) - 1
    data = (int(st.min()), int(st.max()))
    for i in range(tries):
        lo, hi = data if (rw * rh == 1 and N > 1) or over_data or 2 * i >= tries else (0, top + 1)
        thr = rng.integers(lo, max(hi, lo + 1), (K, rh, rw) if maps else (K,)).astype(np_dtype(bits))
        want, n = cref.counts(images, thr, x, y, rw, rh)
        assert n == N
        if rw * rh == 1 and N == 1:
            if K == 1 or ((want == 0).any() and (want == 1).any()):
                return thr
        elif capped(want, N):
            return thr
    raise AssertionError(f"no thresholds with 0 < count < N at every level: window {win}, K={K}, N={N}")


def check(call, s, thr, win, what="", **kw):
    """One call on stream s (wproject_gpu.Stream) with numpy thresholds against counts_ref.  Returns (out, results)."""
    import torch
    x, y, rw, rh = win
    want, count = cref.counts(s.images, thr, x, y, rw, rh)
    out, res = call(s.buf, s.lead, s.total, s.offs, s.W, s.H, s.n, device(thr), x, y, rw, rh, **kw)
    torch.cuda.synchronize()
    what = f"{what} {s.W}x{s.H} n={s.n} K={thr.shape[0]} {win} {'maps' if thr.ndim == 3 else 'scalars'}"
    assert out.out.dtype == torch.int32 and tuple(out.out.shape) == (thr.shape[0], rh, rw), what
    got = planes(out)
    if not np.array_equal(got, want):
        bad = tuple(np.argwhere(got != want)[0])
        raise AssertionError(f"{what}: differs at {bad}: {got[bad]} != {want[bad]}; {int((got != want).sum())} of "
                             f"{got.size} elements")
    assert int(out.count.item()) == count, (what, "count")
    return out, res
