"""What the tests of the neighbour-product projections share (test infrastructure, like counts_gpu.py; not a test
module): the cap that keeps a case from passing with offsets swapped, a pixel paired with itself or nothing counted, and
the one check every GPU case runs -- the call against tests/pairs_ref.py, by equality."""
import numpy as np

import pairs_ref as pref

MASKS = (1, 2, 4, 8, 3, 15, 10)     # every offset alone, the two neighbourhoods and a non-contiguous mask


def planes(out):
    """PairProjection.out (int64) as the U64 planes it holds, on the host."""
    return out.out.cpu().numpy().view(np.uint64)


def sumsq(images, win):
    x, y, rw, rh = win
    return sum(np.asarray(im)[y:y + rh, x:x + rw].astype(np.uint64) ** 2 for im in images if im is not None)


def distinct(want, self_products=None):
    """The cap: the expected planes of a case are pairwise different, none is all zero and each differs from the window's
    sum of squares (a pixel paired with itself).  Compared on the interior [:-1, 1:-1], where every offset has its
    partner, so that the zero edges (which differ from offset to offset) do not tell the planes apart by themselves.
    Applies where the window is at least 3 x 3."""
    inner = [np.asarray(p)[:-1, 1:-1] for p in want]
    assert inner[0].size > 0, "the window is smaller than 3 x 3"
    for i in range(len(inner)):
        assert inner[i].any(), f"plane {i} is all zero"
        if self_products is not None:
            assert not np.array_equal(inner[i], self_products[:-1, 1:-1]), f"plane {i} equals the sum of squares"
        for j in range(i):
            assert not np.array_equal(inner[i], inner[j]), f"planes {j} and {i} are equal"


def expected(images, mask, win, cap=True):
    """pairs_ref on the window, with the cap on all four offsets of the same content (so that a call that computes
    another offset than the one asked for differs) where the window is at least 3 x 3."""
    x, y, rw, rh = win
    want, count = pref.pairs(images, mask, x, y, rw, rh)
    if cap and rw >= 3 and rh >= 3 and count > 0:
        distinct(pref.pairs(images, 15, x, y, rw, rh)[0], sumsq(images, win))
    return want, count


def check(call, s, mask, win, what="", cap=True, **kw):
    """One call on stream s (wproject_gpu.Stream) against pairs_ref.  Returns (out, results)."""
    import torch
    x, y, rw, rh = win
    want, count = expected(s.images, mask, win, cap)
    out, res = call(s.buf, s.lead, s.total, s.offs, s.W, s.H, s.n, pref.offsets_of(mask), x, y, rw, rh, **kw)
    torch.cuda.synchronize()
    what = f"{what} {s.W}x{s.H} n={s.n} mask={mask} {win}"
    assert out.out.dtype == torch.int64 and tuple(out.out.shape) == (len(want), rh, rw), what
    assert list(out.offsets) == pref.offsets_of(mask), what
    got = planes(out)
    if not np.array_equal(got, want):
        bad = tuple(np.argwhere(got != want)[0])
        raise AssertionError(f"{what}: differs at {bad}: {got[bad]} != {want[bad]}; {int((got != want).sum())} of "
                             f"{got.size} elements")
    assert int(out.count.item()) == count, (what, "count")
    return out, res
