"""CPU reference of the neighbour-product projections (dbde_hip_project_pairs) and of the local correlation image
(test infrastructure, not a test module).  Integer arithmetic in Python / numpy from decoded images; the correlation is
a two-pass Pearson per pair over the stacked time courses, written independently of the package's."""
import numpy as np

OFFSETS = ((1, 0), (0, 1), (1, 1), (-1, 1))   # (dx, dy) of mask bits 0..3: RIGHT, DOWN, DOWN_RIGHT, DOWN_LEFT


def offsets_of(mask):
    """The (dx, dy) of each plane of mask, in plane order."""
    assert 1 <= mask <= 15, mask
    return [OFFSETS[b] for b in range(4) if (mask >> b) & 1]


def spans(dx, dy, rw, rh):
    """(first, partner) slices of a (rh, rw) window for offset (dx, dy): first[y][x] pairs with partner = [y+dy][x+dx]."""
    xa = slice(max(0, -dx), rw - max(0, dx))
    xb = slice(max(0, dx), rw - max(0, -dx))
    return (slice(0, rh - dy), xa), (slice(dy, rh), xb)


def pairs(images, mask, x, y, rw, rh):
    """images: the decoded frames, each (H, W) uint8 / uint16, None for a rejected frame.  Returns (planes uint64
    (popcount(mask), rh, rw), count): planes[j][yy][xx] = sum over the accepted frames of win[yy][xx] *
    win[yy + dy][xx + dx] with (dx, dy) the j-th set bit's offset and win = frame[y:y+rh, x:x+rw]; 0 where the partner
    lies outside the window.  Exact: Python integers via object arrays would be slow, uint64 never overflows here
    (a product is below 2^32 and the tests' frame counts are far below 2^31)."""
    offs = offsets_of(mask)
    out = np.zeros((len(offs), rh, rw), np.uint64)
    count = 0
    for im in images:
        if im is None:
            continue
        count += 1
        win = np.asarray(im)[y:y + rh, x:x + rw].astype(np.uint64)
        for j, (dx, dy) in enumerate(offs):
            a, b = spans(dx, dy, rw, rh)
            out[j][a] += win[a] * win[b]
    return out, count


def has_partner(mask, rw, rh):
    """bool (popcount(mask), rh, rw): the elements whose partner lies inside the window."""
    offs = offsets_of(mask)
    m = np.zeros((len(offs), rh, rw), bool)
    for j, (dx, dy) in enumerate(offs):
        m[j][spans(dx, dy, rw, rh)[0]] = True
    return m


def local_correlation(images, mask, x, y, rw, rh):
    """float64 (rh, rw): for every pixel the mean, over its neighbours inside the window along the offsets of mask (both
    directions of each), of the Pearson correlation of the two time courses over the accepted frames; a pair with a
    constant member is left out; no pair left gives 0.  Two passes: subtract each course's mean, then correlate."""
    st = np.stack([np.asarray(im)[y:y + rh, x:x + rw] for im in images if im is not None]).astype(np.float64)
    dev = st - st.mean(0)
    var = (dev * dev).sum(0)
    total = np.zeros((rh, rw))
    number = np.zeros((rh, rw))
    for dx, dy in offsets_of(mask):
        a, b = spans(dx, dy, rw, rh)
        cov = (dev[(slice(None),) + a] * dev[(slice(None),) + b]).sum(0)
        ok = (var[a] > 0) & (var[b] > 0)
        r = np.where(ok, cov / np.sqrt(np.where(ok, var[a] * var[b], 1.0)), 0.0)
        total[a] += r
        total[b] += r
        number[a] += ok
        number[b] += ok
    return np.where(number > 0, total / np.maximum(number, 1), 0.0)
