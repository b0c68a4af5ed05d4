"""The reference of the lag projections (dbde_hip_project_lag), in numpy from decoded images (None = rejected), written
from the definition in include/dbde_hip.h: pair f is (a, b) = (p[f - lag], p[f]) at the same window pixel and is counted
iff f >= max(lead, lag) and frames f and f - lag are both accepted.  Not a test module."""
import numpy as np

STATS = ("product", "pairsum", "absdiff", "sqdiff", "maxdiff")
ALL = 31


def names_of(mask):
    return tuple(STATS[b] for b in range(5) if (mask >> b) & 1)


def mask_of(names):
    return sum(1 << STATS.index(k) for k in names)


def counted(images, lag, lead=0):
    """The later frame index of every counted pair."""
    return [f for f in range(max(lead, lag), len(images)) if images[f] is not None and images[f - lag] is not None]


def window(im, x, y, rw, rh):
    return np.asarray(im)[y:y + rh, x:x + rw].astype(np.int64)


def lag(images, lag, x, y, rw, rh, lead=0, bits=8):
    """{"product", "pairsum", "absdiff", "sqdiff": uint64 (rh, rw), "maxdiff": uint8 / uint16 (rh, rw), "pairs": int,
    "count": int} over the counted pairs; count = accepted frames with index >= lead."""
    px = np.uint8 if bits == 8 else np.uint16
    out = {k: np.zeros((rh, rw), np.uint64) for k in STATS[:4]}
    mx = np.zeros((rh, rw), np.int64)
    fs = counted(images, lag, lead)
    for f in fs:
        a, b = window(images[f - lag], x, y, rw, rh), window(images[f], x, y, rw, rh)
        out["product"] += (a * b).astype(np.uint64)
        out["pairsum"] += (a + b).astype(np.uint64)
        out["absdiff"] += np.abs(b - a).astype(np.uint64)
        out["sqdiff"] += ((b - a) ** 2).astype(np.uint64)
        mx = np.maximum(mx, np.abs(b - a))
    out["maxdiff"] = mx.astype(px)
    out["pairs"] = len(fs)
    out["count"] = sum(im is not None for im in images[lead:])
    return out


def lag_expanded(images, lag, x, y, rw, rh, lead=0, bits=8):
    """The second, independent formulation: stacks instead of a loop, sqdiff from sum a^2 + sum b^2 - 2 sum a b,
    absdiff from sum max(a, b) - sum min(a, b), pairsum from the two stacks' sums, in Python integers (object arrays)."""
    fs = counted(images, lag, lead)
    zero = np.zeros((rh, rw), object)
    if not fs:
        return {"product": zero, "pairsum": zero, "absdiff": zero, "sqdiff": zero, "maxdiff": zero, "pairs": 0}
    A = np.stack([window(images[f - lag], x, y, rw, rh) for f in fs]).astype(object)
    B = np.stack([window(images[f], x, y, rw, rh) for f in fs]).astype(object)
    ab = (A * B).sum(0)
    hi, lo = np.maximum(A, B), np.minimum(A, B)
    return {"product": ab, "pairsum": A.sum(0) + B.sum(0), "absdiff": hi.sum(0) - lo.sum(0),
            "sqdiff": (A * A).sum(0) + (B * B).sum(0) - 2 * ab, "maxdiff": (hi - lo).max(0), "pairs": len(fs)}


def combine(prior, new):
    """What an accumulating call leaves: the sums and scalars added, the maximum taken."""
    out = {k: prior[k] + new[k] for k in STATS[:4] + ("pairs", "count")}
    out["maxdiff"] = np.maximum(prior["maxdiff"], new["maxdiff"])
    return out


def split_calls(n, lag, B):
    """The header's split rule: [(first frame, frames, lead)] of the calls that together equal one call on [0, n)."""
    assert B >= lag
    calls = [(0, min(B, n), 0)]
    k = 1
    while k * B < n:
        calls.append((k * B - lag, min((k + 1) * B, n) - (k * B - lag), lag))
        k += 1
    return calls


def lag_split(images, lag_, x, y, rw, rh, B, bits=8):
    """The reference evaluated call by call under the split rule."""
    total = None
    for lo, cnt, lead in split_calls(len(images), lag_, B):
        part = lag(images[lo:lo + cnt], lag_, x, y, rw, rh, lead, bits)
        total = part if total is None else combine(total, part)
    return total


def sumsq_later(images, lag, x, y, rw, rh, lead=0):
    """sum b^2 over the counted pairs: what a lag of 0 (a pixel paired with itself) would give as the product."""
    out = np.zeros((rh, rw), np.uint64)
    for f in counted(images, lag, lead):
        out += (window(images[f], x, y, rw, rh) ** 2).astype(np.uint64)
    return out


def autocorrelation_two_pass(images, lag, x, y, rw, rh):
    """Two passes over the stacked time courses of the accepted frames: mu and the population variance over the
    accepted frames, then the mean over the counted pairs of (a - mu)(b - mu), divided by the variance; 0 where the
    variance is 0 or no pair is counted."""
    acc = [window(im, x, y, rw, rh).astype(np.float64) for im in images if im is not None]
    fs = counted(images, lag)
    if not acc or not fs:
        return np.zeros((rh, rw))
    X = np.stack(acc)
    mu = X.mean(0)
    var = ((X - mu) ** 2).mean(0)
    A = np.stack([window(images[f - lag], x, y, rw, rh) for f in fs]).astype(np.float64)
    B = np.stack([window(images[f], x, y, rw, rh) for f in fs]).astype(np.float64)
    cov = ((A - mu) * (B - mu)).mean(0)
    flat = X.max(0) == X.min(0)
    return np.where(flat, 0.0, cov / np.where(flat, 1.0, var))
