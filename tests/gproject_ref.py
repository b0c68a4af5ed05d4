"""The numpy reference of the grouped projections (dbde_hip_project_groups), shared by its CPU and GPU tests (test
infrastructure, like family_refs.py; not a test module).

group_ranges: the frames [b, e) of every group, by the call's rule -- the uniform form's ragged last group, the ragged
form's clamping (entries above n, decreasing entries, overlapping ranges).
reduce_groups: family_refs.reduce_numpy / reduce16 over each group's accepted frames, stacked per statistic.
"""
import numpy as np

from family_refs import reduce16, reduce_numpy

ALL = ("max", "min", "sum", "sumsq")


def group_ranges(n, group_frames=None, starts=None):
    """[(b, e)] per group.  Uniform: [k*g, min((k+1)*g, n)) for k < ceil(n / g).  Ragged (starts: n_groups + 1 U32
    values): b = min(s[k], n), e = min(max(s[k+1], s[k]), n)."""
    if (group_frames is None) == (starts is None):
        raise ValueError("exactly one of group_frames and starts")
    if starts is None:
        g = int(group_frames)
        if g < 1:
            raise ValueError("group_frames < 1")
        return [(k * g, min((k + 1) * g, n)) for k in range(-(-n // g))]
    s = [int(v) for v in starts]
    if len(s) < 2:
        raise ValueError("the ragged form needs n_groups >= 1")
    return [(min(s[k], n), min(max(s[k + 1], s[k]), n)) for k in range(len(s) - 1)]


def reduce_groups(images, ranges, x, y, rw, rh, pix=1):
    """images: per frame an (H, W) array, or None for a rejected frame.  Returns int64 arrays max / min / sum / sumsq of
    shape (n_groups, rh, rw) and counts (n_groups,)."""
    red = reduce_numpy if pix == 1 else reduce16
    per = [red([im for im in images[b:e] if im is not None], x, y, rw, rh) for b, e in ranges]
    out = {s: np.stack([np.asarray(p[s], np.int64) for p in per]) if per else np.zeros((0, rh, rw), np.int64)
           for s in ALL}
    out["counts"] = np.array([p["count"] for p in per], np.int64)
    return out
