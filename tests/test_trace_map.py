"""CPU: dbde_hip_trace_map_summary (dv.trace_map_summary) -- the trace map's tile classes and per-label pixel counts,
against a numpy classification written here from the rules in include/dbde_hip.h.  Pure host code; no GPU."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.fixture(scope="module")
def dv():
    import dbde_video_cpp_amd as m
    if not os.path.exists(m.LIB_PATH):
        m.build()
    return m


def classify(labels):
    """(tiles, active, whole, mixed) per the rules: only valid pixels count; padding belongs to no region; a whole tile
    has no padding and one label > 0 throughout; every other tile with a label > 0 is mixed."""
    H, W = labels.shape
    w, h = (W + 7) // 8, (H + 7) // 8
    whole = mixed = 0
    for ty in range(h):
        for tx in range(w):
            t = labels[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8]
            if not (t > 0).any():
                continue
            if t.shape == (8, 8) and (t == t[0, 0]).all():
                whole += 1
            else:
                mixed += 1
    return w * h, whole + mixed, whole, mixed


def check(dv, labels, n_labels=None):
    d = dv.trace_map_summary(labels, n_labels)
    L = int(labels.max()) if n_labels is None else n_labels
    tiles, active, whole, mixed = classify(labels)
    H, W = labels.shape
    assert (d["W"], d["H"], d["n_labels"]) == (W, H, L)
    assert (d["tiles"], d["tiles_active"], d["tiles_whole"], d["tiles_mixed"]) == (tiles, active, whole, mixed)
    assert np.array_equal(d["pixels"], np.bincount(labels.reshape(-1), minlength=L + 1)[1:])
    assert d["device_bytes"] > 0
    return d


def discs(W, H, count, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    lab = np.zeros((H, W), np.int32)
    for k in range(count):
        cx, cy, r = rng.integers(0, W), rng.integers(0, H), rng.integers(2, 20)
        lab[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = k + 1
    return lab


def test_all_zero_labels(dv):
    d = check(dv, np.zeros((64, 48), np.int32), 3)
    assert d["tiles_active"] == 0 and (d["pixels"] == 0).all()


def test_one_label_over_the_whole_frame(dv):
    d = check(dv, np.ones((64, 128), np.int32))
    assert d["tiles_whole"] == d["tiles"] == 128 and d["tiles_mixed"] == 0


def test_aligned_blocks_give_only_whole_tiles(dv):
    by, bx = np.mgrid[0:96, 0:160]
    lab = ((by // 16) * 10 + bx // 16 + 1).astype(np.int32)
    lab[(by // 16 + bx // 16) % 4 == 0] = 0
    d = check(dv, lab)
    assert d["tiles_mixed"] == 0 and d["tiles_whole"] > 0


@pytest.mark.parametrize("W,H,count", [(200, 123, 30), (256, 256, 60), (1921, 33, 12)])
def test_discs_give_whole_and_mixed_tiles(dv, W, H, count):
    d = check(dv, discs(W, H, count, W + H))
    assert d["tiles_whole"] > 0 and d["tiles_mixed"] > 0


def test_single_pixel_labels(dv):
    rng = np.random.default_rng(3)
    lab = np.zeros((77, 91), np.int32)
    idx = rng.choice(lab.size, 200, replace=False)
    lab.reshape(-1)[idx] = np.arange(1, 201)
    d = check(dv, lab)
    assert d["tiles_whole"] == 0 and (d["pixels"] == 1).all()


@pytest.mark.parametrize("W,H", [(9, 9), (100, 75), (13, 64), (64, 13), (1, 1)])
def test_edge_tiles_are_mixed_and_padding_never_counts(dv, W, H):
    d = check(dv, np.full((H, W), 2, np.int32), 2)
    w, h = (W + 7) // 8, (H + 7) // 8
    edge = w * h - (W // 8) * (H // 8)
    assert d["tiles_mixed"] == edge and d["tiles_whole"] == (W // 8) * (H // 8)
    assert list(d["pixels"]) == [0, W * H]


def test_largest_label_count(dv):
    lab = np.zeros((16, 16), np.int32)
    lab[3, 4] = 65535
    d = check(dv, lab, 65535)
    assert d["pixels"][-1] == 1 and d["pixels"][:-1].sum() == 0


@pytest.mark.parametrize("labels,n_labels", [
    (np.full((8, 8), -1, np.int32), 3),          # below 0
    (np.full((8, 8), 4, np.int32), 3),           # above n_labels
    (np.zeros((8, 8), np.int32), 0),             # L = 0
    (np.zeros((8, 8), np.int32), None),          # L defaults to max() = 0
    (np.zeros((8, 8), np.int32), 65536),         # L above 65,535
    (np.full((8, 8), 65536, np.int64), None),    # a label above 65,535
])
def test_bad_labels_raise(dv, labels, n_labels):
    with pytest.raises(ValueError):
        dv.trace_map_summary(labels, n_labels)


def test_c_entry_point_validates_on_its_own(dv):
    """The C function, not only the Python wrapper, rejects out-of-range labels and label counts."""
    import ctypes as C
    lib = dv.lib()
    good = np.zeros((8, 8), np.int32)
    bad = good.copy()
    bad[7, 7] = 9
    assert lib.dbde_hip_trace_map_summary(good.ctypes.data, 8, 8, 3, None, None) == dv.OK
    assert lib.dbde_hip_trace_map_summary(bad.ctypes.data, 8, 8, 3, None, None) == dv.ERR_ARG
    bad[7, 7] = -1
    assert lib.dbde_hip_trace_map_summary(bad.ctypes.data, 8, 8, 3, None, None) == dv.ERR_ARG
    assert lib.dbde_hip_trace_map_summary(good.ctypes.data, 8, 8, 0, None, None) == dv.ERR_ARG
    assert lib.dbde_hip_trace_map_summary(good.ctypes.data, 8, 8, 65536, None, None) == dv.ERR_ARG
    assert lib.dbde_hip_trace_map_summary(None, 8, 8, 3, None, None) == dv.ERR_ARG
    assert lib.dbde_hip_trace_map_summary(good.ctypes.data, 0, 8, 3, None, None) == dv.ERR_ARG
    assert lib.dbde_hip_trace_map_create(None, good.ctypes.data, 8, 8, 3, C.byref(C.c_void_p())) == dv.ERR_ARG


def test_torch_input(dv):
    import torch
    lab = discs(100, 75, 9, 4)
    assert dv.trace_map_summary(torch.from_numpy(lab))["tiles_active"] == dv.trace_map_summary(lab)["tiles_active"]
