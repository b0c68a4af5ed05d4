"""The reference of the weighted projections (dbde_hip_project_weighted), shared by its CPU and GPU tests (test
infrastructure, like gproject_ref.py; not a test module).

The defined value (include/dbde_hip.h): with S segments of fps frames, partial P_s is the chain
acc = fmaf(w_f, (float)p_f, acc) over the accepted frames of segment s in ascending f, from +0.0f, and the result is
((prior + P_0) + P_1) + ... + P_{S-1} in F32 round-to-nearest-even additions (prior absent without accumulate).

The fused multiply-add here is a true single-rounding one, two ways:
  fmaf_libm   libm's fmaf through ctypes, one scalar at a time (the yardstick);
  fma32       numpy, whole planes at once: w * p is exact in float64 (24 x 16 significant bits), the float64 sum with
              acc is formed with its exact error (TwoSum) and rounded TO ODD, and the one rounding to binary32 (nearest
              even, gradual underflow, overflow to infinity) is numpy's float64 -> float32 conversion.  Rounding to odd
              at 53 bits commutes with a final rounding at 24 bits or fewer (Boldo and Melquiond), so this is not the
              double rounding that float64(w) * p + float64(acc) -> float32 would be.
tests/test_wproject_ref.py holds fma32 to fmaf_libm on random, subnormal, huge and tie operands.

Images are what the decoders write: dbde_hip_decode_frames' for encoded batches, tests/crafted.py's numpy decoder for
crafted frames; a rejected frame is None.
"""
import ctypes
import ctypes.util

import numpy as np

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fmaf.restype = ctypes.c_float
_libm.fmaf.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.c_float]


def fmaf_libm(w, p, acc):
    """libm fmaf(w, (float)p, acc) on scalars -> np.float32."""
    return np.float32(_libm.fmaf(float(np.float32(w)), float(p), float(np.float32(acc))))


def fma32(w, p, acc):
    """fmaf(w, (float)p, acc) elementwise: w, acc float32 (arrays or scalars), p integers below 2^16 (or float32 values
    whose product with w is exact in float64).  One rounding, to binary32."""
    with np.errstate(all="ignore"):
        a = np.asarray(w, np.float32).astype(np.float64) * np.asarray(p).astype(np.float64)   # exact
        b = np.asarray(acc, np.float32).astype(np.float64)
        a, b = np.broadcast_arrays(a, b)
        s = a + b
        bb = s - a                                  # TwoSum (Knuth): s + e == a + b exactly
        e = (a - (s - bb)) + (b - bb)
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0.0) & ((s.view(np.int64) & 1) == 0)
        toward = np.where(e > 0.0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)   # round to odd: the even neighbour gives way to the odd one
        return s.astype(np.float32)


def mul_then_add(w, p, acc):
    """What a kernel that multiplies and then adds would compute: two roundings."""
    with np.errstate(all="ignore"):
        return (np.asarray(w, np.float32) * np.asarray(p).astype(np.float32)).astype(np.float32) + np.asarray(acc, np.float32)


def _f32(hexbits):
    return np.array([hexbits], np.uint32).view(np.float32)[0]


# Named witnesses (w, p, acc): fmaf(w, p, acc) differs from round(round(w * p) + acc).  tests/test_wproject_ref.py
# checks each one (and that a search finds such operands); the GPU tests place them at a known pixel and frame.
WITNESS_U8 = (_f32(0x3F800001), 255, _f32(0xC37F0000))       # (1 + 2^-23) * 255 - 255: the product's tail is all there is
WITNESS_U16 = (_f32(0x3F800001), 65535, _f32(0xC77FFF00))    # (1 + 2^-23) * 65535 - 65535


def segment_partial(images, weights, lo, hi, x, y, rw, rh):
    """P_s: the chain over the accepted frames lo <= f < hi, from +0.0 -> float32 (R, rh, rw)."""
    R = weights.shape[0]
    acc = np.zeros((R, rh, rw), np.float32)
    for f in range(lo, hi):
        if images[f] is None:
            continue
        win = np.asarray(images[f])[y:y + rh, x:x + rw].astype(np.int64)[None]
        acc = fma32(weights[:, f].reshape(R, 1, 1), win, acc)
    return acc


def wproject(images, weights, x, y, rw, rh, segments=1, fps=None, accumulate=False, prior=None):
    """The defined value -> (float32 (R, rh, rw), count).  images: per frame an (H, W) array or None (rejected);
    weights: float32 (R, >= n); segments, fps: the plan's; prior: the planes' old content when accumulating."""
    weights = np.asarray(weights, np.float32)
    if weights.ndim == 1:
        weights = weights[None]
    n = len(images)
    fps = n if fps is None else fps
    count = sum(im is not None for im in images)
    if accumulate and n == 0:
        return np.array(prior, np.float32), 0
    parts = [segment_partial(images, weights, s * fps, min((s + 1) * fps, n), x, y, rw, rh) for s in range(max(segments, 1))]
    with np.errstate(all="ignore"):
        if accumulate:
            v = np.array(prior, np.float32)
        else:
            v, parts = parts[0], parts[1:]
        for part in parts:
            v = (v + part).astype(np.float32)
    return v, count


def bits(a):
    """float32 array -> its int32 bit patterns (the comparison the GPU tests make)."""
    return np.ascontiguousarray(a, np.float32).view(np.int32)
