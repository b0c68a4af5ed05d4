"""The scaled float decode's definition in numpy, and the standard test maps (helper; no test of its own).

For the pixel at frame coordinates (X, Y) with decoded value p (U8 or U16), dbde_hip_decode_scaled writes
    v = ((float32)p - D[Y, X]) * G[Y, X]
as two binary32 operations, each rounded to nearest even, then rounds v once, to nearest even, to F32 / F16 / BF16.
Everything here returns BIT PATTERNS (uint32 for F32, uint16 for F16 and BF16), so that comparisons tell -0 from +0 and
see infinities and subnormals.

The standard maps keep the reference independent of denormal modes: dark uniform in [0, 300) (non-integers included),
gain = +-2^u with u uniform in [-8, 8], and some pixels forced to p == D so that +-0 occurs.  p is an integer, so a
non-zero |p - D| is at least the last bit of D (2^-23 D or more), and a uniform draw over [0, 300) is never near
1e-30: times 2^-8 the product stays far above the smallest normal binary32 (1.2e-38), and no F32 intermediate is
subnormal.  F16 results overflow to inf (300 * 256 > 65504) and fall into the F16 subnormal range (below 6.1e-5).
tests/test_scaled_ref.py checks all three on the maps themselves.

The standard maps still avoid binary32 subnormals; that range, and the operands on which a rounding can go wrong
(ties, double roundings, the overflow edges), belong to tests/scaled_witness.py: its exact integer reference is the
definition, and tests/test_scaled_witness.py checks scaled_bits against it over the whole binary32 range.
"""
import numpy as np

TYPES = ("f32", "f16", "bf16")
OUT = {"f32": 0, "f16": 1, "bf16": 2}          # DBDE_HIP_OUT_*
BITS = {"f32": np.uint32, "f16": np.uint16, "bf16": np.uint16}
F32_MIN_NORMAL = np.float32(2.0 ** -126)


def torch_dtype(t):
    import torch
    return {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}[t]


def bf16_bits(v):
    """float32 array -> uint16 bit patterns of round-to-nearest-even bfloat16 (NaN stays a quiet NaN)."""
    b = np.ascontiguousarray(v, np.float32).view(np.uint32)
    r = ((b.astype(np.uint64) + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (b & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, ((b >> 16) | 0x40).astype(np.uint16), r)


def value(p, dark, gain):
    """v as float32: (p - D) * G, the two operations in binary32."""
    # inf - inf, 0 * inf in maps that hold special values: NaN, as IEEE has it; products may overflow and underflow
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        d = np.subtract(np.asarray(p).astype(np.float32), np.asarray(dark, np.float32), dtype=np.float32)
        return np.multiply(d, np.asarray(gain, np.float32), dtype=np.float32)


def scaled_bits(p, dark, gain, t):
    """Bit patterns of the scaled decode of pixels p (any shape that broadcasts against the maps) in type t."""
    v = np.ascontiguousarray(value(p, dark, gain))
    if t == "f32":
        return v.view(np.uint32)
    if t == "f16":
        with np.errstate(over="ignore", under="ignore"):
            return v.astype(np.float16).view(np.uint16)
    if t == "bf16":
        return bf16_bits(v)
    raise ValueError(t)


def maps(seed, W, H, pixels=None, every=5):
    """The standard (dark, gain) float32 maps of an H x W frame.  pixels: an (H, W) image; every `every`-th pixel of
    the maps' raster (offset by the seed) gets dark == that pixel, so that p - D is exactly 0 there and the product's
    sign is the gain's (+0 and -0 both occur)."""
    rng = np.random.default_rng(seed)
    dark = rng.uniform(0.0, 300.0, (H, W)).astype(np.float32)
    dark = np.minimum(dark, np.float32(299.99997))   # (the cast can round up to 300.0)
    u = rng.uniform(-8.0, 8.0, (H, W))
    sign = np.where(rng.integers(0, 2, (H, W)) == 1, 1.0, -1.0)
    gain = (sign * np.exp2(u)).astype(np.float32)
    if pixels is not None:
        flat = dark.reshape(-1)
        idx = np.arange(seed % every, flat.size, every)
        flat[idx] = np.asarray(pixels).reshape(-1)[idx].astype(np.float32)
    return dark, gain


def window(a, x, y, rw, rh):
    """The window of an (..., H, W) array."""
    return a[..., y:y + rh, x:x + rw]


def clamp_origins(origins, W, H, rw, rh):
    """Per-frame (x, y) clamped into [0, W-rw] x [0, H-rh], as dbde_hip_decode_roi clamps them."""
    o = np.asarray(origins, np.int64).reshape(-1, 2)
    return np.stack([np.clip(o[:, 0], 0, W - rw), np.clip(o[:, 1], 0, H - rh)], axis=1)


def expected(images, x, y, rw, rh, dark, gain, t, origins=None):
    """Bit patterns (n, rh, rw) for images (n, H, W); dark / gain: (H, W) maps or scalars; origins: optional per-frame
    (x, y), clamped here.  The maps are taken at the (clamped) FRAME coordinates of every pixel."""
    images = np.asarray(images)
    n, H, W = images.shape
    if origins is None:
        org = np.tile(np.array([[x, y]], np.int64), (n, 1))
    else:
        org = clamp_origins(origins, W, H, rw, rh)
    out = np.empty((n, rh, rw), BITS[t])
    for f in range(n):
        fx, fy = int(org[f, 0]), int(org[f, 1])
        d = window(dark, fx, fy, rw, rh) if np.ndim(dark) == 2 else np.float32(dark)
        g = window(gain, fx, fy, rw, rh) if np.ndim(gain) == 2 else np.float32(gain)
        out[f] = scaled_bits(window(images[f], fx, fy, rw, rh), d, g, t)
    return out
