"""The scaled float decode's contract in exact integer arithmetic, the wrong kernels a plausible change would produce,
and a witness set that tells them apart (helper; no test of its own).

exact_bits(p, D, G, t) is the definition: D and G are binary32 BIT PATTERNS taken at their exact values, (float)p - D
and then * G are each rounded to nearest even to binary32 (gradual underflow, overflow to inf, IEEE signs of zero), and
the result is rounded to nearest even to F32 / F16 / BF16.  Only Python integers are used: no float32, float16 or
bfloat16 operation of numpy or torch.  NaN is out of scope (ValueError).  tests/scaled_ref.py and torch are checked
against it (tests/test_scaled_witness.py).

MUTANTS are functions of the same signature built on the same arithmetic, each wrong in one plausible way.

witnesses(pix) is a deterministic list of operands (p, D bits, G bits), each tagged with a category, an output type,
the pixel size and the sign of its result; is_category() is the category's definition in terms of the exact reference
alone.  Ties and edges are constructed (a power-of-two gain and a dark value of few bits that put a chosen binary32
value out); double roundings are found by a numpy search over the standard maps' distribution, and every candidate of
either kind is kept only if is_category() says so.  scalar_witnesses(pix) are (D0, G0) pairs with the pixel values for
which each is a witness: the kernel's scalar operands are another code path than its map loads.

cases(pix), witness_index() and sites() lay the witnesses out for tests/test_gpu_scaled_witness.py and restate the
kernel's partition of the output (decode_scaled_kernel, step 4): one range per (frame, window tile row, piece), cut
into aligned 16-byte blocks by the output's address; a whole block inside one window row is site A (vector map loads,
packed conversion), a whole block that a window row ends in is site B (element loads, packed conversion), the first and
last partial block of a range are site C (scalar conversion).
"""
import collections
import functools
import math
import random
import struct

import numpy as np

TYPES = ("f32", "f16", "bf16")
FMT = {"f32": (8, 23), "f16": (5, 10), "bf16": (8, 7)}   # exponent bits, stored mantissa bits
F32 = FMT["f32"]
SIGN32, MAG32, EXP32 = 0x80000000, 0x7FFFFFFF, 0x7F800000


# ---- exact arithmetic on (s, m, e): the value (-1)^s * m * 2^e, m a non-negative int; m None is infinity ----

def unpack32(b):
    s, ex, fr = b >> 31, (b >> 23) & 0xFF, b & 0x7FFFFF
    if ex == 255:
        if fr:
            raise ValueError("NaN is out of scope")
        return s, None, 0
    return (s, fr, -149) if ex == 0 else (s, fr | 0x800000, ex - 150)


def split(m, e, fmt):
    """m * 2^e (m > 0) against fmt's grid -> (mant, field, state): the truncated significand, the exponent field less
    one (0 in the subnormal range), and what was cut off: 0 nothing, 1 below half, 2 exactly half, 3 above half."""
    eb, mb = fmt
    emin = 2 - (1 << (eb - 1))
    E = max(m.bit_length() - 1 + e, emin)
    sh = E - mb - e
    if sh <= 0:
        return m << -sh, E - emin, 0
    rem, half = m & ((1 << sh) - 1), 1 << (sh - 1)
    return m >> sh, E - emin, 0 if rem == 0 else (1 if rem < half else (2 if rem == half else 3))


def pack(s, m, e, fmt, mode="even"):
    """(-1)^s * m * 2^e rounded into fmt -> bits.  mode: "even" (the contract), "away" (ties away), "trunc"."""
    eb, mb = fmt
    top, sign = ((1 << eb) - 1) << mb, s << (eb + mb)
    if m is None:
        return sign | top
    if m == 0:
        return sign
    mant, field, state = split(m, e, fmt)
    if mode == "even":
        mant += state == 3 or (state == 2 and mant & 1)
    elif mode == "away":
        mant += state >= 2
    r = mant + (field << mb)   # the hidden bit carries into the exponent field; so does a rounding carry
    if r >= top:
        r = top - 1 if mode == "trunc" else top
    return sign | r


def is_tie(b32, t):
    """The finite binary32 value lies exactly halfway between two neighbours of type t."""
    s, m, e = unpack32(b32)
    return bool(m) and split(m, e, FMT[t])[2] == 2


def neg(v):
    return v[0] ^ 1, v[1], v[2]


def add(a, b):
    (sa, ma, ea), (sb, mb, eb) = a, b
    if ma is None or mb is None:
        if ma is None and mb is None and sa != sb:
            raise ValueError("inf - inf is NaN: out of scope")
        return a if ma is None else b
    e = min(ea, eb)
    M = (-1) ** sa * (ma << (ea - e)) + (-1) ** sb * (mb << (eb - e))
    if M == 0:
        return (sa if sa == sb else 0), 0, e   # x - x = +0; (-0) + (-0) = -0
    return int(M < 0), abs(M), e


def mul(a, b):
    (sa, ma, ea), (sb, mb, eb) = a, b
    if ma is None or mb is None:
        if ma == 0 or mb == 0:
            raise ValueError("0 * inf is NaN: out of scope")
        return sa ^ sb, None, 0
    return sa ^ sb, ma * mb, ea + eb


def subnormal32(b):
    return (b & EXP32) == 0 and (b & MAG32) != 0


def _r32(v, ftz=False):
    b = pack(*v, F32)
    return b & SIGN32 if ftz and subnormal32(b) else b


def stages(p, D, G):
    """The contract's binary32 intermediates: (difference bits, the exact product (s, m, e), product bits)."""
    d = _r32(add((0, int(p), 0), neg(unpack32(D))))
    P = mul(unpack32(d), unpack32(G))
    return d, P, _r32(P)


QNAN = {"f32": 0x7FC00000, "f16": 0x7E00, "bf16": 0x7FC0}


def evaluate(p, D, G, t, how=None):
    """exact_bits (how None) or the mutant named how.  A mutant that meets inf - inf where the contract has a number
    returns a quiet NaN."""
    try:
        return _evaluate(p, D, G, t, how)
    except ValueError:
        if how is None:
            raise
        return QNAN[t]


def _evaluate(p, D, G, t, how):
    p, D, G = int(p), int(D), int(G)
    if how == "ftz_in":
        D, G = (D & SIGN32 if subnormal32(D) else D), (G & SIGN32 if subnormal32(G) else G)
    ftz = how == "ftz_out"
    d_, g_ = unpack32(D), unpack32(G)
    if how == "distributed":
        a, b = _r32(mul((0, p, 0), g_)), _r32(mul(d_, g_))
        v = _r32(add(unpack32(a), neg(unpack32(b))))
    elif how == "fma":
        v = _r32(add(unpack32(_r32(mul((0, p, 0), g_))), mul(neg(d_), g_)))
    else:
        if how == "reversed":   # (D - p) * (-G): the same value, another zero
            d, g_ = _r32(add(d_, (1, p, 0))), neg(g_)
        else:
            d = _r32(add((0, p, 0), neg(d_)), ftz)
        P = mul(unpack32(d), g_)
        if how == "fused" and t != "f32":
            return pack(*P, FMT[t])
        v = _r32(P, ftz)
    if how == "ftz_cvt" and t != "f32" and subnormal32(v):
        v &= SIGN32
    eb, mb = FMT[t]
    inf = ((1 << eb) - 1) << mb
    if t == "f32":
        r = v
    elif how == "early_inf" and EXP32 > (v & MAG32) > {"f16": 0x477FE000, "bf16": 0x7F7F0000}[t]:
        r = (v >> 16 & 0x8000) | inf
    else:
        r = pack(*unpack32(v), FMT[t], {"ties_away": "away", "truncate": "trunc"}.get(how, "even"))
        if how == "flush_half" and r & 0x7FFF and not r & (((1 << eb) - 1) << mb):
            r &= 0x8000
    if how == "saturate" and r & ~(1 << (eb + mb)) == inf:
        r -= 1
    if how == "positive_zero" and not r & (MAG32 if t == "f32" else 0x7FFF):
        r = 0
    return r


def exact_bits(p, D, G, t):
    """The contract: bits of ((float)p - D) * G in type t; D, G: binary32 bit patterns."""
    return evaluate(p, D, G, t)


MUTANT_TYPES = {   # the output types in which each mutant can differ from the contract
    "fused": ("f16", "bf16"), "distributed": TYPES, "fma": TYPES, "ftz_in": TYPES, "ftz_out": TYPES,
    "ftz_cvt": ("bf16",),     # (a subnormal binary32 value converts to an F16 zero either way)
    "flush_half": ("f16", "bf16"), "ties_away": ("f16", "bf16"), "truncate": ("f16", "bf16"), "positive_zero": TYPES,
    # three more, for the categories that none of the above can tell from the contract
    "saturate": TYPES,               # an overflow written as the largest finite value
    "early_inf": ("f16", "bf16"),    # the conversion overflows whatever exceeds the largest finite value, before rounding
    "reversed": TYPES}               # (D - p) * (-G): x - x = +0 meets the other sign of the gain
MUTANTS = {name: functools.partial(evaluate, how=name) for name in MUTANT_TYPES}


def exact_array(p, D, G, t):
    """exact_bits over arrays (p integers; D, G float32 arrays or uint32 bit patterns), element by element."""
    p = np.asarray(p)
    Db, Gb = (np.ascontiguousarray(np.broadcast_to(a, p.shape)) for a in (D, G))
    Db, Gb = (a.view(np.uint32) if a.dtype == np.float32 else a for a in (Db, Gb))
    out = [evaluate(a, b, c, t) for a, b, c in zip(p.reshape(-1).tolist(), Db.reshape(-1).tolist(), Gb.reshape(-1).tolist())]
    return np.array(out, np.uint32 if t == "f32" else np.uint16).reshape(p.shape)


def f32_of(bits):
    """The binary32 bit pattern as a Python float (exact)."""
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def bits_exactly(s, m, e):
    """The binary32 bits of (-1)^s * m * 2^e, or None where binary32 has no such value."""
    if m is None:
        return None
    b = pack(s, m, e, F32)
    if (b & MAG32) >= EXP32:
        return None
    _, m2, e2 = unpack32(b)
    lo = min(e, e2)
    return b if (m << (e - lo)) == (m2 << (e2 - lo)) else None


# ---- categories ----------------------------------------------------------------------------------------------

HALF = ("f16", "bf16")
CATEGORIES = {   # category -> (output types it applies to, pixel sizes)
    "tie_even": (HALF, (8, 16)), "tie_odd": (HALF, (8, 16)),
    "tie_plus_ulp": (HALF, (8, 16)), "tie_minus_ulp": (HALF, (8, 16)),
    "double_round_up": (HALF, (8, 16)), "double_round_down": (HALF, (8, 16)),
    "sub_rounds": (TYPES, (8, 16)),
    "f16_max": (("f16",), (8, 16)), "f16_to_inf": (("f16",), (8, 16)),
    "bf16_max": (("bf16",), (8, 16)), "bf16_to_inf": (("bf16",), (8, 16)),
    "f32_to_inf": (TYPES, (8, 16)), "f32_max": (TYPES, (8, 16)),
    "half_subnormal": (("f16",), (8, 16)),
    "f32_subnormal_in": (TYPES, (8, 16)), "f32_subnormal_out": (TYPES, (8, 16)),
    "subnormal_times_large": (TYPES, (8, 16)), "bf16_subnormal": (("bf16",), (8, 16)),
    "zero_pos": (TYPES, (8, 16)), "zero_neg": (TYPES, (8, 16)),
    "underflow_to_zero": (TYPES, (8, 16)),
    "int_tie": (HALF, (16,)),   # plain pixels with D = 0 and G = +-1: 2049, 2051 (F16); 257, 259 (BF16)
}
SUBNORMAL_CATEGORIES = ("f32_subnormal_in", "f32_subnormal_out", "subnormal_times_large", "bf16_subnormal",
                        "underflow_to_zero")   # a binary32 operand or intermediate is subnormal, or the product underflows
MIN_PER_CELL = 4

Witness = collections.namedtuple("Witness", "p D G cat t pix sign")


def _finite(b):
    return (b & MAG32) < EXP32


def is_category(cat, p, D, G, t, pix):
    """Whether (p, D, G) is a witness of cat for output type t, judged by the exact arithmetic alone."""
    if not (0 <= p < (1 << pix)) or not _finite(D) or not _finite(G) or t not in CATEGORIES[cat][0]:
        return False
    d, P, v = stages(p, D, G)
    mag, out = v & MAG32, evaluate(p, D, G, t)
    omag = out & (MAG32 if t == "f32" else 0x7FFF)
    inexact = P[1] is not None and bits_exactly(*P) != v
    if cat in ("tie_even", "tie_odd"):
        if not (_finite(v) and is_tie(v, t)):
            return False
        return (split(*unpack32(v)[1:], FMT[t])[0] & 1) == (cat == "tie_odd")
    if cat == "tie_plus_ulp":
        return 0 < mag - 1 and _finite(v) and is_tie((v & SIGN32) | (mag - 1), t)
    if cat == "tie_minus_ulp":
        return mag > 0 and mag + 1 < EXP32 and is_tie((v & SIGN32) | (mag + 1), t)
    if cat in ("double_round_up", "double_round_down"):
        if not (inexact and _finite(v) and is_tie(v, t)) or split(P[1], P[2], FMT[t])[2] == 2:
            return False
        if evaluate(p, D, G, t, "fused") == out:
            return False
        _, mv, ev = unpack32(v)
        lo = min(ev, P[2])
        return ((mv << (ev - lo)) > (P[1] << (P[2] - lo))) == (cat == "double_round_up")
    if cat == "sub_rounds":
        s, m, e = add((0, p, 0), neg(unpack32(D)))
        return bits_exactly(s, m, e) != d and any(evaluate(p, D, G, t, h) != out for h in ("distributed", "fma"))
    if cat == "f16_max":
        return omag == 0x7BFF and mag >= 0x477FE000
    if cat == "f16_to_inf":
        return omag == 0x7C00 and 0x477FF000 <= mag <= 0x47800000
    if cat == "bf16_max":
        return omag == 0x7F7F and mag >= 0x7F7F0000
    if cat == "bf16_to_inf":
        return omag == 0x7F80 and _finite(v)
    if cat == "f32_to_inf":
        return mag == EXP32
    if cat == "f32_max":
        return mag == 0x7F7FFFFF
    if cat == "half_subnormal":
        return 0 < mag < 0x38800000 and mag >= 0x32000000   # [2^-27, 2^-14): F16 subnormals and what rounds to +-0
    if cat == "f32_subnormal_in":
        return (subnormal32(D) and p == 0) or subnormal32(G)
    if cat == "f32_subnormal_out":
        return not subnormal32(D) and not subnormal32(G) and not subnormal32(d) and inexact and subnormal32(v)
    if cat == "subnormal_times_large":
        return subnormal32(d) and mag >= 0x00800000 and _finite(v)
    if cat == "bf16_subnormal":
        return subnormal32(v) and 0 < omag < 0x0080
    if cat in ("zero_pos", "zero_neg"):
        return (d & MAG32) == 0 and (G & MAG32) != 0 and out == (0 if cat == "zero_pos" else (SIGN32 if t == "f32" else 0x8000))
    if cat == "underflow_to_zero":
        if (d & MAG32) == 0 or (G & MAG32) == 0 or mag != 0:
            return False
        return P[1].bit_length() - 1 + P[2] < -150
    if cat == "int_tie":
        return pix == 16 and D == 0 and (G & MAG32) == 0x3F800000 and is_tie(v, t) and p < 4096
    raise KeyError(cat)


def result_sign(p, D, G, t):
    return evaluate(p, D, G, t) >> (31 if t == "f32" else 15)


# ---- the generator ---------------------------------------------------------------------------------------------

def _solve(v, pix, rng, ps=()):
    """Operands whose contract value in binary32 is exactly the bit pattern v: G = +-2^k, d = v / G, D = p - d with
    p near |d| (or one of ps), kept where D is a binary32 value.  None if 64 draws find none."""
    s, m, e = unpack32(v)
    top = (1 << pix) - 1
    E = m.bit_length() - 1 + e
    for _ in range(64):
        k = min(127, max(-126, E - rng.randrange(-3, pix)))
        sg = rng.randrange(2)
        d = (s ^ sg, m, e - k)
        near = (m << (e - k)) if e - k >= 0 else (m >> (k - e))
        p = rng.choice(ps) if ps and rng.randrange(2) else min(top, max(0, near + rng.randrange(-2, 3)))
        D = bits_exactly(*add((0, p, 0), neg(d)))
        G = pack(sg, 1, k, F32)
        if D is not None and stages(p, D, G)[2] == v:
            return p, D, G
    return None


def _tie32(t, rng, odd):
    """A binary32 value halfway between two normal neighbours of type t; odd: the lower one's last bit."""
    eb, mb = FMT[t]
    M = (1 << mb) | (rng.randrange(1 << mb) & ~1) | int(odd)
    field = rng.randrange(1, (1 << eb) - 2) if t == "f16" else rng.randrange(90, 170)
    return pack(rng.randrange(2), 2 * M + 1, field - ((1 << (eb - 1)) - 1) - mb - 1, F32)


def _rand_mant(rng):
    return 0x800000 | rng.randrange(1 << 23)


def _candidates(cat, t, pix, rng):
    """An endless stream of (p, D, G) candidates for the cell; is_category() decides."""
    top = (1 << pix) - 1
    edge_p = (0, 255, top)
    sgn = lambda: rng.randrange(2)   # noqa: E731
    while True:
        got = None
        if cat in ("tie_even", "tie_odd"):
            got = _solve(_tie32(t, rng, cat == "tie_odd"), pix, rng, edge_p)
        elif cat in ("tie_plus_ulp", "tie_minus_ulp"):
            got = _solve(_tie32(t, rng, rng.randrange(2)) + (1 if cat == "tie_plus_ulp" else -1), pix, rng, edge_p)
        elif cat == "sub_rounds" and t != "f32":   # draws whose last binary32 bit decides the rounding
            pool = _search_sub(pix, t)
            got = pool[rng.randrange(len(pool))]
        elif cat == "sub_rounds":
            got = (rng.randrange(top + 1), pack(0, _rand_mant(rng), rng.randrange(-30, -15), F32),
                   pack(sgn(), _rand_mant(rng), rng.randrange(-31, -15), F32))
        elif cat in ("f16_max", "f16_to_inf", "bf16_max", "bf16_to_inf", "f32_max", "half_subnormal", "bf16_subnormal"):
            lo, hi = {"f16_max": (0x477FE000, 0x477FEFFF), "f16_to_inf": (0x477FF000, 0x47800000),
                      "bf16_max": (0x7F7F0000, 0x7F7F7FFF), "bf16_to_inf": (0x7F7F8000, 0x7F7FFFFF),
                      "f32_max": (0x7F7FFFFF, 0x7F7FFFFF), "half_subnormal": (0x32000000, 0x387FFFFF),
                      "bf16_subnormal": (0x00004001, 0x007FBFFF)}[cat]
            v = rng.choice((lo, hi, rng.randrange(lo, hi + 1), rng.randrange(lo, hi + 1)))
            got = _solve(v | (sgn() << 31), pix, rng, edge_p)
        elif cat == "f32_to_inf":
            p = rng.choice((top, 255, rng.randrange(1, top + 1)))
            got = (p, pack(sgn(), _rand_mant(rng), -30, F32), pack(sgn(), _rand_mant(rng), 128 - 23 - p.bit_length() + rng.randrange(1, 3), F32))
        elif cat in ("f32_subnormal_in", "subnormal_times_large"):
            if cat == "f32_subnormal_in" and rng.randrange(2):   # a subnormal gain
                got = (rng.choice((top, 255, rng.randrange(top + 1))), pack(0, _rand_mant(rng), -20, F32),
                       (sgn() << 31) | rng.randrange(1, 0x800000))
            else:                                                  # a subnormal dark value under p = 0
                got = (0, (sgn() << 31) | rng.randrange(1, 0x800000), pack(sgn(), _rand_mant(rng), rng.randrange(10, 104), F32))
        elif cat == "f32_subnormal_out":
            if rng.randrange(2):   # d = 1/2 under the largest pixels
                p = rng.choice((top, 255))
                got = (p, bits_exactly(0, 2 * p - 1, -1), pack(sgn(), _rand_mant(rng) | 1, -149, F32))
            else:
                a = rng.randrange(1, 40)
                got = (0, pack(sgn(), _rand_mant(rng), -23 - a, F32), pack(sgn(), _rand_mant(rng) | 1, -23 - rng.randrange(127, 147) + a, F32))
        elif cat in ("zero_pos", "zero_neg"):
            p = rng.choice(edge_p + (rng.randrange(top + 1),))
            got = (p, bits_exactly(0, p, 0), pack(int(cat == "zero_neg"), _rand_mant(rng), rng.randrange(-40, 0), F32))
        elif cat == "underflow_to_zero":
            if rng.randrange(4) == 0:   # d = 2^-24 under p = 1
                got = (1, 0x3F7FFFFF, pack(sgn(), _rand_mant(rng), -23 - rng.randrange(127, 130), F32))
            else:
                a = rng.randrange(25, 60)
                got = (0, pack(sgn(), _rand_mant(rng), -23 - a, F32), pack(sgn(), _rand_mant(rng), -23 - rng.randrange(152 - a, 180 - a), F32))
        if got is not None and got[1] is not None:
            yield got


FIXED = {   # operands that the set must hold, whatever the draws: (cat, t, pix) -> [(p, D, G)]
    ("f16_max", "f16", 16): [(65504, 0, 0x3F800000), (65519, 0, 0x3F800000), (65519, 0, 0xBF800000)],
    ("f16_to_inf", "f16", 16): [(65520, 0, 0x3F800000), (65535, 0, 0x3F800000), (65520, 0, 0xBF800000), (65535, 0, 0xBF800000)],
    ("int_tie", "f16", 16): [(2049, 0, 0x3F800000), (2051, 0, 0x3F800000), (2049, 0, 0xBF800000), (2051, 0, 0xBF800000)],
    ("int_tie", "bf16", 16): [(257, 0, 0x3F800000), (259, 0, 0x3F800000), (257, 0, 0xBF800000), (259, 0, 0xBF800000)],
}
FIXED_VALUES = {   # binary32 values that must come out, in both signs: (cat, t) -> [bits]
    ("f16_max", "f16"): [0x477FE000, 0x477FEFFF], ("f16_to_inf", "f16"): [0x477FF000],
    ("bf16_max", "bf16"): [0x7F7F7FFF], ("bf16_to_inf", "bf16"): [0x7F7F8000],
    ("half_subnormal", "f16"): [0x33000000, 0x33000001, 0x33C00000],   # 2^-25 -> 0, just above -> 2^-24, 1.5 * 2^-24 -> 2^-23
}
SEARCH = 1 << 22        # samples of the double-rounding search
SEARCH_KEEP = 6         # found witnesses kept per (category, type, sign)


@functools.lru_cache(maxsize=None)
def _search_ties(pix):
    """Operands drawn as tests/scaled_ref.py's standard maps draw them whose product is inexact in binary32 and rounds
    onto an F16 or BF16 tie, or one binary32 ulp beside one -> {(kind, type): [(p, D, G)]}, kind "tie", "plus" or
    "minus", in the order found.  (numpy finds candidates; is_category() judges them.)"""
    rng = np.random.default_rng(0x5CA1ED + pix)
    p = rng.integers(0, 1 << pix, SEARCH).astype(np.float64)
    if pix == 16:
        p[::2] = rng.integers(0, 320, SEARCH // 2)
    D = np.minimum(rng.uniform(0.0, 300.0, SEARCH).astype(np.float32), np.float32(299.99997))
    G = (np.where(rng.integers(0, 2, SEARCH) == 1, 1.0, -1.0) * np.exp2(rng.uniform(-8.0, 8.0, SEARCH))).astype(np.float32)
    d = (p - D.astype(np.float64)).astype(np.float32)
    P = d.astype(np.float64) * G.astype(np.float64)   # exact: 24 x 24 bits
    v = P.astype(np.float32)
    b = v.view(np.uint32)
    inexact = v.astype(np.float64) != P
    ex = (b >> 23) & 0xFF
    ok = {"f16": inexact & (ex >= 113) & (ex <= 142), "bf16": inexact & (ex >= 1) & (ex <= 254)}
    low = {"f16": b & 0x1FFF, "bf16": b & 0xFFFF}
    half = {"f16": 0x1000, "bf16": 0x8000}
    Db, Gb = D.view(np.uint32), G.view(np.uint32)
    out = {}
    for t in HALF:
        for kind, off in (("tie", 0), ("plus", 1), ("minus", -1)):
            idx = np.flatnonzero(ok[t] & (low[t] == half[t] + off))[:600]
            out[kind, t] = [(int(p[i]), int(Db[i]), int(Gb[i])) for i in idx]
    return out


@functools.lru_cache(maxsize=None)
def _search_sub(pix, t):
    """Operands with a dark value below 2 (so that p - D is inexact for most p) for which p * G - D * G, each step
    rounded, gives another F16 / BF16 value than the contract -> [(p, D, G)].  (numpy finds; is_category() judges.)"""
    n = SEARCH // 2
    rng = np.random.default_rng(0x5B + pix + len(t))
    p = rng.integers(1, 1 << pix, n).astype(np.float64)
    D = rng.uniform(0.0, 2.0, n).astype(np.float32).astype(np.float64)
    G = (np.where(rng.integers(0, 2, n) == 1, 1.0, -1.0) * np.exp2(rng.uniform(-8.0, 8.0, n))).astype(np.float32).astype(np.float64)
    f = lambda a: a.astype(np.float32).astype(np.float64)   # noqa: E731
    v = f(f(p - D) * G).astype(np.float32).view(np.uint32)
    w = f(f(p * G) - f(D * G)).astype(np.float32).view(np.uint32)
    sh, half = (13, 0xFFF) if t == "f16" else (16, 0x7FFF)
    rnd = lambda b: (b.astype(np.uint64) + half + ((b >> sh) & 1)) >> sh   # noqa: E731
    idx = np.flatnonzero(rnd(v) != rnd(w))[:200]
    Db, Gb = D.astype(np.float32).view(np.uint32), G.astype(np.float32).view(np.uint32)
    return [(int(p[i]), int(Db[i]), int(Gb[i])) for i in idx]


def told_apart(p, D, G, t):
    """The mutants whose result for these operands differs from the contract's."""
    want = evaluate(p, D, G, t)
    return [m for m, types in MUTANT_TYPES.items() if t in types and evaluate(p, D, G, t, m) != want]


@functools.lru_cache(maxsize=None)
def witnesses(pix):
    """The witness list of one pixel size (8 or 16): deterministic; its length is coprime to 2 * 3 * 5 * 7 * 11, so
    that a stride through it meets every 16-byte slot and every row of the test frames' widths."""
    out, seen = [], set()

    def take(p, D, G, cat, t):
        if (p, D, G, cat, t) in seen or not is_category(cat, p, D, G, t, pix):
            return False
        seen.add((p, D, G, cat, t))
        out.append(Witness(p, D, G, cat, t, pix, result_sign(p, D, G, t)))
        return True

    found = _search_ties(pix)
    for cat, (types, sizes) in CATEGORIES.items():
        if pix not in sizes:
            continue
        for t in types:
            rng = random.Random(f"{cat} {t} {pix}")
            have = {0: 0, 1: 0}
            if cat in ("zero_pos", "zero_neg"):   # one sign only
                have = {int(cat == "zero_neg"): 0}
            for p, D, G in FIXED.get((cat, t, pix), ()):
                assert take(p, D, G, cat, t), (cat, t, p, D, G)
                have[out[-1].sign] += 1
            for v in FIXED_VALUES.get((cat, t), ()):
                for s in (0, SIGN32):
                    for _ in range(8):
                        got = _solve(v | s, pix, rng)
                        if got and take(*got, cat, t):
                            have[out[-1].sign] += 1
                            break
                    else:
                        raise AssertionError(f"no operands for {v | s:#x} ({cat} {t} {pix})")
            if cat.startswith("double_round"):
                for p, D, G in found["tie", t]:
                    s = result_sign(p, D, G, t)
                    if have[s] < SEARCH_KEEP and take(p, D, G, cat, t):
                        have[s] += 1
                continue
            if cat == "int_tie":
                continue
            if cat in ("tie_plus_ulp", "tie_minus_ulp"):   # from the standard maps: those a mutant's last bit moves over the tie
                n = 0
                for p, D, G in found[cat[4:-4], t]:
                    if n < 2 and told_apart(p, D, G, t) and take(p, D, G, cat, t):
                        n += 1
                        have[out[-1].sign] += 1
            want = MIN_PER_CELL // len(have) + (1 if cat in ("tie_even", "tie_odd") else 0)
            stream = _candidates(cat, t, pix, rng)
            for _ in range(4000):
                if min(have.values()) >= want:
                    break
                p, D, G = next(stream)
                if _finite(D) and _finite(G):
                    try:
                        s = result_sign(p, D, G, t)
                    except ValueError:
                        continue
                    if have.get(s, want) < want and take(p, D, G, cat, t):
                        have[s] += 1
    for t in HALF:   # ties that the search met without a double rounding: the standard maps' own
        n = 0
        for p, D, G in found["tie", t]:
            for cat in ("tie_even", "tie_odd"):
                if n < 8 and take(p, D, G, cat, t):
                    n += 1
    rng = random.Random(f"pad {pix}")
    while math.gcd(len(out), 2310) != 1:   # pad with zeros of either sign
        cat = ("zero_pos", "zero_neg")[len(out) & 1]
        p, D, G = next(_candidates(cat, "f32", pix, rng))
        take(p, D, G, cat, "f32")
    return tuple(out)


def stride(K):
    """The raster stride through K witnesses: coprime to K, and far from 1 so that neighbours differ."""
    s = 89
    while math.gcd(s, K) != 1:
        s += 2
    return s


ScalarWitness = collections.namedtuple("ScalarWitness", "D0 G0 pix ps tags")   # tags[i]: (cat, t) of ps[i], or None


def _b(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


@functools.lru_cache(maxsize=None)
def scalar_witnesses(pix):
    """(D0, G0) pairs and the pixel values for which each is a witness; every ps has 11 entries (coprime to the test
    frames' widths), filled up with other pixel values (tag None)."""
    top = (1 << pix) - 1
    sub = 0x00234567
    pairs = [   # D0, G0, candidate pixels, categories to try
        (_b(1 / 32), _b(16.0), range(64, 128), ("tie_odd",)),        # p - 1/32: 12 bits, the F16 tie above an odd value
        (_b(3 / 32), _b(-0.25), range(64, 128), ("tie_even",)),
        (_b(0.25), _b(-2.0 ** 100), range(64, 128), ("tie_odd",)),   # p - 1/4: 9 bits, a BF16 tie
        (_b(0.75), _b(2.0 ** -100), range(64, 128), ("tie_even",)),
        (sub, _b(2.0 ** 120), (0,), ("f32_subnormal_in", "subnormal_times_large")),
        (_b(7.0), _b(-2.5), (7,), ("zero_neg",)),
        (_b(0.0), 0x80000123, (top, 255, 1), ("f32_subnormal_in", "bf16_subnormal")),
        (_b(0.5), _b(2.0 ** 127), (top, 255, 3), ("f32_to_inf", "bf16_to_inf")),
    ]
    if pix == 16:
        pairs.append((0, _b(1.0), (2049, 2051, 257, 259, 65504, 65519, 65520, 65535), ("int_tie", "f16_max", "f16_to_inf")))
        pairs.append((0, _b(-1.0), (2049, 2051, 257, 259, 65519, 65520, 65535), ("int_tie", "f16_max", "f16_to_inf")))
    out = []
    for D0, G0, cand, cats in pairs:
        ps, tags = [], []
        for p in cand:
            tag = next(((c, t) for c in cats for t in CATEGORIES[c][0] if is_category(c, p, D0, G0, t, pix)), None)
            if tag and len(ps) < 9:
                ps.append(p)
                tags.append(tag)
        assert ps, (D0, G0)
        fill = [0, top, 255, 1, 128, 77, 200, 13, 101, 64]
        while len(ps) < 11:
            ps.append(fill.pop(0))
            tags.append(None)
        out.append(ScalarWitness(D0, G0, pix, tuple(ps), tuple(tags)))
    return tuple(out)


# ---- layout: which witness sits where, and which arithmetic site of the kernel evaluates it -------------------------

Case = collections.namedtuple("Case", "name W H n win origins")   # origins: None, or n per-frame (x, y) (clamped by the call)
RESIDUE = 1      # elements between a 16-byte boundary and the outputs of the GPU test (test_gpu_scaled.Out, odd=1)
SITES = "ABC"


def cases(pix):
    """The calls of the GPU witness test for one pixel size."""
    W, H = 200, 123
    out = [Case("narrow full", W, H, 3, (0, 0, W, H), None),
           Case("narrow interior", W, H, 3, (13, 7, 150, 101), None)]
    for rw, x in ((1, 199), (1, 46), (1, 100), (1, 17), (3, 77), (3, 162), (5, 120), (5, 9), (9, 31), (9, 150)):
        out.append(Case(f"narrow rw={rw} x={x}", W, H, 3, (x, 0, rw, H), None))
    org = [(-5, 500), (139, 86), (3, 5)] + [(11 * f % 140, 7 * f % 87) for f in range(3, 12)]
    out.append(Case("narrow origins", W, H, len(org), (0, 0, 61, 37), tuple(org)))
    out.append(Case("wide full", 600, 17, 3, (0, 0, 600, 17), None))
    org = [(f % 80, f // 80 % 9) for f in range(0, 720, 2)]
    out.append(Case("wide origins", 600, 17, len(org), (0, 0, 521, 9), tuple(org)))
    Wp = 2100 if pix == 8 else 1100
    out.append(Case("wide pieces", Wp, 9, 3, (0, 0, Wp, 9), None))
    return out


def scalar_cases(pix):
    """The calls that run the scalar witness pairs: the narrow and the wide instance, whole frames."""
    return [Case("scalar narrow", 200, 123, 3, (0, 0, 200, 123), None),
            Case("scalar narrow rw=3", 200, 123, 3, (77, 0, 3, 123), None),
            Case("scalar wide", 600, 17, 3, (0, 0, 600, 17), None),
            Case("scalar wide origins", 600, 17, 24, (0, 0, 521, 9), tuple((3 * f, f % 9) for f in range(24)))]


def origins_of(case):
    """The per-frame window origins of a case, clamped as the call clamps them -> (n, 2) ints."""
    x, y, rw, rh = case.win
    if case.origins is None:
        return np.tile(np.array([[x, y]], np.int64), (case.n, 1))
    o = np.asarray(case.origins, np.int64).reshape(case.n, 2)
    return np.stack([np.clip(o[:, 0], 0, case.W - rw), np.clip(o[:, 1], 0, case.H - rh)], 1)


def witness_index(case, K, s=None):
    """(H, W): the witness of every frame coordinate: raster position i holds witness (i * s) mod K."""
    s = stride(K) if s is None else s
    i = np.arange(case.W * case.H, dtype=np.int64).reshape(case.H, case.W)
    return (i * s) % K


def windowed(case, a):
    """The windows (n, rh, rw) of an (H, W) array at the case's origins."""
    _, _, rw, rh = case.win
    return np.stack([a[y:y + rh, x:x + rw] for x, y in origins_of(case).tolist()])


def sites(case, threads, es, residue=RESIDUE):
    """The kernel's partition of the case's output -> (site, slot), both (n, rh, rw) uint8: site 0 / 1 / 2 for A / B / C,
    slot the element's place in its 16-byte block.  threads: the plan's (tiles of a piece); es: bytes of an element;
    residue: elements between a 16-byte boundary and the output's first element."""
    _, _, rw, rh = case.win
    NE = 16 // es
    site = np.full((case.n, rh * rw), 255, np.uint8)
    slot = np.empty((case.n, rh * rw), np.uint8)
    for f, (x, y) in enumerate(origins_of(case).tolist()):
        tx_a, tx_b = x >> 3, (x + rw - 1) >> 3
        for ty in range(y >> 3, ((y + rh - 1) >> 3) + 1):
            r_lo, r_hi = max(8 * ty, y), min(8 * ty + 8, y + rh)
            for txp in range(tx_a, tx_b + 1, threads):
                nt = min(tx_b + 1 - txp, threads)
                c_lo, c_hi = max(8 * txp, x), min(8 * (txp + nt), x + rw)
                pw, nr = c_hi - c_lo, r_hi - r_lo
                whole = pw == rw
                for r0, ln in ([(r_lo, nr * pw)] if whole else [(r, pw) for r in range(r_lo, r_hi)]):
                    w0 = (r0 - y) * rw + (c_lo - x)               # the range's first element in the frame's window
                    g0 = residue + f * rw * rh + w0               # ... and in elements from the 16-byte boundary
                    a = g0 + np.arange(ln)
                    blk = a // NE
                    st = np.zeros(ln, np.uint8)
                    if whole:                                     # a window row ends inside the block
                        st[(blk * NE - g0) % pw + NE > pw] = 1
                    if g0 % NE:
                        st[blk == blk[0]] = 2
                    if (g0 + ln) % NE:
                        st[blk == blk[-1]] = 2
                    assert (site[f, w0:w0 + ln] == 255).all()
                    site[f, w0:w0 + ln] = st
                    slot[f, w0:w0 + ln] = a % NE
    assert (site != 255).all(), "the ranges cover the window"
    return site.reshape(case.n, rh, rw), slot.reshape(case.n, rh, rw)


def coverage(case_list, threads_of, index_of, K, es, residue=RESIDUE):
    """Which witness the kernel evaluates where, over the given calls -> {threads: (A, B, C)}: A (K, 16 / es) bool by
    block slot, B and C (K,) bool.  threads_of(case): the plan's threads; index_of(case): the (H, W) witness index."""
    out = {}
    for case in case_list:
        th = threads_of(case)
        A, B, C = out.setdefault(th, (np.zeros((K, 16 // es), bool), np.zeros(K, bool), np.zeros(K, bool)))
        site, slot = sites(case, th, es, residue)
        w = windowed(case, index_of(case))
        A[w[site == 0], slot[site == 0]] = True
        B[w[site == 1]] = True
        C[w[site == 2]] = True
    return out
