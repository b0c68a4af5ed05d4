"""CPU: tests/scaled_witness.py -- the scaled decode's exact reference, its mutants, the witness set and its layout.

The witness tags are true by the exact reference alone and the set has its counts; the exact reference, the numpy
definition (tests/scaled_ref.py) and torch on the CPU agree on the witnesses and on 2^16 random operands that reach
into the subnormal range; every mutant is told from the contract in every output type and pixel size it applies to, and
every category is hit by a mutant; and the calls of tests/test_gpu_scaled_witness.py put every witness at every
arithmetic site of every kernel instance, in every slot of a 16-byte block (pure arithmetic from the plans).
"""
import collections
import math
import os

import numpy as np
import pytest

import dbde_video_cpp_amd as dv
import scaled_ref as sr
import scaled_witness as sw
from test_scaled_ref import torch_bits

PIX = (8, 16)
PLAN = {8: dv.scaled_plan, 16: dv.scaled16_plan}


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(dv.LIB_PATH):
        dv.build()


def arrays(ws):
    p = np.array([w.p for w in ws], np.int64)
    D = np.array([w.D for w in ws], np.uint32).view(np.float32)
    G = np.array([w.G for w in ws], np.uint32).view(np.float32)
    return p, D, G


def test_exact_reference_on_known_values():
    one, mone = 0x3F800000, 0xBF800000
    b = sw._b
    assert sw.exact_bits(7, b(7.0), one, "f32") == 0 and sw.exact_bits(7, b(7.0), mone, "f32") == 0x80000000   # x - x = +0
    assert sw.exact_bits(0, 0, mone, "f16") == 0x8000 and sw.exact_bits(0, 0x80000000, one, "bf16") == 0       # 0 - (-0) = +0
    assert sw.exact_bits(3, b(0.5), b(2.0), "f32") == b(5.0)
    assert [sw.exact_bits(p, 0, one, "f16") for p in (2049, 2051, 65504, 65519, 65520, 65535)] == \
        [0x6800, 0x6802, 0x7BFF, 0x7BFF, 0x7C00, 0x7C00]
    assert [sw.exact_bits(p, 0, mone, "bf16") for p in (257, 259)] == [0xC380, 0xC382]
    # 2^-25 -> 0, the binary32 value above it -> 2^-24, 1.5 * 2^-24 -> 2^-23 (F16 subnormals)
    assert [sw.pack(*sw.unpack32(v), sw.FMT["f16"]) for v in (0x33000000, 0x33000001, 0x33C00000)] == [0, 1, 2]
    # BF16: the cases of test_scaled_ref.test_bf16_rounding_ties_to_even
    for v, want in ((0x3F808000, 0x3F80), (0x3F818000, 0x3F82), (0x3F808001, 0x3F81), (0x3F807FFF, 0x3F80),
                    (0xBF818000, 0xBF82), (0x7F7F8000, 0x7F80), (0x7F7F7FFF, 0x7F7F), (0x00008000, 0), (0x00018000, 2),
                    (0x80000000, 0x8000), (0x7F800000, 0x7F80)):
        assert sw.pack(*sw.unpack32(v), sw.FMT["bf16"]) == want
    # gradual underflow of the product, and its overflow
    assert sw.exact_bits(1, 0, 0x00000003, "f32") == 3 and sw.exact_bits(3, 0, 0x00000001, "bf16") == 0
    assert sw.exact_bits(0, b(0.5), 0x00800001, "f32") == 0x80400000          # (2^23 + 1) * 2^-150: the tie goes to even
    assert sw.exact_bits(0, b(0.5), 0x00800003, "f32") == 0x80400002
    assert sw.exact_bits(255, 0, b(2.0 ** 121), "f32") == 0x7F800000 and sw.exact_bits(255, 0, b(-2.0 ** 120), "f32") == 0xFF7F0000
    assert sw.exact_bits(1, 0x3F7FFFFF, b(2.0 ** -126), "f32") == 0           # 2^-150: the tie at half the smallest subnormal
    with pytest.raises(ValueError):
        sw.exact_bits(0, 0x7FC00000, one, "f32")


@pytest.mark.parametrize("pix", PIX)
def test_tags_are_true(pix):
    ws = sw.witnesses(pix)
    for w in ws:
        assert w.pix == pix and 0 <= w.p < 1 << pix and w.t in sw.CATEGORIES[w.cat][0] and pix in sw.CATEGORIES[w.cat][1]
        assert sw.is_category(w.cat, w.p, w.D, w.G, w.t, pix), w
        assert w.sign == sw.exact_bits(w.p, w.D, w.G, w.t) >> (31 if w.t == "f32" else 15), w
    for s in sw.scalar_witnesses(pix):
        assert len(s.ps) == 11 and any(s.tags)
        for p, tag in zip(s.ps, s.tags):
            assert 0 <= p < 1 << pix
            assert tag is None or sw.is_category(tag[0], p, s.D0, s.G0, tag[1], pix), (s, p)
    assert sw.witnesses.__wrapped__(pix) == ws, "the generator is deterministic"


@pytest.mark.parametrize("pix", PIX)
def test_counts_hold(pix):
    ws = sw.witnesses(pix)
    K = len(ws)
    assert 150 <= K <= 600 and math.gcd(K, 2 * 3 * 5 * 7 * 11) == 1 and math.gcd(sw.stride(K), K) == 1
    cells = collections.defaultdict(list)
    for w in ws:
        cells[w.cat, w.t].append(w)
    for cat, (types, sizes) in sw.CATEGORIES.items():
        for t in types if pix in sizes else ():
            got = cells[cat, t]
            assert len(got) >= sw.MIN_PER_CELL, (cat, t, pix, len(got))
            if cat not in ("zero_pos", "zero_neg"):   # (their sign is the category)
                assert {w.sign for w in got} == {0, 1}, (cat, t, pix)
    ps = {w.p for w in ws}
    assert {0, 255, (1 << pix) - 1} <= ps
    v32 = collections.defaultdict(set)
    for w in ws:
        v32[w.cat].add(sw.stages(w.p, w.D, w.G)[2] & sw.MAG32)
    assert {0x477FE000, 0x477FEFFF} <= v32["f16_max"] and 0x477FF000 in v32["f16_to_inf"]
    assert 0x7F7F7FFF in v32["bf16_max"] and 0x7F7F8000 in v32["bf16_to_inf"]
    assert {0x33000000, 0x33000001, 0x33C00000} <= v32["half_subnormal"]
    assert any(sw.subnormal32(w.D) and w.p == 0 for w in cells["f32_subnormal_in", "f32"])
    assert any(sw.subnormal32(w.G) for w in cells["f32_subnormal_in", "f32"])
    if pix == 16:
        plain = {(w.p, w.cat) for w in ws if w.D == 0 and w.G == 0x3F800000}
        assert {(65519, "f16_max"), (65520, "f16_to_inf"), (65535, "f16_to_inf"), (2049, "int_tie"), (2051, "int_tie"),
                (257, "int_tie"), (259, "int_tie")} <= plain
    pairs = sw.scalar_witnesses(pix)
    assert 4 <= len(pairs) <= 12
    tagged = {tag[0] for s in pairs for tag in s.tags if tag}
    assert {"tie_even", "tie_odd", "f32_subnormal_in", "zero_neg", "f32_to_inf"} <= tagged


def flushes(name, got, want, p, D, G, t):
    """The message of a disagreement with the exact reference: names a flush of subnormals where one explains it."""
    i = int(np.flatnonzero(got != want)[0])
    args = (int(p[i]), int(D.view(np.uint32)[i]), int(G.view(np.uint32)[i]), t)
    d, _, v = sw.stages(*args[:3])
    sub = any(sw.subnormal32(b) for b in (args[1], args[2], d, v))
    how = [m for m in ("ftz_in", "ftz_out", "ftz_cvt") if sw.evaluate(*args, m) == int(got[i])]
    msg = f"{name} differs from the exact reference at p={args[0]} D={args[1]:#x} G={args[2]:#x} {t}: " \
          f"{int(got[i]):#x} != {int(want[i]):#x} ({int((got != want).sum())} of {got.size})"
    if sub and how:
        msg += f": {name} FLUSHES SUBNORMALS on this host (as the mutant {how[0]} does)"
    return msg


def agree(p, D, G, want):
    for t in sw.TYPES:
        for name, got in (("numpy (scaled_ref.scaled_bits)", sr.scaled_bits(p, D, G, t)), ("torch on the CPU", torch_bits(p, D, G, t))):
            assert got.dtype == want[t].dtype
            assert np.array_equal(got, want[t]), flushes(name, got, want[t], p, D, G, t)


@pytest.mark.parametrize("pix", PIX)
def test_three_references_agree_on_the_witnesses(pix):
    p, D, G = arrays(sw.witnesses(pix))
    agree(p, D, G, {t: sw.exact_array(p, D, G, t) for t in sw.TYPES})


def random_operands(n):
    """n operand triples over the whole binary32 range: subnormal, tiny, ordinary and huge dark values and gains."""
    rng = np.random.default_rng(0xE5AC7)
    p = np.where(rng.integers(0, 2, n) == 1, rng.integers(0, 256, n), rng.integers(0, 65536, n))
    p[rng.integers(0, 4, n) == 0] = 0   # p = 0 lets a subnormal dark value through the subtraction
    sign = lambda: rng.integers(0, 2, n).astype(np.uint32) << 31   # noqa: E731
    frac = lambda: rng.integers(0, 1 << 23, n).astype(np.uint32)   # noqa: E731
    std = np.minimum(rng.uniform(0.0, 300.0, n).astype(np.float32), np.float32(299.99997)).view(np.uint32)
    kind = rng.integers(0, 4, n)
    D = np.select([kind == 0, kind == 1, kind == 2], [sign() | frac(), sign() | (rng.integers(1, 40, n).astype(np.uint32) << 23) | frac(), std],
                  sign() | (rng.integers(1, 150, n).astype(np.uint32) << 23) | frac())
    kind = rng.integers(0, 4, n)
    pow2 = rng.integers(119, 136, n).astype(np.uint32) << 23
    G = np.select([kind == 0, kind == 1], [sign() | frac(), sign() | pow2], sign() | (rng.integers(1, 255, n).astype(np.uint32) << 23) | frac())
    return p.astype(np.int64), D.astype(np.uint32).view(np.float32), G.astype(np.uint32).view(np.float32)


def test_three_references_agree_on_random_operands_with_subnormals():
    n = 1 << 16
    p, D, G = random_operands(n)
    Db, Gb = D.view(np.uint32).tolist(), G.view(np.uint32).tolist()
    v, sub_d, sub_v = np.empty(n, np.uint32), 0, 0
    for i, (a, b, c) in enumerate(zip(p.tolist(), Db, Gb)):
        d, _, v[i] = sw.stages(a, b, c)
        sub_d += sw.subnormal32(d)
        sub_v += sw.subnormal32(int(v[i]))
    assert sub_d > n // 64 and sub_v > n // 64, "the sample reaches subnormal differences and products"
    assert (np.isinf(v.view(np.float32))).sum() > n // 64 and not np.isnan(v.view(np.float32)).any()
    want = {"f32": v}
    for t in sw.HALF:
        want[t] = np.array([sw.pack(*sw.unpack32(b), sw.FMT[t]) for b in v.tolist()], np.uint16)
    sub16 = (want["bf16"] & 0x7F80) == 0
    assert ((want["bf16"][sub16] & 0x7F) != 0).sum() > n // 128, "BF16 subnormal results occur"
    agree(p, D, G, want)


@pytest.mark.parametrize("pix", PIX)
def test_every_mutant_is_told_apart_and_every_category_is_hit(pix):
    ws = sw.witnesses(pix)
    assert {"fused", "distributed", "fma", "ftz_in", "ftz_out", "ftz_cvt", "flush_half", "ties_away", "truncate",
            "positive_zero"} <= set(sw.MUTANTS)
    hit = collections.defaultdict(set)   # (mutant, type) -> categories
    for w in ws:
        want = sw.exact_bits(w.p, w.D, w.G, w.t)
        for m, fn in sw.MUTANTS.items():
            if w.t in sw.MUTANT_TYPES[m] and fn(w.p, w.D, w.G, w.t) != want:
                hit[m, w.t].add(w.cat)
    for m, types in sw.MUTANT_TYPES.items():
        for t in types:
            assert hit[m, t], f"no {pix}-bit witness tells the mutant {m} from the contract in {t}"
        for t in set(sw.TYPES) - set(types):   # where it is said not to apply it equals the contract
            assert all(sw.MUTANTS[m](w.p, w.D, w.G, t) == sw.exact_bits(w.p, w.D, w.G, t) for w in ws), (m, t)
    cats = set().union(*hit.values())
    for cat, (_, sizes) in sw.CATEGORIES.items():
        assert cat in cats or pix not in sizes, f"no mutant differs on a {pix}-bit witness of {cat}: the category is lost"
    # the mutants the categories were made for
    for m, t, cat in (("fused", "f16", "double_round_up"), ("fused", "bf16", "double_round_down"), ("distributed", "f32", "sub_rounds"),
                      ("fma", "f32", "sub_rounds"), ("ftz_in", "f32", "f32_subnormal_in"), ("ftz_out", "f32", "f32_subnormal_out"),
                      ("ftz_out", "f16", "subnormal_times_large"), ("ftz_cvt", "bf16", "bf16_subnormal"), ("flush_half", "f16", "half_subnormal"),
                      ("flush_half", "bf16", "bf16_subnormal"), ("ties_away", "f16", "tie_even"), ("truncate", "bf16", "tie_odd"),
                      ("truncate", "f16", "tie_plus_ulp"), ("distributed", "bf16", "tie_minus_ulp"), ("positive_zero", "f32", "zero_neg"),
                      ("truncate", "f16", "f16_to_inf"), ("truncate", "bf16", "bf16_to_inf"), ("early_inf", "f16", "f16_max"),
                      ("early_inf", "bf16", "bf16_max"), ("saturate", "f32", "f32_to_inf"), ("reversed", "f32", "zero_pos")):
        assert cat in hit[m, t], (m, t, cat)
    # the scalar pairs tell the rounding, flushing and zero mutants apart as well
    told = set()
    for s in sw.scalar_witnesses(pix):
        for p, tag in zip(s.ps, s.tags):
            if tag:
                told |= set(sw.told_apart(p, s.D0, s.G0, tag[1]))
    assert {"ties_away", "truncate", "ftz_in", "positive_zero", "saturate"} <= told


# ---- placement: every witness at every site of every kernel instance -------------------------------------------------

def threads_of(pix):
    return lambda c: PLAN[pix](c.W, c.H, c.n, *c.win)["threads"]


@pytest.mark.parametrize("pix", PIX)
def test_sites_restate_the_partition_on_a_small_window(pix):
    """A 20 x 3 window at x = 5 of a 64 x 48 frame in F32 at residue 1: one range of 60 elements per frame; its first
    3 and last 2 (1 + 60 = 61 = 15 * 4 + 1 -> 1 for frame 0) elements are site C, blocks over a row end are site B."""
    c = sw.Case("small", 64, 48, 2, (5, 8, 20, 3), None)
    assert threads_of(pix)(c) == 64
    site, slot = sw.sites(c, 64, 4, residue=1)
    assert site.shape == (2, 3, 20)
    flat = site[0].reshape(-1)
    assert flat[:3].tolist() == [2, 2, 2] and flat[-1] == 2 and flat[-2] != 2
    assert slot[0].reshape(-1)[:5].tolist() == [1, 2, 3, 0, 1]
    # blocks start at elements 3, 7, 11, 15, 19, ...: the one at 19 holds the row end (19 + 4 > 20): site B
    assert flat[3:19].tolist() == [0] * 16 and flat[19:23].tolist() == [1] * 4 and flat[23:27].tolist() == [0] * 4
    # frame 1 starts at element 60 of the output, 61 from the boundary: three elements of a first partial block again
    assert site[1].reshape(-1)[:4].tolist() == [2, 2, 2, 0] and slot[1, 0, 0] == 1
    # two pieces: rows leave one by one, no site B
    wide = sw.Case("pieces", 2100 if pix == 8 else 1100, 9, 1, (0, 0, 2100 if pix == 8 else 1100, 9), None)
    th = threads_of(pix)(wide)
    assert th == (256 if pix == 8 else 128) and PLAN[pix](wide.W, 9, 1)["pieces_x"] == 2
    site, _ = sw.sites(wide, th, 2)
    assert not (site == 1).any() and (site[0, :, 8 * th - 1] == 2).all() and (site[0, :, 0] == 2).all()


@pytest.mark.parametrize("t", sw.TYPES)
@pytest.mark.parametrize("pix", PIX)
def test_every_witness_meets_every_site_and_slot_of_every_instance(pix, t):
    K = len(sw.witnesses(pix))
    es = 4 if t == "f32" else 2
    cases = sw.cases(pix)
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    assert {(c.W, c.H) for c in cases} == {(200, 123), (600, 17), (2100 if pix == 8 else 1100, 9)}
    for c in cases:   # each case is small: at most 4M output elements
        assert c.n * c.win[2] * c.win[3] <= 1 << 22
    cov = sw.coverage(cases, threads_of(pix), lambda c: sw.witness_index(c, K), K, es)
    assert set(cov) == {64, 256 if pix == 8 else 128}, "the narrow and the wide instance"
    for th, (A, B, C) in cov.items():
        what = f"{pix}-bit {t} {th} threads"
        assert A.shape == (K, 16 // es) and A.all(), f"{what}: {int((~A).sum())} (witness, slot) pairs never at site A"
        assert B.all(), f"{what}: witnesses {np.flatnonzero(~B).tolist()} never at site B"
        assert C.all(), f"{what}: witnesses {np.flatnonzero(~C).tolist()} never at site C"
    # the pieces > 1 case alone: every row is its own range
    pieces = [c for c in cases if c.name == "wide pieces"]
    assert PLAN[pix](pieces[0].W, 9, 3)["pieces_x"] == 2
    # the scalar pairs: every pixel of every pair's list at all three sites of both instances
    cov = sw.coverage(sw.scalar_cases(pix), threads_of(pix), lambda c: sw.witness_index(c, 11, 1), 11, es)
    assert set(cov) == {64, 256 if pix == 8 else 128}
    for th, (A, B, C) in cov.items():
        assert A.all() and B.all() and C.all(), f"scalar pairs, {pix}-bit {t} {th} threads"


def test_witness_index_strides_through_the_set():
    c = sw.Case("x", 200, 123, 1, (0, 0, 200, 123), None)
    K = len(sw.witnesses(8))
    w = sw.witness_index(c, K)
    s = sw.stride(K)
    assert w[0, 0] == 0 and w[0, 1] == s % K and w[1, 0] == 200 * s % K and set(w.reshape(-1)[:K].tolist()) == set(range(K))
    org = sw.origins_of(sw.Case("o", 200, 123, 3, (0, 0, 61, 37), ((-5, 500), (139, 86), (3, 5))))
    assert org.tolist() == [[0, 86], [139, 86], [3, 5]]
    assert np.array_equal(org, sr.clamp_origins([(-5, 500), (139, 86), (3, 5)], 200, 123, 61, 37))
