"""CPU: the cases of tests/bound_cases.py can fail -- before tests/test_gpu_bounds.py runs them on a device.

  * the palette frames decode (tests/crafted.py's decoder) to the images the references use, with the depths, wrapping
    minima and pixel classes the module's docstring promises in every tile row;
  * the counting references equal the brute-force references of each family (family_refs, gproject_ref, registered_ref,
    pairs_ref, lag_ref) on the same palettes and orders cut to a few dozen frames and short segments;
  * at full length every designated U32 statistic reaches its header bound in every tile row, a quarter of each tile
    row's pixels lies in [2^31, 2^32) and some pixel below 2^31;
  * six wrong kernels (bound_cases.mutant) give planes that differ from the expectation in every tile row;
  * the plans put the cases where intended at 1, 64, 256 and 304 compute units: frames_per_segment = 65,536.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bound_cases as bc          # noqa: E402
import crafted as cr              # noqa: E402
import gproject_ref as gref       # noqa: E402
import lag_ref as lr              # noqa: E402
import pairs_ref as pref          # noqa: E402
import registered_ref as rr       # noqa: E402
from family_refs import reduce16, reduce_numpy   # noqa: E402

FB = [(f, b) for f in bc.FAMILIES for b in bc.BITS]
ROWS = 16                          # tile rows of the CPU setups: one period of the rolls (8) and of the depths (8 / 16)
_SETUPS = {}


def setup_of(family, bits):
    """The family's palette at 16 tile rows (grouped: its own 16 x 64, two tiles across): rows repeat with period 16,
    so what holds for every tile row here holds at any device's 4 * n_cu rows."""
    if (family, bits) not in _SETUPS:
        _SETUPS[(family, bits)] = bc.Setup(family, bits, shape=None if family == "groups" else (8, 8 * ROWS))
    return _SETUPS[(family, bits)]


@pytest.fixture(scope="module")
def dv():
    import dbde_video_cpp_amd as m
    if not os.path.exists(m.LIB_PATH):
        m.build()
    return m


# ---- the palette ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("family,bits", FB)
def test_palette_frames_decode_to_their_images(family, bits):
    s = setup_of(family, bits)
    for k, (fr, im) in enumerate(zip(s.frames, s.images)):
        used, header, got = cr.decode_frame(fr, s.W, s.H, bits)
        assert used == len(fr) and header == (2, k, 0)
        assert got.dtype == im.dtype and np.array_equal(got, im)
        assert np.array_equal(s.window(k, bc.ORIGINS[k]), s.contents[k])
    buf, lead, offs, total = s.stream()
    assert total == sum(len(fr) for fr in s.frames) and list(offs) == list(np.cumsum([0] + [len(f) for f in s.frames[:-1]]))
    rows = s.result_rows([3, 0])
    assert rows.tolist() == [[2, 3, 0, len(s.frames[3])], [2, 0, 0, len(s.frames[0])]]


@pytest.mark.parametrize("bits", bc.BITS)
def test_palette_depths_and_classes(bits):
    full = bc.FULL[bits]
    s = setup_of("project", bits)
    T = cr.tiles(s.W, s.H)
    dep = {k: np.asarray(s.frames[k][24:24 + T]) for k in range(4)}
    mb = bits // 8
    mins = {k: np.asarray(s.frames[k][28 + T:28 + T + mb * T]).view("<u2" if mb == 2 else np.uint8).astype(np.int64)
            for k in range(4)}
    assert not dep[1].any() and not dep[3].any() and (mins[1] == full).all()     # F: flat at full scale
    A, B = s.contents[0], s.contents[2]
    seen = set()
    for q in range(T):
        dA, dB = int(dep[0][q]), int(dep[2][q])
        assert (dA, dB) == bc.depths_of(bits, q) and dA >= 1 and dB >= 1 and dA != dB
        seen.update((dA, dB))
        if bits == 16:
            assert (dA + dB) % 2 == 1                     # one odd-depth tile under the FF pixels of every tile row
        for d, m in ((dA, mins[0][q]), (dB, mins[2][q])):
            assert m == (0 if d == bits else full + 1 - (1 << (d - 1)))      # below full depth the minimum wraps
        cl = bc.classes_of(q)
        a, b = A[8 * q:8 * q + 8], B[8 * q:8 * q + 8]
        assert ((a == full) & (b == full))[cl == "FF"].all() and (cl == "FF").sum() == 20
        assert (a[cl == "F0"] == full).all() and (b[cl == "F0"] == 0).all() and (cl == "F0").sum() == 8
        assert (a[cl == "0F"] == 0).all() and (b[cl == "0F"] == full).all() and (cl == "0F").sum() == 8
        hh = cl == "HH"
        assert (a[hh] >= bc.HIGH[bits]).all() and (b[hh] >= bc.HIGH[bits]).all() and hh.sum() == 20
        ll = cl == "LL"
        assert (a[ll] < 1 << (bits - 2)).all() and (b[ll] < 1 << (bits - 2)).all() and ll.sum() == 8
        if min(dA, dB) >= 4:
            assert (a[hh] < full).any() and not np.array_equal(a[hh], b[hh])       # mid values, not the same in A and B
        if q:                                                                      # no two neighbours alike
            assert not np.array_equal(a, A[8 * q - 8:8 * q]) and not np.array_equal(b, B[8 * q - 8:8 * q])
            assert not np.array_equal(cl, bc.classes_of(q - 1))
    assert seen == set(range(1, bits + 1))
    power = 2 if bits == 8 else 1          # the 8-bit statistic at the bound is a square, the 16-bit one the sum
    assert bc.HIGH[bits] ** power * bc.N_SEG >= 2 ** 31 > (bc.HIGH[bits] - 1) ** power * bc.N_SEG


@pytest.mark.parametrize("bits", bc.BITS)
def test_registered_windows_tell_the_origins_apart(bits):
    """Slot k's window shows its contents only at its own origin: at every other slot's origin, and one pixel off, the
    A and B frames show something else (F is full scale everywhere: its origin cannot matter)."""
    s = setup_of("registered", bits)
    assert (s.W, s.H) == (s.rw + 16, s.rh + 16)
    for k in (0, 2):
        ox, oy = bc.ORIGINS[k]
        for o in [bc.ORIGINS[j] for j in range(4) if j != k] + [(ox + 1, oy), (ox, oy + 1), (ox - 1, oy)]:
            if o != (ox, oy):
                assert not np.array_equal(s.window(k, o), s.contents[k]), (k, o)
    assert np.array_equal(s.window(0, (-5, 99999)), s.window(0, (0, s.H - s.rh)))      # clamped as the header says
    assert len({(d, int(m)) for fr in s.frames for d, m in zip(fr[24:24 + 8], fr[28:28 + 8])}) > 4


# ---- the counting references against the brute-force ones ---------------------------------------------------------

def brute_images(s, slots):
    return [s.images[int(k)] for k in slots]


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and np.array_equal(got.astype(np.int64), want.astype(np.int64)), what


@pytest.mark.parametrize("name", bc.ORDERS)
@pytest.mark.parametrize("family,bits", FB)
def test_counting_equals_brute_force(family, bits, name):
    s = setup_of(family, bits)
    n, fps = 45, 16                                   # three segments, the last one short
    slots = bc.order(name, n, half=fps)
    images = brute_images(s, slots)
    red = reduce_numpy if bits == 8 else reduce16
    what = (family, bits, name)
    if family == "project":
        got, want = bc.expected(s, slots, n, fps=fps), red(images, 0, 0, s.rw, s.rh)
        for k in ("max", "min", "sum", "sumsq", "count"):
            same(got[k], want[k], what + (k,))
    elif family == "registered":
        for org in (bc.origins_of(slots), np.asarray([(7, 0), (-3, 40), (16, 9)], np.int32)[np.arange(n) % 3]):
            got, want = bc.expected(s, slots, n, fps=fps, origins=org), rr.registered(images, org, s.rw, s.rh, bits)
            for k in ("max", "min", "sum", "sumsq", "count"):
                same(got[k], want[k], what + (k,))
    elif family == "pairs":
        got = bc.expected(s, slots, n, fps=fps)
        want, count = pref.pairs(images, 15, 0, 0, s.rw, s.rh)
        assert tuple(pref.OFFSETS) == bc.PAIR_OFFSETS and got["count"] == count
        same(got["product"], want, what)
    elif family == "lag":
        for lag in (1, 2, 3):
            got, want = bc.expected(s, slots, n, lag=lag, fps=fps), lr.lag(images, lag, 0, 0, s.rw, s.rh, 0, bits)
            for k in lr.STATS + ("pairs", "count"):
                same(got[k], want[k], what + (lag, k))
    else:
        for ranges in (gref.group_ranges(n, group_frames=fps), gref.group_ranges(n, starts=[0, 33]),
                       gref.group_ranges(n, starts=[5, 5, 45, 20])):
            got = bc.expected_groups(s, slots, ranges)
            want = gref.reduce_groups(images, ranges, 0, 0, s.rw, s.rh, bits // 8)
            for k in ("max", "min", "sum", "sumsq", "counts"):
                same(got[k], want[k], what + (k,))


@pytest.mark.parametrize("family,bits", FB)
def test_accumulated_calls_double(family, bits):
    s = setup_of(family, bits)
    slots = bc.order("mixed", 40)
    if family == "groups":
        one, two = (bc.expected_groups(s, slots, [(0, 40)], times=t) for t in (1, 2))
        assert np.array_equal(two["sum"], 2 * one["sum"]) and np.array_equal(two["max"], one["max"])
        big = bc.expected_groups(s, bc.order("mixed", bc.N_SEG), [(0, bc.N_SEG)], times=2)
        assert (big["sum"] < 2 ** 32).all() and big["counts"].tolist() == [2 * bc.N_SEG]
        assert big["sum"].max() == (2 * bc.N_SEG * 65535 - 2 ** 32 if bits == 16 else 2 * bc.N_SEG * 255)
        return
    lag = 2 if family == "lag" else 0
    one, two = (bc.expected(s, slots, 40, lag=lag, times=t) for t in (1, 2))
    for k in bc.SUMS[family] + ("count",) + (("pairs",) if lag else ()):
        assert np.array_equal(two[k], 2 * np.asarray(one[k]))
    for k in bc.EXTREMES[family]:
        assert np.array_equal(two[k], one[k])


# ---- at full length -----------------------------------------------------------------------------------------------

FULL_CASES = [(f, b, c) for f, b in FB for c in bc.cases(f)]
IDS = [f"{f}{b}-{c[0]}" for f, b, c in FULL_CASES]


_PARTS = {}


def parts_of(family, bits, case):
    """(setup, the partial of every segment or group of the case, each one's last term), computed once."""
    if (family, bits, case) not in _PARTS:
        s = setup_of(family, bits)
        _, n, name, lag = case
        slots = bc.order(name, n)
        ranges = bc.ranges_of(family, case)
        _PARTS[(family, bits, case)] = s, s.parts(slots, ranges, lag), s.last_terms(slots, ranges, lag)
    return _PARTS[(family, bits, case)]


@pytest.mark.parametrize("family,bits,case", FULL_CASES, ids=IDS)
def test_full_length_planes_reach_the_bounds(family, bits, case):
    s, parts, _ = parts_of(family, bits, case)
    assert [p["frames"] for p in parts] == [min(bc.N_SEG, case[1] - lo) - (case[3] if lo == 0 else 0)
                                            for lo, _ in bc.ranges_of(family, case)]
    checked = 0
    for k in bc.designated(family, case):
        if k not in bc.U32[(family, bits)]:
            assert k in bc.U64[(family, bits)]
            continue
        top = np.maximum.reduce([p[k] for p in parts])          # per pixel, the fullest accumulator of the call
        assert (top <= bc.bound(bits, k)).all() and bc.bound(bits, k) < 2 ** 32
        if bc.fills(family, case):
            assert bc.tile_rows(top == bc.bound(bits, k)).all(), (k, "no pixel at the bound in some tile row")
        if k in bc.near(family, bits):
            quarter = 8 * s.rw // 4
            assert (bc.tile_row_counts(top >= 2 ** 31) >= quarter).all(), (k, bc.tile_row_counts(top >= 2 ** 31).min())
            assert bc.tile_rows(top < 2 ** 31).all(), k
        checked += 1
    assert checked or (family, bits) == ("pairs", 16) or (family, bits, case[3]) == ("lag", 16, 2)


def test_every_u32_statistic_meets_its_bound_somewhere():
    for family, bits in FB:
        met = {k for c in bc.cases(family) if bc.fills(family, c) for k in bc.designated(family, c)}
        assert set(bc.U32[(family, bits)]) <= met, (family, bits)
        assert set(bc.U32[(family, bits)]) | set(bc.U64[(family, bits)]) == set(bc.SUMS[family])
    assert bc.bound(8, "sumsq") == 4261478400 and bc.bound(16, "sum") == 4294901760 == 2 ** 32 - 65536
    assert bc.bound(8, "pairsum") == 65536 * 510 and bc.near("lag", 8) == ("product", "sqdiff")
    assert bc.near("project", 8) == ("sumsq",) and bc.near("project", 16) == ("sum",) and bc.near("lag", 16) == ("absdiff",)


def check_mutants(family, bits, case):
    """Every mutant of the case's designated sums differs from the expectation in every tile row.  Returns the mutants
    that applied."""
    s, parts, lasts = parts_of(family, bits, case)
    keep = bc.designated(family, case)
    # a grouped call never adds two groups: each group is judged as a call of its own
    calls = [([p], [t]) for p, t in zip(parts, lasts)] if family == "groups" else [(parts, lasts)]
    applied = set()
    for ps, ts in calls:
        want = bc.fold(s, ps)
        for which in bc.MUTANTS:
            for k, plane in bc.mutant(s, which, ps, ts).items():
                if k in keep:
                    assert bc.tile_rows(plane != want[k]).all(), (which, k, "equals the expectation in some tile row")
                    applied.add(which)
    return applied


@pytest.mark.parametrize("family,bits,case", FULL_CASES, ids=IDS)
def test_mutants_differ_in_every_tile_row(family, bits, case):
    assert {"c", "d"} <= check_mutants(family, bits, case)


def test_every_mutant_applies_where_it_can():
    """(a), (b), (e) wherever a U32 statistic's bound reaches 2^31 ((e) but for the groups, which are never added),
    (c) and (d) everywhere, (f) wherever a U64 accumulator exists."""
    for family, bits in FB:
        got = set().union(*(check_mutants(family, bits, c) for c in bc.cases(family)))
        want = {"c", "d"}
        if bc.near(family, bits):
            want |= {"a", "b"} | ({"e"} if family != "groups" else set())
        if bc.U64[(family, bits)]:
            want.add("f")
        assert got == want, (family, bits, sorted(got ^ want))


# ---- the plans ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_cu", [1, 64, 256, 304])
@pytest.mark.parametrize("bits", bc.BITS)
def test_plans_put_the_cases_at_the_bound(dv, bits, n_cu):
    W, H = bc.shape_for(n_cu)
    sfx = "" if bits == 8 else "16"
    plan = {k: getattr(dv, f"{k}{sfx}_plan") for k in ("project", "registered", "pairs", "lag", "project_groups")}
    for n in (bc.N_SEG, 2 * bc.N_SEG):
        plans = [plan["project"](W, H, n, n_cu=n_cu), plan["pairs"](W, H, n, pairs=15, n_cu=n_cu),
                 plan["registered"](W + bc.MARGIN, H + bc.MARGIN, n, W, H, n_cu=n_cu)]
        plans += [plan["lag"](W, H, n, lag=lag, stats=31, n_cu=n_cu) for lag in (1, 2)]
        for p in plans:
            assert p["frames_per_segment"] == p["max_frames_per_segment"] == bc.N_SEG
            assert p["segments"] == n // bc.N_SEG and p["grid"] == 4 * n_cu * p["segments"]
            assert p["combine_grid"] == (0 if n == bc.N_SEG else -(-W * H // 256))
        for lag, p in zip((1, 2), plans[3:]):
            assert p["first_pair"] == lag and p["history_frames"] == (p["segments"] - 1) * lag
        # one tile row less and the plan cuts: this is the smallest frame that stops it
        if n_cu > 1:
            assert plan["project"](W, H - 8, bc.N_SEG, n_cu=n_cu)["frames_per_segment"] == bc.N_SEG // 2
    g = plan["project_groups"](*bc.GROUPS_SHAPE, 2 * bc.N_SEG, group_frames=bc.N_SEG, n_cu=n_cu)
    assert g["max_group_frames"] == bc.N_SEG and g["runs"] * g["groups_per_run"] == 2 and g["runs"] in (1, 2)
    r = plan["project_groups"](*bc.GROUPS_SHAPE, bc.N_SEG, has_group_starts=True, n_groups=1, n_cu=n_cu)
    assert (r["runs"], r["groups_per_run"]) == (1, 1)
    with pytest.raises(ValueError):
        plan["project_groups"](*bc.GROUPS_SHAPE, 2 * bc.N_SEG, group_frames=bc.N_SEG + 1, n_cu=n_cu)
