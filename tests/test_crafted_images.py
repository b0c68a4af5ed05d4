"""CPU: the crafted image families of tests/crafted_images.py do what they claim.

For every family and both pixel sizes, over shapes that hold every pair of margins (W mod 8, H mod 8): the oracle's
depth and minimum arrays are the arrays the construction states, three encoders agree byte for byte (the oracle,
crafted_images.pack_numpy and -- 8-bit, where oracle/_ref is built -- the reference), and two decoders return the
image.  Then the coverage each family promises is counted, and mutants of the encoding (an unclamped load, wrong
padding, a min/max that drops a row, a column or a half tile) are shown to change what the family pins.  No kernel is
involved: tests/test_gpu_crafted_encode.py runs the same families through the encoders.
"""
import numpy as np
import pytest

import crafted as cr
import crafted_images as ci
from test_oracle_u16 import o16, pack16, unpack16   # noqa: F401  (fixture + helpers)

# every (rm, dm) in 1..8 x 1..8 once, one to three tiles a side (an interior tile in each)
SHAPES = [(8 * (1 + (rm + dm) % 2) + rm, 8 * (1 + (rm + 2 * dm) % 2) + dm) for rm in range(1, 9) for dm in range(1, 9)]
# frames one tile wide or high, single-tile frames, single-pixel tiles
NARROW = [(1, 1), (1, 9), (9, 1), (3, 20), (20, 3), (8, 8), (5, 7), (7, 29), (8, 17), (33, 8)]
LONE_FRAMES = 64          # a tile's lone pixel moves one valid position per frame: 64 frames visit them all
RUNS = (4, 3, 5)          # depth_runs on these small frames: runs of a few tiles, one off either way


def margins(W, H):
    return W % 8 or 8, H % 8 or 8


def test_shapes_hold_every_margin_pair():
    assert {margins(W, H) for W, H in SHAPES} == {(rm, dm) for rm in range(1, 9) for dm in range(1, 9)}
    assert all(ci.Grid(W, H).cls.min() == 0 for W, H in SHAPES), "every shape has an interior tile"


def all_families(bits):
    """(family, frame numbers) of the differential checks."""
    out = [(ci.lone_extreme(True), range(LONE_FRAMES)), (ci.lone_extreme(False), range(LONE_FRAMES)),
           (ci.range_ladder, range(8)), (ci.padding_trap, range(6))]
    out += [(ci.depth_runs(r), range(12)) for r in RUNS]
    out += [(ci.bit_patterns(d), range(4)) for d in range(1, bits + 1)] + [(ci.bit_patterns(), range(8))]
    out += [(ci.depth_runs(RUNS[0], "runs"), range(2))]
    return out


def oracle_pack(oracle, o16, img, bits):   # noqa: F811
    """frame_data (no frame header) of the image by the oracle of its pixel size."""
    H, W = img.shape
    return oracle.pack_image(img, W, H) if bits == 8 else pack16(o16, img, 0)[20:]


def oracle_unpack(oracle, o16, data, W, H, bits):   # noqa: F811
    if bits == 8:
        return oracle.unpack_image(data, W, H)
    return unpack16(o16, np.concatenate([np.zeros(20, np.uint8), data]), W, H)


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("rm", list(range(1, 9)) + ["narrow"])
def test_families_against_the_oracle(oracle, o16, bits, rm):   # noqa: F811
    shapes = NARROW if rm == "narrow" else [s for s in SHAPES if margins(*s)[0] == rm]
    mb = bits // 8
    for W, H in shapes:
        T = cr.tiles(W, H)
        for fam, frames in all_families(bits):
            for f in frames:
                what = f"{fam.__name__} {W}x{H} ({bits}-bit) frame {f}"
                img, depth, minimum = fam(W, H, f, bits)
                assert img.shape == (H, W) and img.dtype == ci.dtype_of(bits) and len(depth) == len(minimum) == T
                data = oracle_pack(oracle, o16, img, bits)
                d, m, _, _ = ci.frame_arrays(np.concatenate([np.zeros(20, np.uint8), data]), W, H, bits)
                assert np.array_equal(d, depth), f"{what}: the oracle's depths {d} are not the construction's {depth}"
                assert np.array_equal(m, minimum), f"{what}: the oracle's minima {m} are not the construction's {minimum}"
                if f >= 6:
                    continue
                mine = ci.pack_numpy(img, bits)
                assert mine.tobytes() == data.tobytes(), \
                    f"{what}: pack_numpy and the oracle: " + ci.first_difference(
                        np.concatenate([np.zeros(20, np.uint8), mine]), np.concatenate([np.zeros(20, np.uint8), data]), W, H, bits)
                assert len(data) == 12 + T + mb * T + 8 * int(depth.astype(np.int64).sum())
                n, back = cr.decode_image(data, W, H, bits)
                assert n == len(data) and np.array_equal(back, img), f"{what}: the numpy decoder"
                n, back = oracle_unpack(oracle, o16, data, W, H, bits)
                assert n == len(data) and np.array_equal(back, img), f"{what}: the oracle's decoder"


@pytest.mark.parametrize("rm", list(range(1, 9)) + ["narrow"])
def test_oracle_equals_the_reference_on_the_families(oracle, reference, rm):
    shapes = NARROW if rm == "narrow" else [s for s in SHAPES if margins(*s)[0] == rm]
    for W, H in shapes:
        for fam, frames in all_families(8):
            for f in list(frames)[:8]:
                img, _, _ = fam(W, H, f, 8)
                a, b = oracle.pack_frame(f, img, W, H), reference.pack_frame(f, img, W, H)
                assert a.tobytes() == b.tobytes(), \
                    f"{fam.__name__} {W}x{H} frame {f}: oracle and reference: " + ci.first_difference(a, b, W, H)
                n, _, back = reference.unpack_frame(a, W, H)
                assert n == len(a) and np.array_equal(back, img)


def test_frame_numpy_is_the_oracles_frame(oracle, o16):   # noqa: F811
    for bits in (8, 16):
        img, _, _ = ci.range_ladder(27, 13, 2, bits)
        want = oracle.pack_frame(77, img, 27, 13) if bits == 8 else pack16(o16, img, 77)
        assert ci.frame_numpy(77, img, bits).tobytes() == want.tobytes()
        assert ci.first_difference(ci.frame_numpy(77, img, bits), want, 27, 13, bits) == "equal"


# ---- coverage, counted ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [8, 16])
def test_lone_extreme_visits_every_position_and_delta_in_every_tile_class(bits):
    nd = len(ci.deltas(bits))
    for W, H in SHAPES + NARROW:
        g = ci.Grid(W, H)
        for high in (True, False):
            fam = ci.lone_extreme(high)
            seen_pos = {c: set() for c in np.unique(g.cls)}
            seen_delta = {c: set() for c in np.unique(g.cls)}
            for f in range(LONE_FRAMES):
                img, depth, minimum = fam(W, H, f, bits)
                px = ci.tile_pixels(img, bits)
                # the family's own claim first: in every tile exactly one VALID pixel differs from the others
                valid = ((np.arange(64) // 8)[None, :] < g.vr[:, None]) & ((np.arange(64) % 8)[None, :] < g.vc[:, None])
                for t in range(g.T):
                    v = px[t][valid[t]]
                    if len(v) == 1:
                        continue
                    vals, counts = np.unique(v, return_counts=True)
                    assert len(vals) == 2 and 1 in counts, (W, H, f, t, v)
                    lone = vals[counts == 1][-1 if high else 0] if len(v) == 2 else vals[counts == 1][0]
                    assert (lone == vals.max()) == high or len(v) == 2
                    at = int(np.nonzero(valid[t] & (px[t] == lone))[0][0])
                    seen_pos[g.cls[t]].add((at // 8, at % 8))
                    seen_delta[g.cls[t]].add(int(vals[1] - vals[0]))
            for c in seen_pos:
                k = int(np.nonzero(g.cls == c)[0][0])
                if g.nvalid[k] == 1:
                    continue
                want = {(r, col) for r in range(int(g.vr[k])) for col in range(int(g.vc[k]))}
                assert seen_pos[c] == want, f"{W}x{H} {ci.CLASSES[c]} high={high}: positions never visited: {want - seen_pos[c]}"
                assert seen_delta[c] == set(ci.deltas(bits)), f"{W}x{H} {ci.CLASSES[c]} high={high}: {nd} deltas, seen {sorted(seen_delta[c])}"


@pytest.mark.parametrize("bits", [8, 16])
def test_range_ladder_realises_every_range(bits):
    want = set(ci.ladder_ranges(bits))
    assert want >= set(range(256)) and max(want) == ci.top_of(bits)
    for W, H in SHAPES + [(9, 1), (20, 3), (8, 8)]:
        seen, minima = set(), set()
        for f in range(ci.ladder_frames(W, H, bits)):
            img, depth, minimum = ci.range_ladder(W, H, f, bits)
            px = ci.tile_pixels(img, bits)
            r = px.max(1) - px.min(1)
            assert np.array_equal(ci.bit_length(r), depth)
            seen.update(int(v) for v in r)
            minima.update(zip((int(v) for v in r), (int(v) for v in minimum)))
        assert seen == want, f"{W}x{H}: ranges never realised: {sorted(want - seen)}"
        assert any(m == 0 and r > 0 for r, m in minima) and any(m == ci.top_of(bits) - r and r > 0 for r, m in minima)


@pytest.mark.parametrize("bits", [8, 16])
def test_depth_runs_realise_their_patterns(bits):
    for W, H in SHAPES + [(200, 123)]:
        g = ci.Grid(W, H)
        many = g.nvalid > 1                      # a single-pixel tile is depth 0 whatever the pattern asks
        for run in RUNS + (g.T,):
            for kind in ci.RUN_KINDS:
                img, depth, _ = ci.depth_runs(run, kind)(W, H, 0, bits)
                want = ci.run_pattern(kind, g.T, run, bits)
                assert np.array_equal(depth[many], want[many]), (W, H, run, kind)
                if kind == "runs":   # ... and its complement in the odd frames
                    assert np.array_equal(ci.depth_runs(run, kind)(W, H, 1, bits)[1][many], (bits - want)[many])
                px = ci.tile_pixels(img, bits)
                assert np.array_equal(ci.bit_length(px.max(1) - px.min(1)), depth), (W, H, run, kind)
            # the frames of the family take the kinds in turn, `runs` starting empty and full in turn
            kinds = [tuple(ci.depth_runs(run)(W, H, f, bits)[1][many]) for f in range(12)]
            for k, kind in enumerate(ci.RUN_KINDS):
                assert kinds[k] == tuple(ci.run_pattern(kind, g.T, run, bits)[many])
            assert kinds[8] == tuple((bits - ci.run_pattern("runs", g.T, run, bits))[many])
    # the patterns themselves
    assert list(ci.run_pattern("runs", 10, 3, 8)) == [0, 0, 0, 8, 8, 8, 0, 0, 0, 8]
    assert list(ci.run_pattern("last", 4, 3, 16)) == [0, 0, 0, 16] and list(ci.run_pattern("first", 3, 3, 8)) == [8, 0, 0]
    assert list(ci.run_pattern("stairs", 10, 3, 8)) == [0, 1, 2, 3, 4, 5, 6, 7, 8, 0]
    assert set(ci.run_pattern("odd", 64, 3, 16)) == {1, 3, 5, 7, 9, 11, 13, 15} and set(ci.run_pattern("odd", 9, 3, 8)) == {1, 3, 5, 7}


@pytest.mark.parametrize("bits", [8, 16])
def test_every_depth_occurs_in_every_edge_class(bits):
    for W, H in SHAPES:
        g = ci.Grid(W, H)
        depths = {fam.__name__: np.stack([fam(W, H, f, bits)[1] for f in frames]) for fam, frames in all_families(bits)}
        for c in np.unique(g.cls):
            k = int(np.nonzero(g.cls == c)[0][0])
            if c == 0 or g.nvalid[k] == 1:
                continue
            for name in ("lone_high", "lone_low"):
                seen = set(np.unique(depths[name][:, g.cls == c]))
                assert seen >= set(range(1, bits + 1)), f"{name} {W}x{H} {ci.CLASSES[c]}: depths {sorted(seen)}"
            seen = set().union(*(np.unique(d[:, g.cls == c]) for d in depths.values()))
            assert seen == set(range(bits + 1)), f"{W}x{H} {ci.CLASSES[c]}: depths {sorted(seen)}"


@pytest.mark.parametrize("bits", [8, 16])
def test_bit_patterns_hold_their_patterns(bits):
    W, H = 40, 16
    for d in range(1, bits + 1):
        full = (1 << d) - 1
        kinds, bases = set(), set()
        for f in range(6):
            img, depth, minimum = ci.bit_patterns(d)(W, H, f, bits)
            g = ci.Grid(W, H)
            px = ci.tile_pixels(img, bits)
            base = ci.walk_minimum(g.t // 4 + f, full, bits)
            v = px - base[:, None]
            for t in range(g.T):
                k = (t + f) % 4
                i = np.arange(64)
                if k == 0:
                    assert sorted(v[t])[0] == 0 and sorted(v[t])[1] == full and (v[t] == full).sum() == 63
                elif k in (1, 2):
                    want = ((i // 8 + i % 8) & 1) * full
                    assert np.array_equal(v[t], want if k == 1 else full - want)
                else:
                    assert np.array_equal(v[t], 1 << (i % d))
                kinds.add(k)
                bases.add(int(base[t]))
            assert (depth[(g.t + f) % 4 != 3] == d).all()
        assert kinds == {0, 1, 2, 3} and 0 in bases and ci.top_of(bits) - full in bases


# ---- mutants: each family catches the fault it exists for ----------------------------------------------------------------

TRAP_W = list(range(1, 26)) + [75, 100]
TRAP_H = list(range(1, 26)) + [70]


def partial_tiles(g):
    return np.nonzero(g.cls != 0)[0]


@pytest.mark.parametrize("bits", [8, 16])
def test_padding_trap_catches_an_unclamped_load(oracle, bits):
    """A full 8 x 8 read at pitch W where the tile is partial (what a kernel does that forgets a margin), inside the
    buffer the GPU test builds: the depth of EVERY partial tile of every frame changes."""
    n = 3
    for W in TRAP_W:
        for H in TRAP_H:
            g = ci.Grid(W, H)
            buf, lead, frames = ci.trap_batch(W, H, n, bits)
            flat = buf if bits == 8 else buf.view(np.uint16)
            at0 = lead // (bits // 8)
            assert (buf[:lead] == ci.GUARD).all() and (buf[lead + n * W * H * (bits // 8):] == ci.GUARD).all()
            for f, (img, depth, _) in enumerate(frames):
                for t in partial_tiles(g):
                    at = at0 + f * W * H + 8 * int(g.ty[t]) * W + 8 * int(g.tx[t])
                    rows = at + W * np.arange(8)[:, None] + np.arange(8)[None, :]
                    assert rows.max() < len(flat), "the guard behind the batch covers the read"
                    block = flat[rows].astype(np.int64)
                    d = int(ci.bit_length(block.max() - block.min()))
                    assert d != int(depth[t]), f"{W}x{H} ({bits}-bit) frame {f} tile {t}: unclamped depth {d} is the clamped one"
                    if bits == 8:
                        code, _, _ = oracle.pack_8x8(buf, at, W)
                        assert code >> 8 == d


def padded_tiles(img, how):
    """tile_pixels with a wrong padding: `first_row`: every row extended with the FIRST row's last valid pixel;
    `zeros`: zeros to the right of and below the valid part."""
    H, W = img.shape
    g = ci.Grid(W, H)
    px = ci.tile_pixels(img).reshape(g.T, 8, 8).copy()
    for t in range(g.T):
        vc, vr = int(g.vc[t]), int(g.vr[t])
        if how == "first_row":
            px[t, :, vc:] = px[t, 0, vc - 1]
        else:
            px[t, :, vc:] = 0
            px[t, vr:, :] = 0
    return px.reshape(g.T, 64)


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("how", ["first_row", "zeros"])
def test_padding_trap_catches_wrong_padding(bits, how):
    for W, H in SHAPES + NARROW + [(75, 70), (100, 100)]:
        g = ci.Grid(W, H)
        hit = (g.vc < 8) & (g.vr >= 2)
        for f in range(3):
            img, _, _ = ci.padding_trap(W, H, f, bits)
            good, bad = ci.tile_pixels(img, bits), padded_tiles(img, how)
            for t in np.nonzero(hit)[0]:
                a, b = ci.pack_tiles(good[t:t + 1], bits), ci.pack_tiles(bad[t:t + 1], bits)
                assert a[2].tobytes() != b[2].tobytes(), f"{W}x{H} ({bits}-bit) frame {f} tile {t}: {how} padding leaves the payload as it is"


DROPS = [("row", r) for r in range(8)] + [("column", c) for c in range(8)] + [("half", h) for h in ("left", "right", "top", "bottom")]


def kept(drop):
    what, k = drop
    keep = np.ones((8, 8), bool)
    if what == "row":
        keep[k, :] = False
    elif what == "column":
        keep[:, k] = False
    else:
        keep[{"left": (slice(None), slice(0, 4)), "right": (slice(None), slice(4, 8)), "top": (slice(0, 4), slice(None)),
              "bottom": (slice(4, 8), slice(None))}[k]] = False
    return keep.reshape(64)


@pytest.mark.parametrize("bits", [8, 16])
def test_lone_extreme_catches_a_reduction_that_drops_pixels(bits):
    """A min/max over the tile that leaves out one row, one column or one half: the depth array changes in some frame
    of the family, in each polarity, at every shape."""
    for W, H in SHAPES:
        for high in (True, False):
            fam = ci.lone_extreme(high)
            alive = {d: True for d in DROPS}
            for f in range(LONE_FRAMES):
                img, depth, _ = fam(W, H, f, bits)
                px = ci.tile_pixels(img, bits)
                for d in [d for d in DROPS if alive[d]]:
                    k = kept(d)
                    got = ci.bit_length(px[:, k].max(1) - px[:, k].min(1))
                    if not np.array_equal(got, depth):
                        alive[d] = False
            assert not any(alive.values()), f"{W}x{H} ({bits}-bit) high={high}: never caught: {[d for d in DROPS if alive[d]]}"


def test_a_mixed_batch_holds_every_family_and_every_depth_pattern():
    """What the GPU tests encode: 24 frames are two of every family, neighbours from different families, the run
    pattern at each run length in both phases, every depth in one bit_patterns frame."""
    runs = (16, 15, 17)
    imgs, info = ci.mixed_batch(72, 40, 24, 8, runs)
    names = [i[0] for i in info]
    assert len(set(names)) == 12 and all(a != b for a, b in zip(names, names[1:]))
    assert {"lone_high", "lone_low", "range_ladder", "bit_patterns()"} <= set(names)
    for r in runs:
        two = [tuple(i[2]) for i in info if i[0] == f"depth_runs({r}, runs)"]
        assert two == [tuple(ci.run_pattern("runs", 45, r, 8)), tuple(8 - ci.run_pattern("runs", 45, r, 8))]
    for k in ci.RUN_KINDS:
        assert any(i[0] == f"depth_runs(16, {k})" for i in info)
    assert set(next(i[2] for i in info if i[0] == "bit_patterns()")) >= set(range(1, 9))
    assert len({im.tobytes() for im in imgs}) == 24
