"""CPU: tests/match_ref.py against a per-shift, per-pixel loop, and a cap on every case of tests/match_cases.py before
any GPU run.

The cap: on a case's noise content the expected surfaces must tell the right kernel from one that mixes up axes or
offsets.  Over the live entries of every case
  * prod differs from prod with the template transposed (where tw = th) and with the template rolled by one pixel in x
    and in y (where that changes the template);
  * every requested surface differs from the one whose search patch sits one pixel further in x, and in y (sum and sq
    do not see the template, so their offset errors are those of the patch);
  * every requested surface differs from itself with dx and dy swapped (where D > 1).
The shift-recovery scenes of the registration tests must have a unique arg-max at the true shift.
"""
import numpy as np
import pytest

import match_cases as mc
import match_ref as mr
import patch_ref as pr


def loop_surfaces(P, T, S):
    th, tw = T.shape
    D = 2 * S + 1
    out = np.zeros((3, D, D), dtype=object)
    for dy in range(-S, S + 1):
        for dx in range(-S, S + 1):
            p = s = q = 0
            for i in range(th):
                for j in range(tw):
                    v = int(P[i + dy + S][j + dx + S])
                    p += int(T[i][j]) * v
                    s += v
                    q += v * v
            out[0][dy + S][dx + S], out[1][dy + S][dx + S], out[2][dy + S][dx + S] = p, s, q
    return out


@pytest.mark.parametrize("bits", (8, 16))
@pytest.mark.parametrize("tw,th,S", [(1, 1, 0), (3, 5, 2), (9, 1, 1), (6, 6, 3)])
def test_surfaces_equal_the_loop(bits, tw, th, S):
    rng = np.random.default_rng(tw * 100 + th * 10 + S + bits)
    dt = np.uint8 if bits == 8 else np.uint16
    P = rng.integers(0, mc.top(bits) + 1, size=(th + 2 * S, tw + 2 * S)).astype(dt)
    T = rng.integers(0, mc.top(bits) + 1, size=(th, tw)).astype(dt)
    P[0, 0] = T[0, 0] = mc.top(bits)
    got = mr.surfaces(P, T, S)
    want = loop_surfaces(P, T, S)
    for g, w in zip(got, want):
        assert g.dtype == np.int64 and g.tolist() == w.tolist()


def test_expected_follows_patch_ref_and_leaves_dead_entries():
    rng = np.random.default_rng(3)
    W, H, S, tw, th = 40, 30, 2, 5, 4
    frames = [rng.integers(0, 256, size=(H, W)).astype(np.uint8), None, rng.integers(0, 256, size=(H, W)).astype(np.uint8)]
    T = rng.integers(0, 256, size=(2, th, tw)).astype(np.uint8)
    org = np.array([[(-3, -2), (36, 27)]] * 3)
    prod, sm, sq, used, live = mr.expected(frames, W, H, T, S, org, counts=[2, 2, 1], mode=pr.FILL, fill=200)
    assert live.tolist() == [[True, True], [False, False], [True, False]]
    assert (prod[1] == mr.UNTOUCHED).all() and (sq[2, 1] == mr.UNTOUCHED).all() and (used[1] == pr.UNTOUCHED_ORIGIN).all()
    P, _ = pr.patch(frames[0], W, H, tw + 2 * S, th + 2 * S, -3, -2, pr.FILL, 200)
    assert P[0, 0] == 200 and prod[0, 0].tolist() == loop_surfaces(P, T[0], S)[0].tolist()
    assert used[0].tolist() == [[-3, -2], [36, 27]]
    _, _, _, used_c, _ = mr.expected(frames, W, H, T, S, org, mode=pr.CLAMP)
    assert used_c[0].tolist() == [[0, 0], [W - tw - 2 * S, H - th - 2 * S]]


def test_best_tie_rule_and_nan():
    S = 1
    s = np.full((3, 3), 0.5)
    assert mr.best(s, S) == ((0, 0), 0.5)                     # all tied: the centre
    s[1, 1] = 0.1
    assert mr.best(s, S) == ((0, -1), 0.5)                    # |dx| + |dy| = 1: the smallest dy first
    s[0, 1] = 0.1
    assert mr.best(s, S) == ((-1, 0), 0.5)                    # then the smallest dx
    s[:] = np.nan
    assert mr.best(s, S)[0] == (0, 0) and np.isnan(mr.best(s, S)[1])
    s[2, 2] = -0.9
    assert mr.best(s, S) == ((1, 1), -0.9)                    # NaN never wins
    assert mr.best(np.array([[5, 3, 3], [4, 4, 9], [3, 8, 8]]), S, maximize=False) == ((0, -1), 3)


@pytest.mark.parametrize("bits", (8, 16))
@pytest.mark.parametrize("c", mc.CASES, ids=mc.IDS)
def test_every_case_tells_axes_and_offsets_apart(c, bits):
    frames, T, org, counts = mc.content(c, bits)
    W, H, S, mode, fill = c["W"], c["H"], c["S"], c["mode"], mc.fill_of(c, bits)
    base = mr.expected(list(frames), W, H, T, S, org, counts, mode, fill)
    live = base[4]
    assert live.any(), "no live entry"
    req = [i for i in range(3) if c["stats"] >> i & 1]

    def differs(other, which):
        return all((base[i][live] != other[i][live]).any() for i in which)

    if 0 in req:   # prod is requested: the template's axes and offsets
        if c["tw"] == c["th"] and c["tw"] > 1:
            assert differs(mr.expected(list(frames), W, H, T.transpose(0, 2, 1), S, org, counts, mode, fill), [0]), "transposed"
        for axis, size in ((2, c["tw"]), (1, c["th"])):
            if size > 1:
                assert differs(mr.expected(list(frames), W, H, np.roll(T, 1, axis=axis), S, org, counts, mode, fill), [0]), axis
    for d in ((1, 0), (0, 1)):   # the patch one pixel off
        moved = np.clip(org + np.array(d), mc.I32_MIN, mc.I32_MAX)
        assert differs(mr.expected(list(frames), W, H, T, S, moved, counts, mode, fill), req), d
    if S > 0:
        assert differs([b.transpose(0, 1, 3, 2) for b in base[:3]], req), "dx and dy swapped"
    # an 8-bit entry fits the U32 chain of the kernel, a 16-bit entry 2^46
    assert max(int(base[i][live].max()) for i in range(3)) < (2 ** 32 if bits == 8 else 2 ** 46)


def test_case_list_covers_what_the_issue_names():
    by = {c["name"]: c for c in mc.CASES}
    assert {c["S"] for c in mc.CASES} >= {0, 1, 2, 8, 16}
    assert {(c["tw"], c["th"]) for c in mc.CASES} >= set(mc.TEMPLATES) | {(128, 128)}
    assert by["largest"]["S"] == 16 and {c["stats"] for c in mc.CASES} == set(range(1, 8))
    rng = np.random.default_rng(0)
    res = mc.origins_of(by["residues"], rng)[0]
    assert {(int(x) & 7, int(y) & 7) for x, y in res} == {(a, b) for a in range(8) for b in range(8)}
    assert {mc.origins_of(by[k], rng).shape[1] for k in ("K1_own", "K3_own", "K70_shared")} == {1, 3, 70}
    assert all(72 <= c["W"] <= 200 and c["H"] >= 56 and 2 <= c["n"] <= 5 for c in mc.CASES)
    assert any(c["W"] % 8 and c["H"] % 8 for c in mc.CASES)


def test_scenes_have_a_unique_maximum_at_the_true_shift():
    sc = mc.SCENE
    ref, frames = mc.scene_frames()
    S, tw, th = sc["S"], sc["tw"], sc["th"]
    assert all(max(abs(dx), abs(dy)) <= 6 for dx, dy in sc["shifts"]) and S == 8
    T = np.stack([ref[y:y + th, x:x + tw] for x, y in sc["positions"]])
    org = np.array([[(x - S, y - S) for x, y in sc["positions"]]] * sc["n"])
    prod, sm, sq, _, live = mr.expected(list(frames), sc["W"], sc["H"], T, S, org, mode=pr.CLAMP)
    assert live.all()
    for f, (dx, dy) in enumerate(sc["shifts"]):
        z = np.stack([mr.zncc(prod[f, k], sm[f, k], sq[f, k], T[k]) for k in range(len(T))])
        assert not np.isnan(z).any()
        mean = z.mean(0)
        assert mr.best(mean, S)[0] == (dx, dy), f
        assert (mean == mean.max()).sum() == 1, f
        for k in range(len(T)):   # every patch on its own as well: the piecewise-rigid field is the rigid one here
            assert mr.best(z[k], S)[0] == (dx, dy) and (z[k] == z[k].max()).sum() == 1, (f, k)
