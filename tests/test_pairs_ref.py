"""CPU: the numpy reference of the neighbour-product projections (tests/pairs_ref.py) on cases worked out by hand, and
the cap of tests/pairs_gpu.py on the content the GPU tests use, at every shape and window they list."""
import numpy as np
import pytest

import pairs_gpu as pg
import pairs_ref as pref

SEED = 0x9E0_2016        # test_gpu_project.SEED: Batch's synthetic frames are the oracle's with this seed, frames 0..
MODES = {"noise8": 0, "mixed": 1, "flat": 2, "smooth": 3}


def test_a_3x3_window_of_two_frames_by_hand():
    a = np.array([[1, 2, 3],
                  [4, 5, 6],
                  [7, 8, 9]], np.uint8)
    b = np.array([[10, 0, 20],
                  [0, 30, 0],
                  [40, 0, 50]], np.uint8)
    want, n = pref.pairs([a, b], 15, 0, 0, 3, 3)
    assert n == 2 and want.dtype == np.uint64 and want.shape == (4, 3, 3)
    right = [[1 * 2, 2 * 3, 0], [4 * 5, 5 * 6, 0], [7 * 8, 8 * 9, 0]]                  # b adds nothing: a 0 in every pair
    down = [[1 * 4, 2 * 5, 3 * 6], [4 * 7, 5 * 8, 6 * 9], [0, 0, 0]]
    down_right = [[1 * 5 + 10 * 30, 2 * 6, 0], [4 * 8, 5 * 9 + 30 * 50, 0], [0, 0, 0]]
    down_left = [[0, 2 * 4, 3 * 5 + 20 * 30], [0, 5 * 7 + 30 * 40, 6 * 8], [0, 0, 0]]
    assert want.tolist() == [right, down, down_right, down_left]
    # plane j is the j-th set bit in ascending order
    assert pref.pairs([a, b], 10, 0, 0, 3, 3)[0].tolist() == [down, down_left]
    assert pref.pairs([a, b], 4, 0, 0, 3, 3)[0].tolist() == [down_right]
    assert pref.offsets_of(10) == [(0, 1), (-1, 1)]


def test_a_rejected_frame_adds_nothing_and_the_window_cuts_the_pairs():
    rng = np.random.default_rng(3)
    ims = [rng.integers(0, 256, (9, 11), dtype=np.uint8) for _ in range(3)]
    one, n1 = pref.pairs(ims, 15, 2, 1, 5, 4)
    two, n2 = pref.pairs(ims[:1] + [None] + ims[1:] + [None], 15, 2, 1, 5, 4)
    assert (n1, n2) == (3, 3) and np.array_equal(one, two)
    none, n0 = pref.pairs([None, None], 3, 0, 0, 4, 4)
    assert n0 == 0 and none.shape == (2, 4, 4) and not none.any()
    # pixels outside the window never contribute, even where the frame has them: the last column / row hold 0
    assert not one[0][:, -1].any() and not one[1][-1].any() and not one[2][-1].any() and not one[2][:, -1].any()
    assert not one[3][-1].any() and not one[3][:, 0].any()
    assert one[0][1, 3] == sum(int(im[2, 5]) * int(im[2, 6]) for im in ims)
    assert one[3][0, 1] == sum(int(im[1, 3]) * int(im[2, 2]) for im in ims)
    # U16 values of 65,535: two frames give 2 * 65,535^2 > 2^32 exactly
    big = np.full((4, 4), 65535, np.uint16)
    assert pref.pairs([big, big], 1, 0, 0, 4, 4)[0][0, 0, 0] == 2 * 65535 ** 2 > 2 ** 32


def test_has_partner_of_strips_and_corners():
    assert not pref.has_partner(15, 1, 1).any()
    tall = pref.has_partner(15, 1, 5)                 # one pixel wide: only DOWN has partners
    assert tall[1][:4].all() and not tall[1][4].any() and not tall[[0, 2, 3]].any()
    flat = pref.has_partner(15, 5, 1)                 # one pixel high: only RIGHT
    assert flat[0][:, :4].all() and not flat[0][:, 4].any() and not flat[1:].any()
    two = pref.has_partner(15, 2, 2)
    assert two.sum(axis=(1, 2)).tolist() == [2, 2, 1, 1] and two[2][0, 0] and two[3][0, 1]


def test_local_correlation_by_hand():
    """Two pixels side by side over three frames: (1, 2, 3) against (2, 4, 6) is r = 1, against (3, 2, 1) r = -1; a
    constant pixel is left out, and a pixel with no pair left gives 0."""
    f = [np.array([[1, 2, 3, 7]], np.uint8), np.array([[2, 4, 2, 7]], np.uint8), np.array([[3, 6, 1, 7]], np.uint8)]
    r = pref.local_correlation(f, 1, 0, 0, 4, 1)
    assert r[0, 0] == pytest.approx(1.0) and r[0, 1] == pytest.approx(0.0) and r[0, 2] == pytest.approx(-1.0)
    assert r[0, 3] == 0.0
    assert pref.local_correlation(f, 2, 0, 0, 4, 1).tolist() == [[0.0] * 4]     # no row below


def test_distinct_rejects_swapped_self_paired_and_empty_planes():
    rng = np.random.default_rng(5)
    ims = [rng.integers(0, 256, (8, 8), dtype=np.uint8) for _ in range(2)]
    want, _ = pref.pairs(ims, 15, 0, 0, 8, 8)
    pg.distinct(want, pg.sumsq(ims, (0, 0, 8, 8)))
    with pytest.raises(AssertionError):
        pg.distinct(np.stack([want[0], want[0]]))
    with pytest.raises(AssertionError):
        pg.distinct(np.stack([want[0], np.zeros_like(want[0])]))
    with pytest.raises(AssertionError):
        pg.distinct(want[:1], want[0])
    flat = [np.full((8, 8), 9, np.uint8)]
    with pytest.raises(AssertionError):                      # flat content cannot tell the offsets apart
        pg.distinct(pref.pairs(flat, 15, 0, 0, 8, 8)[0])


@pytest.mark.parametrize("mode", ["mixed", "noise8", "smooth"])
def test_the_gpu_tests_content_meets_the_cap(oracle, mode):
    """The frames test_gpu_pairs.py encodes (the oracle's synthetic frames are the device generator's, held equal by
    test_gpu_parity.py) at every shape, frame count and window of at least 3 x 3 it uses."""
    import test_gpu_pairs as t
    cases = [(W, H, n) for W, H in t.SHAPES for n in (t.COUNTS if mode == "mixed" else (5,))]
    if mode == "mixed":
        cases += [(72, 40, 50), (72, 40, 70), t.WIDE + (3,)]
    for W, H, n in cases:
        ims = [oracle.synth_frame(MODES[mode], SEED, f, W, H) for f in range(n)]
        wins = t.windows(W, H) if mode == "mixed" else t.windows(W, H)[:2]
        if (W, H) == t.WIDE:
            wins = [(0, 0, W, H), (4090, 3, 14, 12)]
        seen = 0
        for win in wins:
            if win[2] >= 3 and win[3] >= 3:
                pg.expected(ims, 15, win)
                seen += 1
        assert seen >= 2
