"""CPU: tests/mask_ref.py (the threshold mask's definition) against a per-pixel loop, numpy.packbits and the edge cases."""
import numpy as np
import pytest

import mask_ref as mr


def loop(images, x, y, rw, rh, lo, hi, mode, origins=None):
    """The definition pixel by pixel, in plain Python integers."""
    n, H, W = images.shape
    nw = (rw + 63) // 64
    words = [[[0] * nw for _ in range(rh)] for _ in range(n)]
    cnt, box = [0] * n, [[rw, rh, -1, -1] for _ in range(n)]
    for f in range(n):
        ox, oy = (x, y) if origins is None else origins[f]
        ox, oy = min(max(int(ox), 0), W - rw), min(max(int(oy), 0), H - rh)
        for r in range(rh):
            for c in range(rw):
                X, Y = ox + c, oy + r
                p = int(images[f, Y, X])
                L = int(lo[Y, X]) if isinstance(lo, np.ndarray) else int(lo)
                Hh = int(hi[Y, X]) if isinstance(hi, np.ndarray) else int(hi)
                bit = (L <= p <= Hh) if mode == mr.INSIDE else (p < L or p > Hh)
                if bit:
                    words[f][r][c >> 6] |= 1 << (c & 63)
                    cnt[f] += 1
                    b = box[f]
                    box[f] = [min(b[0], c), min(b[1], r), max(b[2], c), max(b[3], r)]
    return np.array(words, np.uint64).reshape(n, rh, nw), np.array(cnt, np.uint32), np.array(box, np.int32)


@pytest.mark.parametrize("dtype,top", [(np.uint8, 255), (np.uint16, 65535)])
@pytest.mark.parametrize("W,H,win", [(9, 5, (0, 0, 9, 5)), (70, 4, (3, 1, 66, 3)), (131, 3, (1, 0, 129, 3)), (64, 2, (0, 0, 64, 2)),
                                     (1, 1, (0, 0, 1, 1))])
def test_against_the_pixel_loop(dtype, top, W, H, win):
    rng = np.random.default_rng(W * 100 + H + top)
    n = 3
    images = rng.integers(0, top + 1, (n, H, W)).astype(dtype)
    lo_map = rng.integers(0, top + 1, (H, W)).astype(dtype)
    hi_map = rng.integers(0, top + 1, (H, W)).astype(dtype)
    x, y, rw, rh = win
    org = np.array([[-4, 9], [x, y], [W, 0]], np.int32)
    for lo, hi in ((top // 3, 2 * top // 3), (lo_map, top), (0, hi_map), (lo_map, hi_map)):
        for mode in (mr.INSIDE, mr.OUTSIDE):
            for o in (None, org):
                got = mr.expected(images, x, y, rw, rh, lo, hi, mode, o)
                want = loop(images, x, y, rw, rh, lo, hi, mode, o)
                for g, w in zip(got, want):
                    assert g.dtype == w.dtype and np.array_equal(g, w)


@pytest.mark.parametrize("rw", [1, 63, 64, 65, 129, 200])
def test_pack_is_packbits_little_of_padded_rows(rw):
    rng = np.random.default_rng(rw)
    bits = rng.integers(0, 2, (2, 5, rw)).astype(bool)
    words = mr.pack(bits)
    nw = (rw + 63) // 64
    assert words.shape == (2, 5, nw)
    padded = np.zeros((2, 5, 64 * nw), bool)
    padded[:, :, :rw] = bits
    assert words.astype("<u8").tobytes() == np.packbits(padded, axis=2, bitorder="little").tobytes()
    assert np.array_equal(mr.unpack(words, rw), bits)


def test_the_empty_band_and_the_empty_box():
    rng = np.random.default_rng(1)
    images = rng.integers(0, 256, (2, 6, 70)).astype(np.uint8)
    words, cnt, box = mr.expected(images, 1, 1, 66, 4, 100, 99, mr.INSIDE)   # lo > hi: nothing lies inside
    assert not words.any() and (cnt == 0).all() and (box == [66, 4, -1, -1]).all()
    words, cnt, box = mr.expected(images, 1, 1, 66, 4, 100, 99, mr.OUTSIDE)  # ... and everything outside
    assert (cnt == 66 * 4).all() and (box == [0, 0, 65, 3]).all()
    assert (words[:, :, 0] == np.uint64(0xFFFFFFFFFFFFFFFF)).all() and (words[:, :, 1] == np.uint64(3)).all()
    images[1] = 7
    words, cnt, box = mr.expected(images, 0, 0, 70, 6, 8, 255, mr.INSIDE)
    assert cnt[1] == 0 and (box[1] == [70, 6, -1, -1]).all() and not words[1].any()
    one = np.zeros((1, 3, 65), np.uint8)
    one[0, 2, 64] = 200
    words, cnt, box = mr.expected(one, 0, 0, 65, 3, 200, 200)
    assert cnt[0] == 1 and (box[0] == [64, 2, 64, 2]).all() and words[0, 2, 1] == 1 and words.sum() == 1
