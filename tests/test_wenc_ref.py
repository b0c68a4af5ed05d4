"""CPU: the window encoder's model (tests/wenc_ref.py: pitched byte buffer -> clamped origin -> window -> oracle frame)
pinned to the real thing: the README's 10 x 10 image as a window of a pitched source gives the golden frame, the
reference's dbde_pack_frame agrees with the model on every geometry the GPU tests use, and origins are clamped by
dbde_hip_decode_roi's documented rule."""
import numpy as np
import pytest

import wenc_ref as wr

# (W, H, pitch, base, x, y, rw, rh) of the GPU tests' 8-bit cases: margins and narrow windows, alignments, surroundings,
# buffer edges, origins, record levels
CASES = ([(40, 29, 43, 1, 5, 3, rw, rh) for rw in range(17, 25) for rh in range(9, 17)]
         + [(40, 29, 43, 1, 5, 3, rw, 9) for rw in range(1, 17)]
         + [(100, 20, p, 0, x0, 2, 64, 16) for p in (100, 101, 112, 113) for x0 in range(16)]
         + [(33 + 29, 31 + 13, 33 + 32, 1, 11, 5, 33, 31), (72 + 29, 72 + 13, 72 + 32, 1, 11, 5, 72, 72)]
         + [(61, 23, p, 1, x, y, rw, rh) for p in (61, 66) for rw, rh in ((61, 23), (37, 13), (9, 5), (16, 8), (33, 23))
            for x, y in ((0, 0), (61 - rw, 23 - rh))]
         + [(90, 50, 91, 1, 7, 3, 33, 31), (47, 19, 47, 0, 13, 5, 20, 12), (1500, 1460, 1500, 0, 31, 7, 1456, 1448)])


def test_readme_image_as_a_window_of_a_pitched_source_gives_the_golden_frame(oracle, golden):
    manifest, arrays = golden
    img, packed = arrays["readme_10x10.image"].reshape(10, 10), arrays["readme_10x10.packed"]
    assert len(packed) == 112
    for fill in (0, 255):
        buf = wr.embed([img], 40, 29, 5, 3, 8, pitch=43, base=1, fill=fill)
        frames, offs, sizes = wr.encode_window(wr.packer(oracle), buf, 1, 40, 29, 43, 0, 1, 5, 3, 10, 10, first_index=7)
        assert frames[0].tobytes() == np.asarray(packed).tobytes() and offs == [0] and sizes == [112]


def test_reference_pack_frame_agrees_on_every_gpu_case(reference, oracle):
    rng = np.random.default_rng(2016)
    pack = wr.packer(oracle)
    for W, H, pitch, base, x, y, rw, rh in CASES:
        buf = rng.integers(0, 256, base + 2 * H * pitch + 64).astype(np.uint8)
        frames, _, _ = wr.encode_window(pack, buf, base, W, H, pitch, 0, 2, x, y, rw, rh, first_index=40)
        for f in range(2):
            win = wr.window(buf, base, pitch, H * pitch, f, x, y, rw, rh)
            assert frames[f].tobytes() == reference.pack_frame(40 + f, win, rw, rh).tobytes(), (W, H, pitch, x, y, rw, rh, f)


def test_window_reads_the_documented_bytes():
    buf = np.arange(7 + 3 * 1000, dtype=np.int64).astype(np.uint8)
    w8 = wr.window(buf, 7, 50, 1000, 2, 4, 3, 5, 2)
    assert w8.tolist() == [[(7 + 2000 + (3 + r) * 50 + 4 + c) & 255 for c in range(5)] for r in range(2)]
    w16 = wr.window(buf, 6, 50, 1000, 1, 4, 3, 5, 2, bits=16)
    at = lambda r, c: 6 + 1000 + (3 + r) * 50 + 2 * (4 + c)   # noqa: E731
    assert w16.tolist() == [[(at(r, c) & 255) | (((at(r, c) + 1) & 255) << 8) for c in range(5)] for r in range(2)]


def test_clamping_is_decode_rois_documented_rule(oracle):
    """include/dbde_hip.h, dbde_hip_decode_roi: origins are CLAMPED into [0, W-rw] x [0, H-rh]."""
    W, H, rw, rh = 90, 50, 33, 31
    assert wr.clamp_origin(-5, -5, W, H, rw, rh) == (0, 0)
    assert wr.clamp_origin(W, H, W, H, rw, rh) == (W - rw, H - rh)
    assert wr.clamp_origin(W - rw + 1, 4, W, H, rw, rh) == (W - rw, 4)
    assert wr.clamp_origin(-1, H - rh, W, H, rw, rh) == (0, H - rh)
    assert wr.clamp_origin(12, 7, W, H, rw, rh) == (12, 7)
    rng = np.random.default_rng(1)
    buf = rng.integers(0, 256, 3 * W * H).astype(np.uint8)
    pack = wr.packer(oracle)
    got, _, _ = wr.encode_window(pack, buf, 0, W, H, 0, 0, 3, 0, 0, rw, rh, origins=[(-5, -5), (W, H), (60, 2)])
    want = [pack(f, buf[f * W * H:(f + 1) * W * H].reshape(H, W)[y:y + rh, x:x + rw])
            for f, (x, y) in enumerate([(0, 0), (W - rw, H - rh), (W - rw, 2)])]
    assert [g.tobytes() for g in got] == [w.tobytes() for w in want]


def test_layouts_and_embed():
    pack = lambda index, img: np.full(10 + int(index), 1, np.uint8)   # noqa: E731
    buf = np.zeros(4 * 20 * 10, np.uint8)
    _, offs, sizes = wr.encode_window(pack, buf, 0, 20, 10, 0, 0, 4, 0, 0, 8, 8)
    assert offs == [0, 10, 21, 33] and sizes == [10, 11, 12, 13]
    _, offs, _ = wr.encode_window(pack, buf, 0, 20, 10, 0, 0, 4, 0, 0, 8, 8, slot_stride=100)
    assert offs == [0, 100, 200, 300]
    img = np.arange(6, dtype=np.uint16).reshape(2, 3) + 300
    b = wr.embed([img, img + 1], 8, 5, 2, 1, 16, pitch=20, base=2, fill=65535, exact=True)
    assert len(b) == 2 + 100 + 2 * 20 + 5 * 2
    assert wr.window(b, 2, 20, 100, 1, 2, 1, 3, 2, 16).tolist() == (img + 1).tolist()
    assert wr.window(b, 2, 20, 100, 0, 0, 0, 2, 1, 16).tolist() == [[65535, 65535]]
