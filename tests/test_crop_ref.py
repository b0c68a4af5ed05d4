"""CPU: tests/crop_ref.py (the splice model of the compressed-domain crop) against the oracles.

The contract of dbde_hip_crop_frames is byte identity with an encoder's frame of the cropped image, for sources an
encoder wrote.  Here the model is held to exactly that: against the pinned oracle's (and, where it is built, the
reference's own) dbde_pack_frame of the cropped image for DBDE, and against dbde16_oracle_pack_frame for DBDE16.
"""
import ctypes as C

import numpy as np
import pytest

import crafted
import crafted_images as ci
import crop_ref
from oracle_ffi import ORACLE_SO


def random_window(rng, W, H, k):
    """Window k of a frame: the whole frame, one that ends on the frame's own edge, free ones."""
    if k == 0:
        return 0, 0, W, H
    x, y = 8 * int(rng.integers(0, (W - 1) // 8 + 1)), 8 * int(rng.integers(0, (H - 1) // 8 + 1))
    if k == 1:
        return x, y, W - x, H - y
    return x, y, int(rng.integers(1, W - x + 1)), int(rng.integers(1, H - y + 1))


def image_of(rng, oracle, kind, W, H, it):
    if kind == 0:
        return rng.integers(0, 256, (H, W), dtype=np.uint8)
    if kind in (1, 2):
        return oracle.synth_frame(kind - 1, 0xC20B, it, W, H)          # noise8 / mixed
    d = int(rng.integers(0, 9))                                         # one depth everywhere
    base = int(rng.integers(0, 257 - (1 << d)))
    return (base + rng.integers(0, 1 << d, (H, W))).astype(np.uint8)


def family(rng_seed, n_frames, side, n_windows, oracle):
    rng = np.random.default_rng(rng_seed)
    for it in range(n_frames):
        W, H = int(rng.integers(1, side)), int(rng.integers(1, side))
        img = image_of(rng, oracle, it % 4, W, H, it)
        for k in range(n_windows):
            yield it, W, H, img, random_window(rng, W, H, k)


def with_header(frame, src):
    out = frame.copy()
    out[4:20] = src[4:20]
    return out


def test_splice_equals_the_oracle_encoder_of_the_cropped_image(oracle):
    stats, n = {}, 0
    for it, W, H, img, (x, y, rw, rh) in family(20161004, 400, 120, 6, oracle):
        src = oracle.pack_frame(1000 + it, img, W, H)
        got = crop_ref.crop_frame(src, W, H, x, y, rw, rh, stats=stats)
        want = with_header(oracle.pack_frame(0, np.ascontiguousarray(img[y:y + rh, x:x + rw]), rw, rh), src)
        assert got.tobytes() == want.tobytes(), (it, W, H, x, y, rw, rh, ci.first_difference(got, want, rw, rh))
        n += 1
    assert n == 2400 and stats["copied"] > 1000 and stats["recoded"] > 1000, stats


def test_splice_equals_the_reference_encoder_of_the_cropped_image(reference, oracle):
    for it, W, H, img, (x, y, rw, rh) in family(20161004, 400, 120, 6, oracle):
        src = reference.pack_frame(1000 + it, img, W, H)
        got = crop_ref.crop_frame(src, W, H, x, y, rw, rh)
        want = with_header(reference.pack_frame(0, np.ascontiguousarray(img[y:y + rh, x:x + rw]), rw, rh), src)
        assert got.tobytes() == want.tobytes(), (it, W, H, x, y, rw, rh, ci.first_difference(got, want, rw, rh))


def test_golden_frames_at_boundary_inside_and_edge_windows(oracle, golden):
    manifest, arrays = golden
    for e in manifest["frames"]:
        img, packed = arrays[e["name"] + ".image"], arrays[e["name"] + ".packed"]
        W, H = e["W"], e["H"]
        for (x, y, rw, rh) in crop_ref.windows(W, H):
            got = crop_ref.crop_frame(packed, W, H, x, y, rw, rh)
            want = with_header(oracle.pack_frame(0, np.ascontiguousarray(img[y:y + rh, x:x + rw]), rw, rh), packed)
            assert got.tobytes() == want.tobytes(), (e["name"], x, y, rw, rh)
        assert crop_ref.crop_frame(packed, W, H, 0, 0, W, H).tobytes() == np.asarray(packed).tobytes()


@pytest.fixture(scope="module")
def pack16(oracle):
    L = C.CDLL(ORACLE_SO)
    u8p, u16p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint16)
    L.dbde16_oracle_pack_frame.restype = C.c_size_t
    L.dbde16_oracle_pack_frame.argtypes = [C.c_uint64, u16p, C.c_int, C.c_int, u8p]

    def pack(index, img):
        H, W = img.shape
        img = np.ascontiguousarray(img, np.uint16)
        out = np.zeros(crop_ref.max_frame_bytes(W, H, 16) + 64, np.uint8)
        n = L.dbde16_oracle_pack_frame(index, img.ctypes.data_as(u16p), W, H, out.ctypes.data_as(u8p))
        return out[:n].copy()
    return pack


def test_splice16_equals_the_dbde16_oracle_of_the_cropped_image(pack16):
    rng = np.random.default_rng(20161005)
    n = 0
    for it in range(150):
        W, H = int(rng.integers(1, 70)), int(rng.integers(1, 70))
        d = int(rng.integers(0, 17)) if it % 2 else 16
        base = int(rng.integers(0, 65537 - (1 << d)))
        img = (base + rng.integers(0, 1 << d, (H, W))).astype(np.uint16)
        src = pack16(7 + it, img)
        for k in range(4):
            x, y, rw, rh = random_window(rng, W, H, k)
            got = crop_ref.crop_frame(src, W, H, x, y, rw, rh, bits=16)
            want = with_header(pack16(0, img[y:y + rh, x:x + rw]), src)
            assert got.tobytes() == want.tobytes(), (it, W, H, x, y, rw, rh, ci.first_difference(got, want, rw, rh, 16))
            n += 1
    assert n == 600


def test_batch_rules_rejected_frames_and_origins(oracle):
    rng = np.random.default_rng(5)
    W, H, rw, rh = 100, 60, 37, 21
    imgs = [rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(4)]
    frames = [oracle.pack_frame(f, imgs[f], W, H) for f in range(4)]
    frames[1] = crafted.break_rule(frames[1], "n64+1")
    origins = [(-5, 1000), (3, 3), (50, 17), (1000, -1)]
    outs, offs, nbytes, used = crop_ref.crop_batch(frames, W, H, 0, 0, rw, rh, origins=origins)
    assert used.tolist() == [[0, 32], [0, 0], [48, 16], [56, 0]]      # clamped, then rounded down to 8
    assert outs[1] is None and nbytes[1] == 0 and offs[1] == offs[2] == nbytes[0]
    for f in (0, 2, 3):
        x, y = used[f]
        n, img = crafted.decode_image(outs[f][20:], rw, rh)
        assert n == len(outs[f]) - 20 and np.array_equal(img, imgs[f][y:y + rh, x:x + rw])
    slot = crop_ref.max_frame_bytes(rw, rh) + 3
    _, offs, _, _ = crop_ref.crop_batch(frames, W, H, 8, 8, rw, rh, slot_stride=slot)
    assert offs.tolist() == [0, slot, 2 * slot, 3 * slot]
