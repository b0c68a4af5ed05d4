"""GPU: the DBDE16 encoder on the crafted images of tests/crafted_images.py (16-bit families).

The DBDE16 oracle is unpinned -- no reference defines the format -- so the depth and minimum arrays known by
construction are the one expectation here that does not pass through it.  Geometries: those of
tests/test_gpu_u16.py's persistent-encoder tests, with the fewest frames that still give the persistent encoder more
chunks than the device holds workgroups (the PIX = 2 instance of the persistent encoder at 16-byte rows and at
any width, output offsets that leave the U16 minima unaligned, image bases shifted by whole pixels, enc16_kernel for
everything else), and one small geometry per right and bottom margin 1..8.  Batches, layout and checks are those of
tests/test_gpu_crafted_encode.py: a mixed batch and a padding_trap batch per case, both slot layouts.
"""
import pytest

import crafted_images as ci
from test_gpu_crafted_encode import FIRST_INDEX, SENTINEL, mixed_frames, run_batch, trap_frames
from test_oracle_u16 import o16, pack16   # noqa: F401  (fixture + helper)

pytestmark = pytest.mark.gpu

CASES16 = [  # (W, H, n, output offset residue, image shift in pixels)
    (1000, 1003, 20, 32, 0), (1000, 1003, 20, 33, 0), (1024, 768, 24, 40, 0), (8, 8, 600 * 512, 32, 0), (4096, 3072, 2, 32, 0),
    (1001, 1003, 20, 32, 0),
    (1001, 67, 180, 32, 0), (1002, 67, 180, 32, 0), (1003, 61, 180, 32, 1), (1004, 67, 180, 32, 0), (1005, 67, 180, 32, 3),
    (1006, 70, 180, 32, 0), (1007, 67, 180, 32, 0), (1000, 67, 180, 32, 1), (1000, 67, 180, 32, 4), (9, 9, 700, 32, 0),
    (15, 8, 600, 32, 1),
] + [(24 + m, 16 + m, 7, 32, 0) for m in range(1, 9)] + [(200, 123, 5, 32, 0), (33, 31, 7, 32, 0), (1, 1, 2, 32, 0)]


@pytest.fixture(scope="module")
def codec():
    import dbde_video_cpp_amd as dv
    dv.build()
    c = dv.Codec(0)
    assert c.arch.startswith("gfx950")
    yield c
    c.close()


def test_cases_hold_every_margin():
    assert {c[0] % 8 or 8 for c in CASES16} == set(range(1, 9)) and {c[1] % 8 or 8 for c in CASES16} == set(range(1, 9))


@pytest.mark.parametrize("batch", ["mixed", "padding_trap"])
@pytest.mark.parametrize("W,H,n,off,shift", CASES16, ids=[f"{c[0]}x{c[1]}x{c[2]}-o{c[3]}-s{c[4]}" for c in CASES16])
def test_encoder16_on_crafted_images(codec, o16, W, H, n, off, shift, batch):   # noqa: F811
    T = ((W + 7) // 8) * ((H + 7) // 8)
    maxf = int(codec.L.dbde16_hip_max_frame_bytes(W, H))
    assert maxf == 32 + 131 * T
    # runs of the persistent encoder's 512-tile chunks and of enc16_kernel's 256-tile chunks, one tile off either way
    runs = (512, 511, 513, 256, 255, 257) if T > 512 else (64, T)
    slot = (maxf + 255) // 256 * 256
    # (hundreds of thousands of one-tile frames, and 12-megapixel frames -- one per family: the slot layout only)
    slots = (slot,) if n > 100000 or W * H > (1 << 23) else (0, slot)
    for stride in slots:
        def encode(images, out, lead, cap):
            return codec.encode_frames16(images, W, H, n, out, lead, cap, first_index=FIRST_INDEX, slot_stride=stride)

        def decode(out, lead, total, offs):
            return codec.decode_frames16(out, lead, total, offs, W, H, n)[0]

        batches, fill = (mixed_frames(W, H, n, 16, runs), SENTINEL) if batch == "mixed" else (trap_frames(W, H, n, 16), ci.GUARD)
        for imgs, info, which in batches:
            what = f"16-bit {W}x{H} x{n} (rm {W % 8 or 8}, dm {H % 8 or 8}) stride {stride} {batch} batch"
            run_batch(codec, what, W, H, 16, imgs, info, which, 2 * shift, off, stride,
                      lambda img: pack16(o16, img, 0)[20:], fill, encode, decode)
