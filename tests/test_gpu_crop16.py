"""GPU: the compressed-domain crop of DBDE16 frames -- dbde16_hip_crop_frames, the families of test_gpu_crop.py with
U16 minima and depths 0..16.  Small frames against tests/crop_ref.py's 16-bit model (pinned to dbde16_oracle_pack_frame
by tests/test_crop_ref.py), device-scale batches against encode_frames16(decode_roi16(...)), byte for byte.
"""
import numpy as np
import pytest

import crafted
import crop_gpu as cg
import crop_ref
from test_crop_ref import pack16   # noqa: F401  (fixture)
from test_gpu_crop import codec, crafted_frames, dv   # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
BITS = 16


def images16(rng, W, H, n):
    """Every depth 0..16 over the tiles, bases that make some sums pass 2^16 - 1 only where the format allows."""
    out = []
    for k in range(n):
        w, h = (W + 7) // 8, (H + 7) // 8
        sh = np.repeat(np.repeat(rng.integers(0, 18, (h, w)), 8, 0), 8, 1)[:H, :W]
        px = rng.integers(0, 65536, (H, W)) >> sh
        out.append((np.minimum(px + rng.integers(0, 65536 - int(px.max())), 65535)).astype(np.uint16))
    return out


@pytest.mark.parametrize("W,H", [(333, 77), (69, 69), (8, 8), (1, 1)])
def test_encoded_frames_against_the_model(codec, pack16, W, H):   # noqa: F811
    rng = np.random.default_rng(W + H)
    imgs = images16(rng, W, H, 3)
    frames = [pack16(1 << 40 | k, im) for k, im in enumerate(imgs)]
    for k, (x, y, rw, rh) in enumerate(crop_ref.windows(W, H)):
        buf, lead, offs, total = cg.upload(frames, "residues", misalign=k % 16)
        slot = cg.max_frame(rw, rh, BITS) + k if k % 2 else 0
        c = cg.run_crop(codec, BITS, buf, lead, total, offs, W, H, 3, x, y, rw, rh, slot_stride=slot,
                        out_misalign=(3 * k) % 16)
        outs = cg.check_host(c, frames, W, H, x, y, rw, rh, BITS, slot_stride=slot, what=f"{W}x{H} {(x, y, rw, rh)}")
        for f in range(3):   # guarantee (b): the encoder's frame of the cropped image
            want = pack16(0, imgs[f][y:y + rh, x:x + rw])
            want[4:20] = frames[f][4:20]
            assert outs[f].tobytes() == want.tobytes(), (W, H, x, y, rw, rh, f)


@pytest.mark.parametrize("W,H", [(333, 77), (136, 136), (1, 1)])
def test_identity_and_non_canonical_streams(codec, W, H):   # noqa: F811
    import torch
    frames = crafted_frames(W, H, BITS)
    n = len(frames)
    buf, lead, offs, total = cg.upload(frames, "residues")
    c = cg.run_crop(codec, BITS, buf, lead, total, offs, W, H, n, 0, 0, W, H, out_misalign=7)
    for f, fr in enumerate(frames):
        assert c.frame(f).cpu().numpy().tobytes() == fr.tobytes(), (W, H, f)
    c.untouched_outside_frames()
    for (x, y, rw, rh) in crop_ref.windows(W, H):
        c = cg.run_crop(codec, BITS, buf, lead, total, offs, W, H, n, x, y, rw, rh, out_misalign=9)
        cg.check_host(c, frames, W, H, x, y, rw, rh, BITS, what=f"{W}x{H} {(x, y, rw, rh)}")
        want, _ = codec.decode_roi16(buf, lead, total, offs, W, H, n, x, y, rw, rh)
        got, res = codec.decode_frames16(c.canvas, c.base, int(c.offsets[-1] + c.nbytes[-1]),
                                         torch.from_numpy(c.offsets).cuda(), rw, rh, n)
        codec.sync()
        assert torch.equal(got, want), (W, H, x, y, rw, rh)
        assert [r[3] for r in codec.parse_results(res)] == c.nbytes.tolist()


SCALE = [  # W, H, n, windows
    (4096, 3072, 2, [(1000, 696, 2045, 2043), (0, 0, 4096, 3072), (1000, 696, 1024, 1024)]),
    (1921, 1081, 2, [(0, 0, 1921, 1081), (960, 536, 961, 545), (1912, 1080, 9, 1)]),
    (8200, 24, 3, [(0, 0, 8200, 24), (8, 8, 8185, 9), (4088, 0, 4112, 17)]),      # > 512 tiles wide
    (64, 64, 40, [(0, 0, 64, 64), (8, 16, 33, 47)]),
]


@pytest.mark.parametrize("W,H,n,wins", SCALE, ids=[f"{s[0]}x{s[1]}" for s in SCALE])
def test_device_scale_batches_equal_decode_roi16_then_encode16(codec, dv, W, H, n, wins):   # noqa: F811
    k = 0
    for slot_in in (None, 13):
        s = cg.Stream16(codec, dv, W, H, n, first=100, slot_extra=slot_in, misalign=3 if slot_in else 0)
        for (x, y, rw, rh) in wins:
            for slot_out in (None, 7):
                cg.check_device(codec, s, x, y, rw, rh, slot_extra=slot_out, out_misalign=(5 * k) % 16,
                                what=f"16-bit {W}x{H} {(x, y, rw, rh)} in {slot_in} out {slot_out}")
                k += 1


def test_every_residue_and_per_frame_origins(codec, dv):   # noqa: F811
    W, H, n = 1921, 97, 3
    s0 = cg.Stream16(codec, dv, W, H, n, first=5)
    for r in range(16):
        s = s0.moved(r)
        cg.check_device(codec, s, 8, 8, 1900, 83, out_misalign=(5 * r + 3) % 16, what=f"residue {r}")
    W, H, n, rw, rh = 333, 77, 6, 300, 70
    s = cg.Stream16(codec, dv, W, H, n, first=9)
    origins = [(0, 0), (33, 7), (32, 8), (16, 3), (-4, 100), (10 ** 6, -(10 ** 6))]
    for slot in (None, 3):
        c = cg.check_device(codec, s, 0, 0, rw, rh, slot_extra=slot, origins=origins)
        assert c.used.tolist() == [list(crop_ref.clamp_origin(W, H, rw, rh, *o)) for o in origins]


def test_rejected_frames_between_good_ones(codec, pack16):   # noqa: F811
    import torch
    W, H = 200, 123
    rng = np.random.default_rng(11)
    good = [pack16(50 + k, im) for k, im in enumerate(images16(rng, W, H, 4))]
    frames = [good[0]]
    for k, how in enumerate(crafted.BREAKS):
        frames += [crafted.break_rule(good[k % 4], how, BITS), good[(k + 1) % 4]]
    n = len(frames) + 1
    buf, lead, offs, total = cg.upload(frames, "residues")
    offs = torch.cat([offs, torch.tensor([total + 4096], dtype=torch.int64, device="cuda")])   # beyond the extent
    for slot_extra in (None, 9):
        for (x, y, rw, rh) in [(0, 0, W, H), (8, 16, 101, 50), (96, 64, 104, 59)]:
            slot = cg.max_frame(rw, rh, BITS) + slot_extra if slot_extra is not None else 0
            c = cg.run_crop(codec, BITS, buf, lead, total, offs, W, H, n, x, y, rw, rh, slot_stride=slot, out_misalign=2)
            cg.check_host(c, frames + [np.zeros(0, np.uint8)], W, H, x, y, rw, rh, BITS, slot_stride=slot,
                          what=f"{(x, y, rw, rh)}")
            _, want = codec.decode_frames16(buf, lead, total, offs, W, H, n)
            codec.sync()
            assert torch.equal(c.results, want)
            assert (c.nbytes == 0).sum() == len(crafted.BREAKS) + 1


def test_last_frame_ends_the_stream_and_refused_calls(codec, dv, pack16):   # noqa: F811
    import torch
    W, H = 200, 123
    rng = np.random.default_rng(3)
    frames = [pack16(k, im) for k, im in enumerate(images16(rng, W, H, 3))]
    outs = []
    for junk in (0x00, 0xFF):
        for r in (0, 1, 7, 8, 15):
            host, lead, offs, total = crafted.layout(frames, "concat", lead=32 + r, junk=junk)
            c = cg.run_crop(codec, BITS, torch.from_numpy(host).cuda(), lead, total, torch.from_numpy(offs).cuda(), W, H,
                            3, 8, 8, 185, 110)
            cg.check_host(c, frames, W, H, 8, 8, 185, 110, BITS, what=f"junk {junk} residue {r}")
            outs.append(c.canvas.cpu().numpy().tobytes())
    assert len(set(outs)) == 1
    buf, lead, offs, total = cg.upload(frames)
    c = cg.run_crop(codec, BITS, buf, lead, total, offs, W, H, 0, 0, 0, 50, 30)
    c.untouched_outside_frames()
    canvas = cg.canary(4 * cg.max_frame(W, H, BITS))
    want = canvas.clone()
    mx = cg.max_frame(50, 30, BITS)
    for args, kw in (((4, 0, 50, 30), {}), ((0, 12, 50, 30), {}), ((0, 0, 50, 124), {}),
                     ((0, 0, 50, 30), dict(slot_stride=mx - 1))):
        with pytest.raises(dv.DbdeError, match=r"\(-1\)"):
            codec.crop_frames16(buf, lead, total, offs, W, H, 3, *args, canvas, 64, canvas.numel() - 64, **kw)
    with pytest.raises(dv.DbdeError, match=r"\(-3\)"):
        codec.crop_frames16(buf, lead, total, offs, W, H, 3, 0, 0, 50, 30, canvas, 64, 3 * mx - 1)
    codec.sync()
    assert torch.equal(canvas, want)
