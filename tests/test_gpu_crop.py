"""GPU: the compressed-domain crop of DBDE frames -- dbde_hip_crop_frames.  Every comparison is byte for byte.

Small frames are compared on the host with tests/crop_ref.py (the splice model that tests/test_crop_ref.py pins to
the reference), device-scale batches on the device with the path the crop replaces, encode_frames(decode_roi(...)).
Every call writes into a canvas of canary bytes, and every byte outside the accepted frames must keep its canary.
"""
import numpy as np
import pytest

import crafted
import crop_gpu as cg
import crop_ref

pytestmark = pytest.mark.gpu
BITS = 8


@pytest.fixture(scope="module")
def dv():
    import dbde_video_cpp_amd as m
    return m


@pytest.fixture(scope="module")
def codec(dv):
    c = dv.Codec(0)
    assert c.arch.startswith("gfx950")
    yield c
    c.close()


def crafted_frames(W, H, bits=BITS, seed=7):
    """Valid crafted frames of one geometry: every depth / minima / payload pattern once, and every (depth, minimum)
    pair with an all-ones payload (minima that wrap, depths larger than the range needs: non-canonical)."""
    rng = np.random.default_rng(seed + W * 31 + H)
    out = []
    for k, d in enumerate(crafted.DEPTHS):
        out.append(crafted.craft(rng, W, H, bits, d, crafted.MINIMA[k % 3], crafted.PAYLOADS[k % 3]))
    for k, m in enumerate(crafted.MINIMA):
        out.append(crafted.craft(rng, W, H, bits, "random", m, crafted.PAYLOADS[(k + 1) % 3]))
    out.append(crafted.all_pairs_frame(rng, "ones", "random", crafted.tiles(W, H), header=crafted.random_header(rng, 2),
                                       bits=bits))
    return out


def test_golden_frames_against_the_model_and_the_reference(codec, golden, request):
    manifest, arrays = golden
    from oracle_ffi import Reference
    ref = Reference() if Reference.available() else None
    for e in manifest["frames"]:
        img, packed = arrays[e["name"] + ".image"], np.asarray(arrays[e["name"] + ".packed"], np.uint8)
        W, H = e["W"], e["H"]
        frames = [packed, packed]
        for k, (x, y, rw, rh) in enumerate(crop_ref.windows(W, H)):
            buf, lead, offs, total = cg.upload(frames, misalign=k % 16)
            c = cg.run_crop(codec, BITS, buf, lead, total, offs, W, H, 2, x, y, rw, rh, out_misalign=(3 * k) % 16)
            outs = cg.check_host(c, frames, W, H, x, y, rw, rh, what=f"{e['name']} window {(x, y, rw, rh)}")
            if ref is not None:
                want = ref.pack_frame(0, np.ascontiguousarray(img[y:y + rh, x:x + rw]), rw, rh)
                want[4:20] = packed[4:20]
                assert outs[0].tobytes() == want.tobytes(), (e["name"], x, y, rw, rh)


@pytest.mark.parametrize("W,H", [(333, 77), (384, 384), (64, 64), (9, 200), (1, 1)])
def test_identity_crop_reproduces_every_frame(codec, golden, W, H):
    frames = crafted_frames(W, H)
    for how, slot in (("concat", 0), ("residues", 0), ("slots", max(len(f) for f in frames) + 5)):
        buf, lead, offs, total = cg.upload(frames, how, slot=slot)
        for slot_stride in (0, cg.max_frame(W, H, BITS) + 11):
            c = cg.run_crop(codec, BITS, buf, lead, total, offs, W, H, len(frames), 0, 0, W, H, slot_stride=slot_stride,
                            out_misalign=5)
            for f, fr in enumerate(frames):
                assert c.frame(f).cpu().numpy().tobytes() == fr.tobytes(), (W, H, how, slot_stride, f)
            c.untouched_outside_frames()


def test_identity_crop_of_golden_frames(codec, golden):
    manifest, arrays = golden
    for e in manifest["frames"]:
        packed = np.asarray(arrays[e["name"] + ".packed"], np.uint8)
        buf, lead, offs, total = cg.upload([packed], misalign=1)
        c = cg.run_crop(codec, BITS, buf, lead, total, offs, e["W"], e["H"], 1, 0, 0, e["W"], e["H"])
        assert c.frame(0).cpu().numpy().tobytes() == packed.tobytes(), e["name"]
        c.untouched_outside_frames()


@pytest.mark.parametrize("W,H", [(333, 77), (384, 384), (4104, 24)])
def test_non_canonical_streams_decode_to_the_window(codec, W, H):
    """Guarantee (a): decode_frames of the output as an rw x rh frame equals decode_roi of the source; and the output
    equals the model's (copied tiles stay as stored)."""
    frames = crafted_frames(W, H)
    n = len(frames)
    buf, lead, offs, total = cg.upload(frames, "residues")
    for (x, y, rw, rh) in crop_ref.windows(W, H):
        c = cg.run_crop(codec, BITS, buf, lead, total, offs, W, H, n, x, y, rw, rh, out_misalign=9)
        cg.check_host(c, frames, W, H, x, y, rw, rh, what=f"{W}x{H} {(x, y, rw, rh)}")
        want, _ = codec.decode_roi(buf, lead, total, offs, W, H, n, x, y, rw, rh)
        import torch
        got, res = codec.decode_frames(c.canvas, c.base, int(c.offsets[-1] + c.nbytes[-1]),
                                       torch.from_numpy(c.offsets).cuda(), rw, rh, n)
        codec.sync()
        assert torch.equal(got, want), (W, H, x, y, rw, rh)
        assert [r[3] for r in codec.parse_results(res)] == c.nbytes.tolist()


SCALE = [  # W, H, n, mode, windows
    (4096, 3072, 3, "mixed", [(1000, 696, 2045, 2043), (0, 0, 4096, 3072), (2048, 1024, 2048, 2048)]),
    (4096, 3072, 2, "noise8", [(1000, 696, 1024, 1024), (8, 8, 4081, 3059)]),
    (1921, 1081, 3, "mixed", [(0, 0, 1921, 1081), (960, 536, 961, 545), (8, 0, 1913, 1080), (1912, 1080, 9, 1)]),
    (8200, 24, 3, "noise8", [(0, 0, 8200, 24), (8, 8, 8185, 9), (4088, 0, 4112, 17)]),      # > 512 tiles wide
    (64, 64, 40, "mixed", [(0, 0, 64, 64), (8, 16, 33, 47), (56, 56, 8, 8)]),
]


@pytest.mark.parametrize("W,H,n,mode,wins", SCALE, ids=[f"{s[0]}x{s[1]}-{s[3]}" for s in SCALE])
def test_device_scale_batches_equal_decode_roi_then_encode(codec, dv, W, H, n, mode, wins):
    k = 0
    for slot_in in (None, 13):
        s = cg.Stream(codec, dv, mode, W, H, n, first=100, slot_extra=slot_in, misalign=3 if slot_in else 0)
        for (x, y, rw, rh) in wins:
            for slot_out in (None, 7):
                cg.check_device(codec, s, x, y, rw, rh, slot_extra=slot_out, out_misalign=(5 * k) % 16,
                                what=f"{W}x{H} {mode} {(x, y, rw, rh)} in {slot_in} out {slot_out}")
                k += 1


def test_every_residue_of_input_and_output_base(codec, dv):
    W, H, n = 1921, 97, 3
    s0 = cg.Stream(codec, dv, "mixed", W, H, n, first=5)
    for r in range(16):
        s = s0.moved(r)
        cg.check_device(codec, s, 8, 8, 1900, 83, out_misalign=(5 * r + 3) % 16, what=f"residue {r}")
        cg.check_device(codec, s, 0, 0, W, H, slot_extra=r, out_misalign=(11 * r + 1) % 16, what=f"residue {r} slots")


def test_per_frame_origins(codec, dv, oracle):
    W, H, n, rw, rh = 1000, 500, 9, 123, 61
    origins = [(-5, H), (W, -3), (10 ** 6, 10 ** 6), (-(10 ** 6), 7), (3, 5), (W - rw, H - rh), (W - rw + 1, 0),
               (437, 211), (872, 432)]
    s = cg.Stream(codec, dv, "mixed", W, H, n, first=1)
    c = cg.check_device(codec, s, 0, 0, rw, rh, origins=origins, what="origins")
    want = [crop_ref.clamp_origin(W, H, rw, rh, *o) for o in origins]
    assert c.used.tolist() == [list(o) for o in want]
    host = s.buf.cpu().numpy()
    o, z = s.offs.cpu().numpy(), s.sizes.cpu().numpy()
    frames = [host[s.lead + o[f]: s.lead + o[f] + z[f]] for f in range(n)]
    cg.check_host(c, frames, W, H, 0, 0, rw, rh, origins=origins, what="origins")
    # a window as wide as the frame allows: the frame's own partial edge for some origins, a cut tile for others
    W, H, n, rw, rh = 333, 77, 4, 300, 70
    s = cg.Stream(codec, dv, "noise8", W, H, n, first=9)
    for slot in (None, 3):
        cg.check_device(codec, s, 0, 0, rw, rh, slot_extra=slot, origins=[(0, 0), (33, 7), (32, 8), (16, 3)])


def rejected_batch(oracle, W, H):
    rng = np.random.default_rng(11)
    good = [oracle.pack_frame(50 + k, rng.integers(0, 256, (H, W), dtype=np.uint8) >> (k % 5), W, H) for k in range(4)]
    frames = [good[0]]
    for k, how in enumerate(crafted.BREAKS):
        frames += [crafted.break_rule(good[k % 4], how), good[(k + 1) % 4]]
    return frames


@pytest.mark.parametrize("slot_stride_extra", [None, 9])
def test_rejected_frames_between_good_ones(codec, oracle, slot_stride_extra):
    import torch
    W, H = 200, 123
    frames = rejected_batch(oracle, W, H)
    n = len(frames) + 1
    buf, lead, offs, total = cg.upload(frames, "residues")
    offs = torch.cat([offs, torch.tensor([total + 4096], dtype=torch.int64, device="cuda")])   # beyond the extent
    for (x, y, rw, rh) in [(0, 0, W, H), (8, 16, 101, 50), (96, 64, 104, 59)]:
        slot = cg.max_frame(rw, rh, BITS) + slot_stride_extra if slot_stride_extra is not None else 0
        c = cg.run_crop(codec, BITS, buf, lead, total, offs, W, H, n, x, y, rw, rh, slot_stride=slot, out_misalign=2)
        cg.check_host(c, frames + [np.zeros(0, np.uint8)], W, H, x, y, rw, rh, slot_stride=slot, what=f"{(x, y, rw, rh)}")
        _, want = codec.decode_frames(buf, lead, total, offs, W, H, n)
        codec.sync()
        assert torch.equal(c.results, want)
        assert (c.nbytes == 0).sum() == len(crafted.BREAKS) + 1


def test_last_frame_ends_the_stream_whatever_lies_behind(codec, oracle):
    import torch
    W, H = 200, 123
    rng = np.random.default_rng(3)
    frames = [oracle.pack_frame(k, rng.integers(0, 256, (H, W), dtype=np.uint8), W, H) for k in range(3)]
    outs = []
    for junk in (0x00, 0xFF):
        for r in range(16):
            host, lead, offs, total = crafted.layout(frames, "concat", lead=32 + r, junk=junk)
            buf = torch.from_numpy(host).cuda()
            c = cg.run_crop(codec, BITS, buf, lead, total, torch.from_numpy(offs).cuda(), W, H, 3, 8, 8, 185, 110)
            cg.check_host(c, frames, W, H, 8, 8, 185, 110, what=f"junk {junk} residue {r}")
            outs.append(c.canvas.cpu().numpy().tobytes())
    assert len(set(outs)) == 1


def test_no_frames_and_refused_calls_leave_the_output_untouched(codec, dv, oracle):
    import torch
    W, H, n = 100, 60, 2
    rng = np.random.default_rng(1)
    frames = [oracle.pack_frame(k, rng.integers(0, 256, (H, W), dtype=np.uint8), W, H) for k in range(n)]
    buf, lead, offs, total = cg.upload(frames)
    c = cg.run_crop(codec, BITS, buf, lead, total, offs, W, H, 0, 0, 0, 50, 30)
    c.untouched_outside_frames()
    canvas = cg.canary(4 * cg.max_frame(W, H, BITS))
    want = canvas.clone()
    cap = n * cg.max_frame(50, 30, BITS)
    for args, kw in (((4, 0, 50, 30), {}), ((0, 12, 50, 30), {}), ((56, 0, 50, 30), {}), ((0, 0, 50, 61), {}),
                     ((0, 0, 0, 30), {}), ((0, 0, 50, 30), dict(slot_stride=cg.max_frame(50, 30, BITS) - 1))):
        with pytest.raises(dv.DbdeError, match=r"\(-1\)"):
            codec.crop_frames(buf, lead, total, offs, W, H, n, *args, canvas, 64, canvas.numel() - 64, **kw)
    with pytest.raises(dv.DbdeError, match=r"\(-3\)"):
        codec.crop_frames(buf, lead, total, offs, W, H, n, 0, 0, 50, 30, canvas, 64, cap - 1)
    with pytest.raises(dv.DbdeError, match=r"\(-3\)"):
        codec.crop_frames(buf, lead, total, offs, W, H, n, 0, 0, 50, 30, canvas, 64, cap + cap // n - 1, slot_stride=cap)
    codec.sync()
    assert torch.equal(canvas, want)
