"""GPU: scaled float decode of DBDE16 streams -- dbde16_hip_decode_scaled (Codec.decode_scaled16).

As tests/test_gpu_scaled.py with U16 pixels: expected values are tests/scaled_ref.py's definition applied to the images
dbde16_hip_decode_frames writes for the same frames (which the DBDE16 oracle's decode equals: Batch16 checks it), bit
pattern for bit pattern, in guarded outputs off 16-byte alignment.
"""
import numpy as np
import pytest

import crafted as cr
import scaled_ref as sr
from test_gpu_project import windows
from test_gpu_project16 import Crafted16
from test_gpu_roi16 import Batch16, images16
from test_gpu_scaled import SENT, SHAPES, Out, compare, run
from test_oracle_u16 import o16   # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

CALL = "decode_scaled16"


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


def batch(codec, o16, kind, W, H, n, seed=0, **kw):   # noqa: F811
    import torch
    b = Batch16(codec, o16, images16(np.random.default_rng(W * 31 + H + n + seed), n, W, H, kind), **kw)
    _, b.results = codec.decode_frames16(b.buf, b.lead, b.total, b.offs, W, H, n)
    codec.sync()
    assert all((b.gpu_full[f] == b.full[f]).all() for f in range(n))
    assert isinstance(b.results, torch.Tensor)
    return b


def maps16(images, seed):
    """The standard maps; half the frames' pixels lie far above the dark level (U16), so the forced p == D pixels and
    the small differences come from frame 0."""
    n, H, W = images.shape
    return sr.maps(seed, W, H, pixels=images[0])


@pytest.mark.parametrize("kind", ("mixed", "full"))
@pytest.mark.parametrize("W,H,n", SHAPES)
def test_windows_in_all_types_with_both_maps(codec, o16, kind, W, H, n):   # noqa: F811
    import torch
    b = batch(codec, o16, kind, W, H, n)
    images = b.gpu_full
    dark, gain = maps16(images, W + H)
    import test_gpu_scaled as g8
    dd, dg = g8.dev(dark), g8.dev(gain)
    for win in windows(W, H):
        for t in sr.TYPES:
            what = f"{kind} {W}x{H} window {win} {t}"
            got, res = run(codec, b, W, H, n, win, t, dd, dg, call=CALL, what=what)
            compare(got, sr.expected(images, *win, dark, gain, t), what)
            assert torch.equal(res, b.results)


@pytest.mark.parametrize("W,H,n", [(200, 123, 4), (4200, 24, 2)])
def test_one_map_or_scalars_only(codec, o16, W, H, n):   # noqa: F811
    b = batch(codec, o16, "small", W, H, n)
    images = b.gpu_full
    dark, gain = maps16(images, 11)
    one = float(np.float32(1.0 / 65535.0))
    for d, g in ((dark, None), (None, gain), (dark, -0.75), (12.5, gain), (0.0, one), (100.25, 2.0), (None, None)):
        for win in windows(W, H)[:1] + windows(W, H)[-1:]:
            for t in sr.TYPES:
                what = f"{W}x{H} {win} {t} dark {type(d).__name__} gain {type(g).__name__}"
                got, _ = run(codec, b, W, H, n, win, t, d, g, call=CALL, what=what)
                want = sr.expected(images, *win, 0.0 if d is None else d, 1.0 if g is None else g, t)
                compare(got, want, what)


@pytest.mark.parametrize("W,H,n,rw,rh", [(200, 123, 9, 61, 37), (4200, 24, 4, 4150, 20), (64, 48, 6, 64, 48)])
def test_per_frame_origins_take_the_maps_at_clamped_frame_coordinates(codec, o16, W, H, n, rw, rh):   # noqa: F811
    import torch
    rng = np.random.default_rng(W + rw + 16)
    b = batch(codec, o16, "mixed", W, H, n)
    images = b.gpu_full
    dark, gain = maps16(images, 23)
    org = np.stack([rng.integers(-9, W + 9, n), rng.integers(-9, H + 9, n)], 1).astype(np.int32)
    org[0] = (-5, H + 100)
    org[1] = (W - rw, H - rh)
    moved = False
    for t in sr.TYPES:
        what = f"{W}x{H} origins window {rw}x{rh} {t}"
        got, res = run(codec, b, W, H, n, (0, 0, rw, rh), t, dark, gain, origins=org, call=CALL, what=what)
        compare(got, sr.expected(images, 0, 0, rw, rh, dark, gain, t, origins=org), what)
        assert torch.equal(res, b.results)
        if rw < W or rh < H:
            cl = sr.clamp_origins(org, W, H, rw, rh)
            wrong = np.stack([sr.scaled_bits(images[f, y:y + rh, x:x + rw], dark[:rh, :rw], gain[:rh, :rw], t)
                              for f, (x, y) in enumerate(cl)])
            moved = moved or not np.array_equal(wrong, got)
    assert moved or (rw == W and rh == H)


@pytest.mark.parametrize("slot", [False, True])
@pytest.mark.parametrize("shift", [0, 1, 6, 15])
def test_layouts_and_stream_bases(codec, o16, slot, shift):   # noqa: F811
    """Concatenated and slotted streams whose base sits at several residues mod 16; stream_bytes ends exactly at the
    last frame's last byte, with junk behind it."""
    import torch
    W, H, n = 203, 45, 3
    stride = (int(codec.L.dbde16_hip_max_frame_bytes(W, H)) + 255) // 256 * 256 + 24 if slot else 0
    b = batch(codec, o16, "full" if shift % 2 else "mixed", W, H, n, seed=shift, first=1, slot_stride=stride, shift=shift,
              junk=0x5A + shift)
    images = b.gpu_full
    dark, gain = maps16(images, shift)
    for win in [(0, 0, W, H), (3, 5, 197, 33), (W - 9, H - 3, 9, 3)]:
        for t in sr.TYPES:
            what = f"slot={slot} shift={shift} {win} {t}"
            got, res = run(codec, b, W, H, n, win, t, dark, gain, call=CALL, what=what)
            compare(got, sr.expected(images, *win, dark, gain, t), what)
            assert torch.equal(res, b.results)


@pytest.mark.parametrize("W,H,n,how", [(64, 48, 30, "concat"), (200, 123, 23, "residues"), (1921, 17, 9, "slots"),
                                       (8, 8, 70, "offsets")])
def test_crafted_and_rejected_frames(codec, W, H, n, how):
    import torch
    rng = np.random.default_rng(W * 7919 + H + 16)
    s = Crafted16(rng, W, H, n, how)
    keep = [im is not None for im in s.images]
    assert any(keep) and not all(keep)
    canvas = torch.full((n, H, W), 0x3333, dtype=torch.int16, device="cuda")
    images, want_res = codec.decode_frames16(s.buf, s.lead, s.total, s.offs, W, H, n, images=canvas)
    codec.sync()
    images = images.cpu().numpy().view(np.uint16)
    assert all((images[f] == s.images[f]).all() for f in range(n) if keep[f])
    dark, gain = maps16(np.stack([im for im in s.images if im is not None]), H)
    for k, win in enumerate(windows(W, H)):
        t = sr.TYPES[k % 3]
        what = f"crafted {how} {W}x{H} {win} {t}"
        got, res = run(codec, s, W, H, n, win, t, dark, gain, call=CALL, what=what)
        compare(got, sr.expected(images, *win, dark, gain, t), what, keep=keep, sentinel=SENT[got.itemsize])
        assert torch.equal(res, want_res)


def test_wrapping_minima_scale_as_decoded_values(codec):
    import torch
    rng = np.random.default_rng(6)
    W, H, n = 43, 27, 6
    frames = [cr.craft(rng, W, H, 16, "max", "max" if f % 2 else "boundary", "ones" if f % 3 else "random",
                       header=(2, f, 0)) for f in range(n)]
    images = np.stack([cr.decode_frame(fr, W, H, 16)[2] for fr in frames])
    buf, lead, offs, total = cr.layout(frames, "concat", lead=32)

    class S:
        pass
    s = S()
    s.buf, s.lead, s.total, s.offs = torch.from_numpy(buf).cuda(), lead, total, torch.from_numpy(offs).cuda()
    dark, gain = maps16(images, 5)
    for win in windows(W, H):
        for t in sr.TYPES:
            got, _ = run(codec, s, W, H, n, win, t, dark, gain, call=CALL)
            compare(got, sr.expected(images, *win, dark, gain, t), f"wrapping minima {win} {t}")


def test_zero_frames_and_argument_errors(dv, codec, o16):   # noqa: F811
    import torch
    W, H, n = 64, 48, 2
    b = batch(codec, o16, "mixed", W, H, n)
    args = (b.buf, b.lead, b.total, b.offs, W, H)
    o = Out(n, 41, 30, "bf16")
    codec.decode_scaled16(*args, 0, 5, 3, 41, 30, dtype=torch.bfloat16, out=o.t)
    codec.sync()
    assert (o.read() == SENT[2]).all(), "n == 0 wrote the output"
    out, res = codec.decode_scaled16(*args, 0, dtype=torch.float16)
    assert tuple(out.shape) == (0, H, W) and out.dtype == torch.float16 and tuple(res.shape) == (0, 4)
    good = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    for kw in (dict(dtype=torch.int16), dict(dark=good[:, :-1]), dict(gain=good.to(torch.bfloat16))):
        with pytest.raises(dv.DbdeError):
            codec.decode_scaled16(*args, n, **kw)
    raw = torch.zeros(4 * n * H * W + 16, dtype=torch.uint8, device="cuda")
    rc = codec.L.dbde16_hip_decode_scaled(codec.h, b.buf.data_ptr() + b.lead, b.total, b.offs.data_ptr(), W, H, n, 0, 0,
                                          W, H, None, dv.OUT_F32, None, 0.0, None, 1.0, raw.data_ptr() + 2, None)
    assert rc == dv.ERR_ARG
    rc = codec.L.dbde16_hip_decode_scaled(codec.h, b.buf.data_ptr() + b.lead, b.total, b.offs.data_ptr(), W, H, n, 0, 0,
                                          W, H, None, 3, None, 0.0, None, 1.0, raw.data_ptr(), None)
    assert rc == dv.ERR_ARG and (raw == 0).all()
    out, res = codec.decode_scaled16(*args, n)
    codec.sync()
    want = torch.from_numpy(b.gpu_full.astype(np.int32)).cuda().float()
    assert torch.equal(out, want) and torch.equal(res, b.results)
