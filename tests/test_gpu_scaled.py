"""GPU: scaled float decode -- dbde_hip_decode_scaled (Codec.decode_scaled).

Expected values are tests/scaled_ref.py's definition, ((float32)p - D) * G rounded once to the output type, applied to
the images dbde_hip_decode_frames writes for the same frames, and compared as BIT PATTERNS (-0, inf and subnormals
count).  The maps are scaled_ref's standard ones (never constant, so a kernel that indexed them by window coordinates
would fail).  Every output starts GUARD + odd elements into a sentinel-filled buffer whose guards are checked, which
also puts it off 16-byte alignment.  Results rows are compared with what dbde_hip_decode_frames reports.
"""
import numpy as np
import pytest

import crafted as cr
import scaled_ref as sr
from test_gpu_project import Batch, Crafted, windows

pytestmark = pytest.mark.gpu

GUARD = 40
SENT = {4: 0x5A5A5A5A, 2: 0x5A5A}
SHAPES = [(200, 123, 7), (1, 1, 5), (8, 8, 9), (9, 9, 9), (1921, 1081, 2), (4200, 24, 3), (4096, 3072, 2)]


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


class Out:
    """An (n, rh, rw) output of type t that starts GUARD + odd elements into a sentinel-filled buffer."""

    def __init__(self, n, rw, rh, t, odd=1):
        import torch
        es = 4 if t == "f32" else 2
        self.es, self.lo, self.count = es, GUARD + odd, n * rw * rh
        self.buf = torch.full((2 * GUARD + odd + self.count,), SENT[es], dtype=torch.int32 if es == 4 else torch.int16,
                              device="cuda")
        self.t = self.buf[self.lo: self.lo + self.count].view(sr.torch_dtype(t)).view(n, rh, rw)
        assert self.t.data_ptr() % 16 != 0 and self.t.data_ptr() % es == 0
        self.shape = (n, rh, rw)

    def read(self, what=""):
        """The output's bit patterns (n, rh, rw), after checking the guards."""
        h = self.buf.cpu().numpy().view(np.uint32 if self.es == 4 else np.uint16)
        hi = self.lo + self.count
        assert (h[:self.lo] == SENT[self.es]).all(), f"{what}: wrote in front of the output"
        assert (h[hi:] == SENT[self.es]).all(), f"{what}: wrote behind the output"
        return h[self.lo:hi].reshape(self.shape)


def dev(a):
    """A map (numpy (H, W) float32), a scalar or None as Codec.decode_scaled takes it."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda() if isinstance(a, np.ndarray) else a


def run(codec, src, W, H, n, win, t, dark, gain, origins=None, call="decode_scaled", what=""):
    """src: anything with .buf, .lead, .total, .offs.  -> (bit patterns (n, rh, rw), results)."""
    import torch
    x, y, rw, rh = win
    o = Out(n, rw, rh, t)
    org = None if origins is None else torch.from_numpy(np.asarray(origins, np.int32).reshape(n, 2)).cuda()
    out, res = getattr(codec, call)(src.buf, src.lead, src.total, src.offs, W, H, n, x, y, rw, rh,
                                    dtype=sr.torch_dtype(t), dark=dev(dark), gain=dev(gain), origins=org, out=o.t)
    codec.sync()
    assert out is o.t
    return o.read(what), res


def compare(got, want, what, keep=None, sentinel=None):
    for f in range(got.shape[0]):
        if keep is not None and not keep[f]:
            assert (got[f] == sentinel).all(), f"{what}: rejected frame {f}'s window was written"
            continue
        if not np.array_equal(got[f], want[f]):
            j, i = np.argwhere(got[f] != want[f])[0]
            raise AssertionError(f"{what}: frame {f} differs at row {j} column {i}: "
                                 f"{int(got[f][j, i]):#x} != {int(want[f][j, i]):#x} "
                                 f"({int((got[f] != want[f]).sum())} of {got[f].size} elements)")


def both_maps(images, seed):
    n, H, W = images.shape
    return sr.maps(seed, W, H, pixels=images[0])


@pytest.mark.parametrize("mode", ("mixed", "noise8"))
@pytest.mark.parametrize("W,H,n", SHAPES)
def test_windows_in_all_types_with_both_maps(codec, mode, W, H, n):
    import torch
    bt = Batch(codec, mode, W, H, n)
    images = bt.images.cpu().numpy()
    dark, gain = both_maps(images, W + H)
    dd, dg = dev(dark), dev(gain)
    for win in windows(W, H):
        for t in sr.TYPES:
            what = f"{mode} {W}x{H} window {win} {t}"
            got, res = run(codec, bt, W, H, n, win, t, dd, dg, what=what)
            compare(got, sr.expected(images, *win, dark, gain, t), what)
            assert torch.equal(res, bt.results)


@pytest.mark.parametrize("W,H,n", [(200, 123, 7), (4200, 24, 3)])
def test_one_map_or_scalars_only(codec, W, H, n):
    bt = Batch(codec, "mixed", W, H, n)
    images = bt.images.cpu().numpy()
    dark, gain = both_maps(images, 11)
    one255 = float(np.float32(1.0 / 255.0))
    for d, g in ((dark, None), (None, gain), (dark, -0.75), (12.5, gain), (0.0, one255), (12.5, -3.0), (None, None)):
        for win in windows(W, H)[:1] + windows(W, H)[-1:]:
            for t in sr.TYPES:
                what = f"{W}x{H} {win} {t} dark {type(d).__name__} gain {type(g).__name__}"
                got, _ = run(codec, bt, W, H, n, win, t, d, g, what=what)
                want = sr.expected(images, *win, 0.0 if d is None else d, 1.0 if g is None else g, t)
                compare(got, want, what)
    # plain 1/255 scaling of a U8 frame in F32: exactly the torch expression
    got, _ = run(codec, bt, W, H, n, (0, 0, W, H), "f32", 0.0, one255)
    want = (bt.images.float() * one255).cpu().numpy().view(np.uint32)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("W,H,n,rw,rh", [(200, 123, 9, 61, 37), (4200, 24, 5, 4150, 20), (64, 48, 6, 64, 48),
                                         (1921, 1081, 3, 700, 9)])
def test_per_frame_origins_take_the_maps_at_clamped_frame_coordinates(codec, W, H, n, rw, rh):
    import torch
    rng = np.random.default_rng(W + rw)
    bt = Batch(codec, "mixed", W, H, n)
    images = bt.images.cpu().numpy()
    dark, gain = both_maps(images, 23)
    org = np.stack([rng.integers(-9, W + 9, n), rng.integers(-9, H + 9, n)], 1).astype(np.int32)
    org[0] = (-5, H + 100)
    org[1] = (W - rw, H - rh)
    org[2] = (min(3, W - rw), min(5, H - rh))
    moved = False
    for t in sr.TYPES:
        what = f"{W}x{H} origins window {rw}x{rh} {t}"
        got, res = run(codec, bt, W, H, n, (0, 0, rw, rh), t, dark, gain, origins=org, what=what)
        compare(got, sr.expected(images, 0, 0, rw, rh, dark, gain, t, origins=org), what)
        assert torch.equal(res, bt.results)
        if rw < W or rh < H:   # the maps at window coordinates would give other values: the test can tell
            cl = sr.clamp_origins(org, W, H, rw, rh)
            wrong = np.stack([sr.scaled_bits(images[f, y:y + rh, x:x + rw], dark[:rh, :rw], gain[:rh, :rw], t)
                              for f, (x, y) in enumerate(cl)])
            moved = moved or not np.array_equal(wrong, got)
    assert moved or (rw == W and rh == H)


@pytest.mark.parametrize("slot,misalign", [(0, 1), (0, 3), (4096 * 3 + 5, 0), (20000, 2)])
def test_layouts(codec, slot, misalign):
    """Concatenated streams at misaligned leads and slot layouts; stream_bytes ends exactly at the last frame."""
    import torch
    W, H, n = 100, 75, 11
    bt = Batch(codec, "mixed", W, H, n, slot_stride=slot, misalign=misalign)
    images = bt.images.cpu().numpy()
    dark, gain = both_maps(images, slot + misalign)
    for win in [(0, 0, W, H), (3, 2, 95, 70)]:
        for t in sr.TYPES:
            what = f"slot {slot} misalign {misalign} {win} {t}"
            got, res = run(codec, bt, W, H, n, win, t, dark, gain, what=what)
            compare(got, sr.expected(images, *win, dark, gain, t), what)
            assert torch.equal(res, bt.results)


@pytest.mark.parametrize("W,H,n,how", [(64, 48, 40, "concat"), (200, 123, 23, "residues"), (1921, 17, 9, "slots"),
                                       (8, 8, 70, "offsets"), (4200, 9, 7, "concat")])
def test_crafted_and_rejected_frames(codec, W, H, n, how):
    """Every depth, wrapping minima, random payload; rejected windows keep the sentinel, results are decode_frames'."""
    import torch
    rng = np.random.default_rng(W * 7919 + H)
    s = Crafted(rng, W, H, n, how)
    keep = [im is not None for im in s.images]
    assert any(keep) and not all(keep)
    canvas = torch.full((n, H, W), 0x33, dtype=torch.uint8, device="cuda")
    images, want_res = codec.decode_frames(s.buf, s.lead, s.total, s.offs, W, H, n, images=canvas)
    codec.sync()
    images = images.cpu().numpy()
    assert all((images[f] == s.images[f]).all() for f in range(n) if keep[f])
    dark, gain = both_maps(np.stack([im for im in s.images if im is not None]), H)
    for k, win in enumerate(windows(W, H)):
        t = sr.TYPES[k % 3]
        what = f"crafted {how} {W}x{H} {win} {t}"
        got, res = run(codec, s, W, H, n, win, t, dark, gain, what=what)
        compare(got, sr.expected(images, *win, dark, gain, t), what, keep=keep, sentinel=SENT[got.itemsize])
        assert torch.equal(res, want_res)


def test_wrapping_minima_scale_as_decoded_bytes(codec):
    import torch
    rng = np.random.default_rng(5)
    W, H, n = 43, 27, 6
    frames = [cr.craft(rng, W, H, 8, "max", "max" if f % 2 else "boundary", "ones" if f % 3 else "random",
                       header=(2, f, 0)) for f in range(n)]
    images = np.stack([cr.decode_frame(fr, W, H)[2] for fr in frames])
    buf, lead, offs, total = cr.layout(frames, "concat", lead=32)

    class S:
        pass
    s = S()
    s.buf, s.lead, s.total, s.offs = torch.from_numpy(buf).cuda(), lead, total, torch.from_numpy(offs).cuda()
    dark, gain = both_maps(images, 5)
    for win in windows(W, H):
        for t in sr.TYPES:
            got, _ = run(codec, s, W, H, n, win, t, dark, gain)
            compare(got, sr.expected(images, *win, dark, gain, t), f"wrapping minima {win} {t}")


def test_special_values_in_the_maps_propagate(codec):
    W, H, n = 40, 24, 2
    bt = Batch(codec, "noise8", W, H, n)
    images = bt.images.cpu().numpy()
    dark, gain = both_maps(images, 1)
    gain[3, 5], gain[4, 6], dark[5, 7], dark[6, 8] = np.inf, -np.inf, np.inf, np.nan
    gain[7, 9] = np.nan
    for t in sr.TYPES:
        got, _ = run(codec, bt, W, H, n, (0, 0, W, H), t, dark, gain)
        want = sr.expected(images, 0, 0, W, H, dark, gain, t)
        top = 0x7F800000 if t == "f32" else (0x7C00 if t == "f16" else 0x7F80)
        mag = 0x7FFFFFFF if t == "f32" else 0x7FFF
        isnan = (want & mag) > top
        assert isnan[:, 6, 8].all() and isnan[:, 7, 9].all() and isnan.sum() >= 2 * n
        assert (((got & mag) > top) == isnan).all(), "NaN where the definition has NaN (payload bits unspecified)"
        assert np.array_equal(got[~isnan], want[~isnan])
        assert ((want[:, 3, 5] & mag) == top).all() and ((want[:, 5, 7] & mag) == top).all(), "infinities"


def test_zero_frames_defaults_and_timing_slots(dv, codec):
    import torch
    W, H, n = 200, 123, 4
    bt = Batch(codec, "mixed", W, H, n)
    o = Out(n, 191, 113, "f16")
    codec.decode_scaled(bt.buf, bt.lead, bt.total, bt.offs, W, H, 0, 8, 8, 191, 113, dtype=torch.float16, out=o.t)
    codec.sync()
    assert (o.read() == SENT[2]).all(), "n == 0 wrote the output"
    out, res = codec.decode_scaled(bt.buf, bt.lead, bt.total, bt.offs, W, H, 0, dtype=torch.bfloat16)
    assert tuple(out.shape) == (0, H, W) and out.dtype == torch.bfloat16 and tuple(res.shape) == (0, 4)
    with pytest.raises((dv.DbdeError, ValueError)):
        codec.decode_scaled(bt.buf, bt.lead, bt.total, bt.offs, W, H, 0, 8, 8, 193, 113)
    # defaults: the whole frame as float32, dark 0 and gain 1
    out, res = codec.decode_scaled(bt.buf, bt.lead, bt.total, bt.offs, W, H, n)
    codec.sync()
    assert out.dtype == torch.float32 and torch.equal(out, bt.images.float()) and torch.equal(res, bt.results)
    codec.timing(True)
    codec.timing_read(reset=True)
    codec.decode_scaled(bt.buf, bt.lead, bt.total, bt.offs, W, H, n, dtype=torch.float16, gain=0.5)
    t = codec.timing_read(reset=True)
    codec.timing(False)
    assert [t[k][1] for k in ("encode", "decode_index", "decode", "scan")] == [0, 1, 1, 0]


def test_argument_errors_leave_the_codec_usable(dv, codec):
    import torch
    W, H, n = 64, 48, 2
    bt = Batch(codec, "mixed", W, H, n)
    args = (bt.buf, bt.lead, bt.total, bt.offs, W, H, n)
    good = torch.zeros((H, W), dtype=torch.float32, device="cuda")
    for kw in (dict(dtype=torch.float64), dict(dtype=torch.uint8), dict(dark=torch.zeros((H, W + 1), device="cuda")),
               dict(gain=torch.zeros((W, H), device="cuda")), dict(dark=good.double()), dict(gain=good.half()),
               dict(gain=torch.zeros((H, 2 * W), device="cuda")[:, ::2]), dict(dtype=torch.float16, out=good.new_zeros((n, H, W))),
               dict(out=good.new_zeros((n, H, W - 1))), dict(out=good.new_zeros((n, H, 2 * W))[:, :, ::2]),
               dict(out=torch.zeros((n, H, W)))):   # too small, strided, on the host
        with pytest.raises(dv.DbdeError):
            codec.decode_scaled(*args, **kw)
    for kw in (dict(x=1, rw=64), dict(rw=65), dict(rh=0), dict(x=60, rw=8)):
        with pytest.raises((dv.DbdeError, ValueError)):
            codec.decode_scaled(*args, **kw)
    raw = torch.zeros(4 * n * H * W + 16, dtype=torch.uint8, device="cuda")
    L, ptr = codec.L, bt.buf.data_ptr() + bt.lead

    def c_call(out_type, out_ptr, dark_ptr=None, gain_ptr=None):
        return L.dbde_hip_decode_scaled(codec.h, ptr, bt.total, bt.offs.data_ptr(), W, H, n, 0, 0, W, H, None, out_type,
                                        dark_ptr, 0.0, gain_ptr, 1.0, out_ptr, None)
    for bad in (3, -1, 99):
        assert c_call(bad, raw.data_ptr()) == dv.ERR_ARG
    assert c_call(dv.OUT_F32, raw.data_ptr() + 2) == dv.ERR_ARG      # F32 output at 2 mod 4
    assert c_call(dv.OUT_F16, raw.data_ptr() + 1) == dv.ERR_ARG      # F16 / BF16 output at an odd address
    assert c_call(dv.OUT_BF16, raw.data_ptr() + 3) == dv.ERR_ARG
    assert c_call(dv.OUT_F32, None) == dv.ERR_ARG                    # NULL output with frames to write
    assert c_call(dv.OUT_F32, raw.data_ptr(), dark_ptr=good.data_ptr() + 2) == dv.ERR_ARG   # misaligned maps
    assert c_call(dv.OUT_F32, raw.data_ptr(), gain_ptr=good.data_ptr() + 1) == dv.ERR_ARG
    with pytest.raises(dv.DbdeError):
        codec._check(c_call(dv.OUT_F32, raw.data_ptr() + 2), "dbde_hip_decode_scaled")
    assert (raw == 0).all()
    # the next valid call on the same codec succeeds
    out, res = codec.decode_scaled(*args, dtype=torch.float16, dark=good, gain=2.0)
    codec.sync()
    assert torch.equal(out, (bt.images.float() * 2.0).half()) and torch.equal(res, bt.results)
    assert c_call(dv.OUT_F16, raw.data_ptr() + 2) == dv.OK           # 2-byte aligned is enough for F16
    codec.sync()
    assert torch.equal(raw[2:2 + 2 * n * H * W].view(torch.float16).view(n, H, W), bt.images.half())
