"""GPU: DBDE16 binned decode -- dbde16_hip_decode_binned (Codec.decode_binned16).

Expected values are exact integers: tests/binned_ref.py's definition applied to the DBDE16 oracle's images of the
device-encoded bytes and to dbde16_hip_decode_frames' images (the two must agree).  Depths 0-16, 12-bit content,
minima that wrap modulo 2^16, rejected frames.  U32 sums, U16 maxima and minima; every plane sits at an odd element
offset inside a sentinel-filled buffer whose guard elements are checked.
"""
import numpy as np
import pytest

import binned_ref as br
from test_gpu_binned import ALL, BINS, SHAPES, Planes, compare
from test_gpu_histogram16 import twelve_bit
from test_gpu_roi16 import KINDS, Batch16, images16
from test_oracle_u16 import o16   # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

SENT16 = {"sum": 0x5A5A5A5A, "max": 0x5A5A, "min": 0x5A5A}
CONTENT = KINDS + ("twelve",)


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


def run16(dv, codec, b, bn, win, stats, buf=None, stream_bytes=None):
    x, y, rw, rh = win
    pl = Planes(dv, b.n, rw, rh, bn, stats, pix=2)
    out, res = codec.decode_binned16(b.buf if buf is None else buf, b.lead, b.total if stream_bytes is None else stream_bytes,
                                     b.offs, b.W, b.H, b.n, bn, x, y, rw, rh, out=pl.out)
    codec.sync()
    assert out is pl.out and (out.pixels.cpu().numpy() == br.bin_pixels(rw, rh, bn)).all()
    return pl.read(), res


@pytest.mark.parametrize("W,H,n", SHAPES)
def test_planes_match_binned_images(dv, codec, o16, W, H, n):
    rng = np.random.default_rng(W * 7919 + H * 31 + n)
    for i, kind in enumerate(CONTENT):
        if W * H > 10 ** 7 and kind not in ("mixed", "depth0", "twelve"):
            continue   # (4096 x 3072: three kinds; the oracle decodes every frame on the CPU)
        imgs = twelve_bit(rng, n, W, H) if kind == "twelve" else images16(rng, n, W, H, kind)
        b = Batch16(codec, o16, imgs, first=3 + i, shift=i)
        full = np.stack(b.full)
        assert (full == b.gpu_full).all()
        for bn in BINS:
            wins = br.windows(W, H, bn)
            assert len(wins) == 5 or min(W, H) < 12
            for win in wins:
                want = br.binned_reduceat(full, *win, bn)
                for stats in (ALL, ("sum",)):
                    got, res = run16(dv, codec, b, bn, win, stats)
                    compare(got, want, stats, f"{kind} {W}x{H} bin {bn} window {win} {stats}", sent=SENT16)
                    assert codec.parse_results(res) == [(2, b.first + f, 0, len(b.packed[f])) for f in range(n)]


def test_wrapping_minima(dv, codec, o16):
    """Minima raised so that min + value passes 65535: the planes reduce the U16 values dbde16_hip_decode_frames
    writes (modulo 2^16)."""
    import torch
    W, H, n = 61, 37, 3
    rng = np.random.default_rng(21)
    b = Batch16(codec, o16, images16(rng, n, W, H, "mixed"), first=7)
    T = ((W + 7) // 8) * ((H + 7) // 8)
    host = b.buf.cpu().numpy().copy()
    o = b.offs.cpu().numpy()
    for f in range(n):
        m0 = b.lead + int(o[f]) + 28 + T
        host[m0 + 1: m0 + 2 * T: 2] = 0xFF   # every minimum's high byte: min >= 0xFF00
    buf = torch.from_numpy(host).cuda()
    back, res = codec.decode_frames16(buf, b.lead, b.total, b.offs, W, H, n)
    codec.sync()
    assert [r[0] for r in codec.parse_results(res)] == [2] * n
    wrapped = back.cpu().numpy().view(np.uint16)
    assert (wrapped != b.gpu_full).any() and (wrapped < 0xFF00).any()
    for bn in BINS:
        for win in br.windows(W, H, bn):
            got, _ = run16(dv, codec, b, bn, win, ALL, buf=buf)
            compare(got, br.binned_reduceat(wrapped, *win, bn), ALL, f"wrapping bin {bn} {win}", sent=SENT16)


@pytest.mark.parametrize("slot", [0, 4096 * 3 * 2 + 7])
def test_layouts_and_stream_end(dv, codec, o16, slot):
    W, H, n = 203, 19, 3
    for shift in (0, 5, 11):
        rng = np.random.default_rng(300 + shift)
        b = Batch16(codec, o16, images16(rng, n, W, H, "full"), slot_stride=slot, shift=shift, junk=0x5A + shift)
        full = np.stack(b.full)
        for bn in BINS:
            for win in [(0, 0, W, H), (bn, bn, 193, 11)]:
                got, _ = run16(dv, codec, b, bn, win, ALL)
                compare(got, br.binned_reduceat(full, *win, bn), ALL, f"slot {slot} shift {shift} bin {bn}", sent=SENT16)


def test_rejected_frames_keep_their_planes(dv, codec, o16):
    """Depth byte 17, nm == T, an n64 mismatch and a truncated last frame: their planes keep the sentinel; results
    equal dbde16_hip_decode_frames'."""
    import torch
    W, H, n = 61, 37, 5
    rng = np.random.default_rng(9)
    b = Batch16(codec, o16, images16(rng, n, W, H, "mixed"), first=40)
    T = ((W + 7) // 8) * ((H + 7) // 8)
    o = b.offs.cpu().numpy()
    host = b.buf.cpu().numpy()
    base = b.lead
    host[base + o[0] + 24 + 3] = 17
    host[base + o[1] + 24 + T: base + o[1] + 28 + T] = np.frombuffer(np.int32(T).tobytes(), np.uint8)
    n64 = base + o[3] + 28 + 3 * T
    host[n64: n64 + 4] = np.frombuffer(np.int32(int(host[n64: n64 + 4].view("<i4")[0]) + 1).tobytes(), np.uint8)
    buf = torch.from_numpy(host).cuda()
    truncated = b.total - 1
    _, want_res = codec.decode_frames16(buf, b.lead, truncated, b.offs, W, H, n)
    codec.sync()
    keep = [False, False, True, False, False]
    full = np.stack(b.full)
    for bn in BINS:
        for win in br.windows(W, H, bn):
            got, res = run16(dv, codec, b, bn, win, ALL, buf=buf, stream_bytes=truncated)
            compare(got, br.binned_reduceat(full, *win, bn), ALL, f"rejected bin {bn} {win}", keep=keep, sent=SENT16)
            assert torch.equal(res, want_res)


def test_zero_frames_absent_planes_and_errors(dv, codec, o16):
    import torch
    W, H, n = 64, 48, 2
    rng = np.random.default_rng(1)
    b = Batch16(codec, o16, images16(rng, n, W, H, "mixed"))
    full = np.stack(b.full)
    pl = Planes(dv, n, W, H, 2, ALL, pix=2)
    codec.decode_binned16(b.buf, b.lead, b.total, b.offs, W, H, 0, 2, out=pl.out)
    codec.sync()
    got = pl.read()
    assert all((got[s] == SENT16[s]).all() for s in ALL)
    for stats in (("max",), ("sum", "min")):
        got, _ = run16(dv, codec, b, 4, (4, 4, 55, 41), stats)
        compare(got, br.binned_reduceat(full, 4, 4, 55, 41, 4), stats, f"planes {stats}", sent=SENT16)
    out, _ = codec.decode_binned16(b.buf, b.lead, b.total, b.offs, W, H, n, 8, stats=ALL)
    codec.sync()
    assert out.sum.dtype == torch.int32 and out.max.dtype == torch.int16 and tuple(out.min.shape) == (n, 6, 8)
    assert (out.max.cpu().numpy().view(np.uint16) == br.binned_reduceat(full, 0, 0, W, H, 8)["max"]).all()
    for kw in (dict(bin=3), dict(bin=4, x=2), dict(bin=8, y=4), dict(bin=2, rw=65), dict(bin=2, stats=())):
        bn = kw.pop("bin")
        with pytest.raises((dv.DbdeError, ValueError)):
            codec.decode_binned16(b.buf, b.lead, b.total, b.offs, W, H, n, bn, **kw)
    raw = torch.zeros(4 * n * 24 * 32 + 4, dtype=torch.uint8, device="cuda")
    for k, args in enumerate(((raw.data_ptr() + 2, None, None), (None, raw.data_ptr() + 1, None),
                              (None, None, raw.data_ptr() + 1))):   # U32 sums at 2 mod 4, U16 planes at odd addresses
        rc = codec.L.dbde16_hip_decode_binned(codec.h, b.buf.data_ptr() + b.lead, b.total, b.offs.data_ptr(), W, H, n,
                                              0, 0, W, H, 2, *args, None)
        assert rc == dv.ERR_ARG, k
