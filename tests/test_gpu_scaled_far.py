"""GPU: the scaled float decode at stream offsets past 2^31 and 2^32 bytes and with an output past 2^32 bytes.

The buffers follow tests/far.py's layout rules (a sentinel lead in front of every buffer a kernel is given, a tail
behind it, every offset below 2^33), so a narrowed offset lands inside the test's own allocation: on a decoy frame, on
sentinel bytes or on the wrong output element, and the test fails with wrong values rather than a fault.

1. decode_scaled and decode_scaled16 read the six far placements of far.SLOTS, once for each field that crosses 2^32,
   with both maps, fixed and per-frame origins; every output lies in a far.guarded buffer.  Expected:
   tests/scaled_ref.py over the oracle's decode of every frame; the same call on a near copy of the stream, element
   for element; rejected entries keep the sentinel; results rows are the real frames' (a decoy's index would show).
2. An F32 output past 2^32 bytes: 90 windows of 4096 x 3072 (4.53 GB) from repeated offsets of three smooth frames.
   Frame 43 starts past 2^31 bytes, frame 86 past 2^32 bytes.  A handful of frames are compared on the device with
   ((p.float() - dark) * gain) of torch, one of them on the host with tests/scaled_ref.py; the lead and the tail are
   checked for writes.
"""
import numpy as np
import pytest

import far
import scaled_ref as sr
from test_gpu_far_offsets import (assert_rows, assert_same, codec, device_memory, dv, far_and_near,   # noqa: F401
                                  frames_of)
from test_oracle_u16 import o16   # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

G31, G32 = far.G31, far.G32
S8 = far.SENTINEL


@pytest.mark.parametrize("bits,W,H,n", [(8, 200, 123, 13), (8, 1024, 768, 6), (16, 200, 123, 13), (16, 1024, 768, 6)])
def test_scaled_far(dv, codec, oracle, o16, bits, W, H, n):   # noqa: F811
    import torch
    fr = frames_of(oracle, o16, W, H, bits)
    rng = np.random.default_rng(W + n + bits)
    fn = codec.decode_scaled if bits == 8 else codec.decode_scaled16
    dark, gain = sr.maps(bits + W, W, H)
    dd, dg = torch.from_numpy(dark).cuda(), torch.from_numpy(gain).cuda()
    k = 0
    for (x, y, rw, rh), per_frame in (((W // 3, H // 5, W // 2, H // 3), True), ((0, 0, W, H), False),
                                      ((W - 9, 1, 9, H - 2), False)):
        org = None
        if per_frame:
            org = np.stack([rng.integers(-3, W + 3, n), rng.integers(-3, H + 3, n)], 1).astype(np.int32)
        for straddle, lay in fr.layouts.items():
            t = sr.TYPES[k % 3]
            k += 1
            ents = far.entries(n)

            def call(s):
                g = far.guarded((n, rh, rw), sr.torch_dtype(t))
                _, res = fn(s.buf, s.lead, s.stream_bytes, s.offs, W, H, n, x, y, rw, rh, dtype=sr.torch_dtype(t),
                            dark=dd, gain=dg, origins=None if org is None else torch.from_numpy(org).cuda(), out=g.t)
                codec.sync()
                g.check(f"scaled {bits}-bit {straddle}")
                return g.t.view(torch.int32 if t == "f32" else torch.int16), res

            got, near = far_and_near(lay, ents, call)
            what = f"{bits}-bit scaled {W}x{H} window {(x, y, rw, rh)} per-frame {per_frame} {t} {straddle}"
            assert_same(got, near, what)
            refs = fr.refs(lay, ents)
            assert_rows(codec, got[1], refs, what)
            win = got[0].cpu().numpy().view(sr.BITS[t])
            sent = S8 * (0x01010101 if t == "f32" else 0x0101)
            for f, (_, img) in enumerate(refs):
                if img is None:
                    assert (win[f] == sent).all(), f"{what}: rejected entry {f}'s window was written"
                    continue
                want = sr.expected(img[None], x, y, rw, rh, dark, gain, t, origins=None if org is None else org[f:f + 1])
                assert np.array_equal(win[f], want[0]), f"{what}: entry {f}"
            del got, near


def test_f32_output_past_4gib(dv, codec):   # noqa: F811
    import torch
    W, H, k, n = 4096, 3072, 3, 90
    src = far.guarded((k, H, W), torch.uint8)
    codec.synth_frames("smooth", 0x5CA1ED, 0, k, W, H, out=src.t)
    cap = k * dv.max_frame_bytes(W, H)
    stream = far.guarded((cap,), torch.uint8)
    offs, sizes = codec.encode_frames(src.t, W, H, k, stream.buf, stream.lead, cap)
    codec.sync()
    total = int((offs[-1] + sizes[-1]).item())
    rep, rsz = offs.repeat(n // k), sizes.repeat(n // k)
    plan = dv.scaled_plan(W, H, n)
    frame_bytes = W * H * 4
    assert plan["out_bytes"] == n * frame_bytes > G32 and 42 * frame_bytes < G31 < 43 * frame_bytes
    assert 85 * frame_bytes < G32 < 86 * frame_bytes
    dark, gain = sr.maps(90, W, H, pixels=src.t[1].cpu().numpy())
    dd, dg = torch.from_numpy(dark).cuda(), torch.from_numpy(gain).cuda()
    out = far.guarded((n, H, W), torch.float32)
    _, res = codec.decode_scaled(stream.buf, stream.lead, total, rep, W, H, n, dark=dd, gain=dg, out=out.t)
    codec.sync()
    out.check("F32 windows")
    assert torch.equal(res[:, 3], rsz)
    for f in (0, 1, 42, 43, 44, 85, 86, 87, 89):
        want = (src.t[f % k].float() - dd) * dg
        assert torch.equal(out.t[f].view(torch.int32), want.view(torch.int32)), f"frame {f} (starts at byte {f * frame_bytes})"
    host = sr.expected(src.t[89 % k].cpu().numpy()[None], 0, 0, W, H, dark, gain, "f32")
    assert np.array_equal(out.t[89].cpu().numpy().view(np.uint32), host[0])
