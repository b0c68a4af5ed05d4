"""GPU: the compressed-domain crop at stream offsets past 2^31 and 2^32 bytes, and into output slots past them.

The buffers follow tests/far.py's layout rules (a sentinel lead in front of every buffer a kernel is given, a tail
behind it, every offset below 2^33), so a narrowed offset lands inside the test's own allocation: on a decoy frame or on
sentinel bytes, and the test fails with wrong bytes rather than a fault.

1. crop_frames and crop_frames16 read the six far placements of far.SLOTS, once for each field that crosses 2^32.
   Expected: tests/crop_ref.py of every distinct frame; the same call on a near copy of the stream, byte for byte;
   rejected entries write nothing; results rows are the real frames' (a decoy's index would show).
2. Output slots at 0, 2^31 + 2^20 and 2^32 + 2^21 for both formats: every frame equals the model's, and every other
   byte of the allocation keeps the sentinel.
"""
import numpy as np
import pytest

import crop_ref
import far
from test_gpu_far_offsets import (assert_rows, assert_same, check_untouched, codec, device_memory, dv,   # noqa: F401
                                  far_and_near, frames_of, slot_stride)
from test_oracle_u16 import o16   # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu


def crop_fn(codec, bits):   # noqa: F811
    return codec.crop_frames if bits == 8 else codec.crop_frames16


@pytest.mark.parametrize("bits,W,H,n", [(8, 200, 123, 13), (8, 1024, 768, 6), (16, 200, 123, 13), (16, 1024, 768, 6)])
def test_crop_far(dv, codec, oracle, o16, bits, W, H, n):   # noqa: F811
    import torch
    fr = frames_of(oracle, o16, W, H, bits)
    for (x, y, rw, rh), stride_extra in (((0, 0, W, H), None), ((8, 16, W - 11, H - 19), 5), ((96, 64, 64, 48), None)):
        maxf = crop_ref.max_frame_bytes(rw, rh, bits)
        stride = maxf + stride_extra if stride_extra is not None else 0
        cap = (n - 1) * stride + maxf if stride else n * maxf
        model = {}
        for straddle, lay in fr.layouts.items():
            ents = far.entries(n)

            def call(s):
                g = far.guarded((cap,), torch.uint8)
                o, b, res = crop_fn(codec, bits)(s.buf, s.lead, s.stream_bytes, s.offs, W, H, n, x, y, rw, rh, g.buf,
                                                 g.lead, cap, slot_stride=stride)
                codec.sync()
                g.check(f"{bits}-bit crop {straddle}")
                return g.t, o, b, res

            got, near = far_and_near(lay, ents, call)
            what = f"{bits}-bit crop {W}x{H} window {(x, y, rw, rh)} {straddle}"
            assert_same(got, near, what)
            refs = fr.refs(lay, ents)
            assert_rows(codec, got[3], refs, what)
            out, o, b = got[0], got[1].cpu().numpy(), got[2].cpu().numpy()
            at, spans = 0, []
            for f, (_, img) in enumerate(refs):
                src = lay.frames[ents[f]]
                assert int(o[f]) == (f * stride if stride else at), (what, f)
                if img is None:
                    assert int(b[f]) == 0, f"{what}: rejected entry {f} wrote a frame"
                    continue
                if id(src) not in model:
                    model[id(src)] = crop_ref.crop_frame(src[:crop_ref.frame_length(src, W, H, bits)], W, H, x, y, rw,
                                                         rh, bits)
                want = model[id(src)]
                assert int(b[f]) == len(want), (what, f)
                assert out[int(o[f]): int(o[f]) + len(want)].cpu().numpy().tobytes() == want.tobytes(), f"{what}: entry {f}"
                spans.append((int(o[f]), int(o[f]) + len(want)))
                at += len(want)
            p = 0
            for s0, s1 in spans + [(cap, cap)]:
                assert far.all_equal(out[p:s0], far.SENTINEL), f"{what}: bytes in [{p}, {s0}) were written"
                p = s1
            del got, near


@pytest.mark.parametrize("bits,W,H", [(8, 1921, 1081), (8, 200, 123), (16, 1024, 768), (16, 33, 31)])
def test_crop_writes_far_slots(dv, codec, oracle, o16, bits, W, H):   # noqa: F811
    import torch
    n, stride = 3, slot_stride(3)
    fr = frames_of(oracle, o16, W, H, bits) if (W, H) in ((200, 123), (1024, 768)) else None
    if fr is not None:
        frames = [f for f in next(iter(fr.layouts.values())).frames if crop_ref.frame_valid(f, W, H, bits)][:n]
    else:
        rng = np.random.default_rng(W)
        if bits == 8:
            frames = [oracle.pack_frame((1 << 33) + k, rng.integers(0, 256, (H, W), dtype=np.uint8) >> (2 * k), W, H)
                      for k in range(n)]
        else:
            from test_oracle_u16 import pack16
            frames = [pack16(o16, (rng.integers(0, 65536, (H, W)) >> (5 * k)).astype(np.uint16), (1 << 33) + k)
                      for k in range(n)]
    assert len(frames) == n
    import crafted
    host, lead, offs, total = crafted.layout(frames, "residues", lead=32)
    buf, offs = torch.from_numpy(host).cuda(), torch.from_numpy(offs).cuda()
    x, y, rw, rh = 8, 8, W - 13, H - 10
    maxf = crop_ref.max_frame_bytes(rw, rh, bits)
    cap = (n - 1) * stride + maxf
    out = far.guarded((cap,), torch.uint8)
    o, b, _ = crop_fn(codec, bits)(buf, lead, total, offs, W, H, n, x, y, rw, rh, out.buf, out.lead, cap,
                                   slot_stride=stride)
    codec.sync()
    o, b = o.cpu().numpy(), b.cpu().numpy()
    assert [int(v) for v in o] == [f * stride for f in range(n)] and far.G31 < int(o[1]) < far.G32 < int(o[2])
    for f in range(n):
        want = crop_ref.crop_frame(frames[f], W, H, x, y, rw, rh, bits)
        assert int(b[f]) == len(want), f
        assert out.t[int(o[f]): int(o[f]) + len(want)].cpu().numpy().tobytes() == want.tobytes(), f"frame {f} at {int(o[f])}"
    check_untouched(out.buf, out.lead, [(int(a), int(a) + int(c)) for a, c in zip(o, b)], f"{bits}-bit {W}x{H}")
