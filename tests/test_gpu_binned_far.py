"""GPU: the binned decode at stream offsets past 2^31 and 2^32 bytes and with planes past 2^32 bytes.

The buffers follow tests/far.py's layout rules (a sentinel lead in front of every buffer a kernel is given, a tail
behind it, every offset below 2^33), so a narrowed offset lands inside the test's own allocation: on a decoy frame, on
sentinel bytes or on the wrong plane element, and the test fails with wrong values rather than a fault.

1. decode_binned and decode_binned16 read the six far placements of far.SLOTS, once for each field that crosses 2^32,
   at bins of 2 and 8; every plane lies in a far.guarded buffer.  Expected: tests/binned_ref.py over the oracle's decode
   of every distinct frame; the same call on a near copy of the stream, element for element; rejected entries keep the
   sentinel; results rows are the real frames' (a decoy's index would show).
2. Planes past 2^32 bytes: repeated offsets of three 4096 x 3072 frames at a bin of 2, the sum plane only: 700 U16
   planes (4.40 GB) and 350 DBDE16 U32 planes (4.40 GB), each compared with its source frame's expected plane.
"""
import numpy as np
import pytest

import binned_ref as br
import far
from test_gpu_far_offsets import (assert_rows, assert_same, codec, device_memory, dv, far_and_near,   # noqa: F401
                                  frames_of)
from test_oracle_u16 import o16   # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

G32 = far.G32
S8 = far.SENTINEL
ALL = ("sum", "max", "min")


def plane_types(bits):
    """{stat: (torch dtype, numpy view, sentinel element)} of the planes."""
    import torch
    if bits == 8:
        return {"sum": (torch.int16, np.uint16, S8 * 0x0101), "max": (torch.uint8, np.uint8, S8),
                "min": (torch.uint8, np.uint8, S8)}
    return {"sum": (torch.int32, np.uint32, S8 * 0x01010101), "max": (torch.int16, np.uint16, S8 * 0x0101),
            "min": (torch.int16, np.uint16, S8 * 0x0101)}


@pytest.mark.parametrize("bits,W,H,n", [(8, 200, 123, 13), (8, 1024, 768, 6), (16, 200, 123, 13), (16, 1024, 768, 6)])
def test_binned_far(dv, codec, oracle, o16, bits, W, H, n):   # noqa: F811
    fr = frames_of(oracle, o16, W, H, bits)
    types = plane_types(bits)
    fn = codec.decode_binned if bits == 8 else codec.decode_binned16
    for b, (x, y, rw, rh) in ((2, (0, 0, W, H)), (8, (8, 16, W - 11, H - 19)), (2, (2, 6, W - 5, H - 9)), (8, (0, 0, W, H))):
        oh, ow = br.out_shape(rw, rh, b)
        for straddle, lay in fr.layouts.items():
            ents = far.entries(n)

            def call(s):
                g = {st: far.guarded((n, oh, ow), types[st][0]) for st in ALL}
                out = dv.Binned(**{st: g[st].t for st in ALL})
                _, res = fn(s.buf, s.lead, s.stream_bytes, s.offs, W, H, n, b, x, y, rw, rh, out=out)
                codec.sync()
                for st in ALL:
                    g[st].check(f"{st} plane {bits}-bit {straddle}")
                return tuple(g[st].t for st in ALL) + (res,)

            got, near = far_and_near(lay, ents, call)
            what = f"{bits}-bit binned {W}x{H} bin {b} window {(x, y, rw, rh)} {straddle}"
            assert_same(got, near, what)
            refs = fr.refs(lay, ents)
            assert_rows(codec, got[3], refs, what)
            per = {}
            for k, st in enumerate(ALL):
                planes = got[k].cpu().numpy().view(types[st][1]).astype(np.int64)
                for f, (_, img) in enumerate(refs):
                    if img is None:
                        assert (planes[f] == types[st][2]).all(), f"{what}: rejected entry {f}'s {st} plane was written"
                        continue
                    if id(img) not in per:
                        per[id(img)] = br.binned_reduceat(img, x, y, rw, rh, b)
                    assert np.array_equal(planes[f], per[id(img)][st]), f"{what}: {st} of entry {f}"
            del got, near


def check_repeated(plane, want, k, what):
    """plane (n, oh, ow) on the device: frame f equals want[f % k]."""
    import torch
    n = plane.shape[0]
    whole = n // k * k
    assert bool((plane[:whole].view(n // k, k, *plane.shape[1:]) == want.unsqueeze(0)).all()), f"{what}: planes past 2^32 differ"
    for f in range(whole, n):
        assert torch.equal(plane[f], want[f % k]), f"{what}: plane {f}"


def test_sum_planes_past_4gib(dv, codec, oracle):   # noqa: F811
    """700 U16 sum planes of 2048 x 1536 (4.40 GB) from repeated offsets of three 4096 x 3072 frames."""
    import torch
    W, H, k, n, b = 4096, 3072, 3, 700, 2
    src = far.guarded((k, H, W), torch.uint8)
    codec.synth_frames("mixed", 0xFA2_0B12, 0, k, W, H, out=src.t)
    cap = k * dv.max_frame_bytes(W, H)
    stream = far.guarded((cap,), torch.uint8)
    offs, sizes = codec.encode_frames(src.t, W, H, k, stream.buf, stream.lead, cap)
    codec.sync()
    total = int((offs[-1] + sizes[-1]).item())
    reps = (n + k - 1) // k
    rep, rsz = offs.repeat(reps)[:n].contiguous(), sizes.repeat(reps)[:n]
    plan = dv.binned_plan(W, H, n, b)
    assert (plan["out_w"], plan["out_h"], plan["sum_bytes"]) == (2048, 1536, n * 6291456) and plan["sum_bytes"] > G32
    planes = far.guarded((n, H // b, W // b), torch.int16)
    _, res = codec.decode_binned(stream.buf, stream.lead, total, rep, W, H, n, b, out=dv.Binned(sum=planes.t))
    codec.sync()
    planes.check("sum planes")
    want = src.t.view(k, H // b, b, W // b, b).to(torch.int16).sum((2, 4), dtype=torch.int16)
    check_repeated(planes.t, want, k, "U16 sums")
    assert torch.equal(res[:, 3], rsz)


def test_sum_planes16_past_4gib(dv, codec, o16):   # noqa: F811
    """350 U32 sum planes of 2048 x 1536 (4.40 GB) from repeated offsets of three full-range 4096 x 3072 U16 frames."""
    import torch
    W, H, k, n, b = 4096, 3072, 3, 350, 2
    src = far.guarded((k, H, W), torch.int16)
    g = torch.Generator(device="cuda").manual_seed(350)
    src.t[:] = torch.randint(-32768, 32768, (k, H, W), dtype=torch.int16, device="cuda", generator=g)
    src.t[1] >>= 5   # (arithmetic: values on both sides of 2^15, smaller depths)
    cap = k * int(codec.L.dbde16_hip_max_frame_bytes(W, H))
    stream = far.guarded((cap,), torch.uint8)
    offs, sizes = codec.encode_frames16(src.t, W, H, k, stream.buf, stream.lead, cap)
    codec.sync()
    total = int((offs[-1] + sizes[-1]).item())
    reps = (n + k - 1) // k
    rep, rsz = offs.repeat(reps)[:n].contiguous(), sizes.repeat(reps)[:n]
    plan = dv.binned16_plan(W, H, n, b)
    assert plan["sum_bytes"] == n * 12582912 and plan["sum_bytes"] > G32
    planes = far.guarded((n, H // b, W // b), torch.int32)
    _, res = codec.decode_binned16(stream.buf, stream.lead, total, rep, W, H, n, b, out=dv.Binned(sum=planes.t))
    codec.sync()
    planes.check("U32 sum planes")
    u16 = src.t.to(torch.int32) & 0xFFFF
    want = u16.view(k, H // b, b, W // b, b).sum((2, 4), dtype=torch.int32)
    check_repeated(planes.t, want, k, "U32 sums")
    assert torch.equal(res[:, 3], rsz)
