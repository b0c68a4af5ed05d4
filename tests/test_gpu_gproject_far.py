"""GPU: grouped projections at stream offsets past 2^31 and 2^32 bytes and with plane sets past 2^32 bytes.

The buffers follow tests/far.py's layout rules (a sentinel lead in front of every buffer a kernel is given, a tail
behind it, every offset below 2^33), so a narrowed offset lands inside the test's own allocation and the test fails
with wrong values rather than a fault.

1. project_groups and project_groups16 read the six far placements of far.SLOTS (two of them rejected frames), once
   for each field that crosses 2^32, in uniform and ragged groups; every plane lies in a far.guarded buffer.  Expected:
   tests/gproject_ref.py over the oracle's decode of every distinct frame; the same call on a near copy of the stream,
   element for element; results rows are the real frames'.
2. Plane sets past 2^32 bytes from repeated offsets of three 4096 x 3072 frames in groups of 2: 342 U8 max planes
   (4.30 GB) and 172 DBDE16 U16 max planes (4.33 GB), each compared with the reduction of its two source frames.
"""
import numpy as np
import pytest

import far
from gproject_ref import group_ranges, reduce_groups
from test_gpu_far_offsets import (assert_rows, assert_same, codec, device_memory, dv, far_and_near,   # noqa: F401
                                  frames_of)
from test_gpu_gproject import assert_groups
from test_oracle_u16 import o16   # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

G32 = far.G32
ALL = ("max", "min", "sum", "sumsq")


@pytest.mark.parametrize("bits,W,H,n", [(8, 200, 123, 13), (8, 1024, 768, 6), (16, 200, 123, 13), (16, 1024, 768, 6)])
def test_grouped_projection_far(dv, codec, oracle, o16, bits, W, H, n):   # noqa: F811
    import torch
    fr = frames_of(oracle, o16, W, H, bits)
    pix = bits // 8
    fn = codec.project_groups if bits == 8 else codec.project_groups16
    types = dict(max=torch.uint8 if pix == 1 else torch.int16, min=torch.uint8 if pix == 1 else torch.int16,
                 sum=torch.int32, sumsq=torch.int64)
    cases = [((0, 0, W, H), dict(group_frames=2)), ((8, 16, W - 11, H - 19), dict(group_starts=[0, 3, 1, n + 5, 2, 2])),
             ((2, 6, W - 5, H - 9), dict(group_frames=n))]
    for (x, y, rw, rh), form in cases:
        ranges = group_ranges(n, form.get("group_frames"), form.get("group_starts"))
        ng = len(ranges)
        for straddle, lay in fr.layouts.items():
            ents = far.entries(n)

            def call(s):
                g = {st: far.guarded((ng, rh, rw), types[st]) for st in ALL}
                cnt = torch.full((ng,), -1, dtype=torch.int32, device="cuda")
                out = dv.GroupProjection(**{st: g[st].t for st in ALL}, counts=cnt)
                _, res = fn(s.buf, s.lead, s.stream_bytes, s.offs, W, H, n, x, y, rw, rh, out=out, **form)
                codec.sync()
                for st in ALL:
                    g[st].check(f"{st} planes {bits}-bit {straddle}")
                return tuple(g[st].t for st in ALL) + (cnt, res)

            got, near = far_and_near(lay, ents, call)
            what = f"{bits}-bit groups {W}x{H} {form} window {(x, y, rw, rh)} {straddle}"
            assert_same(got, near, what)
            refs = fr.refs(lay, ents)
            assert_rows(codec, got[5], refs, what)
            want = reduce_groups([img for _, img in refs], ranges, x, y, rw, rh, pix=pix)
            assert 0 < want["counts"].sum() < sum(e - b for b, e in ranges)   # accepted and rejected entries
            assert_groups(dv.GroupProjection(*got[:4], counts=got[4]), want, what=what)
            del got, near


def check_pairs(planes, want, k, what):
    """planes (n_groups, H, W) on the device: group j equals want[(2j) % k, (2j + 1) % k]'s entry."""
    import torch
    for j in range(planes.shape[0]):
        a, b = (2 * j) % k, (2 * j + 1) % k
        assert torch.equal(planes[j], want[(a, b)]), f"{what}: group {j} (frames {a}, {b})"


def test_max_planes_past_4gib(dv, codec, oracle):   # noqa: F811
    """342 U8 max planes of 4096 x 3072 (4.30 GB): groups of 2 over repeated offsets of three frames."""
    import torch
    W, H, k, ng = 4096, 3072, 3, 342
    n = 2 * ng
    src = far.guarded((k, H, W), torch.uint8)
    codec.synth_frames("mixed", 0xFA2_0B14, 0, k, W, H, out=src.t)
    cap = k * dv.max_frame_bytes(W, H)
    stream = far.guarded((cap,), torch.uint8)
    offs, sizes = codec.encode_frames(src.t, W, H, k, stream.buf, stream.lead, cap)
    codec.sync()
    total = int((offs[-1] + sizes[-1]).item())
    reps = (n + k - 1) // k
    rep, rsz = offs.repeat(reps)[:n].contiguous(), sizes.repeat(reps)[:n]
    plan = dv.project_groups_plan(W, H, n, group_frames=2, stats=("max",))
    assert plan["max_bytes"] == ng * W * H and plan["max_bytes"] > G32
    planes = far.guarded((ng, H, W), torch.uint8)
    counts = torch.zeros(ng, dtype=torch.int32, device="cuda")
    _, res = codec.project_groups(stream.buf, stream.lead, total, rep, W, H, n, group_frames=2,
                                  out=dv.GroupProjection(max=planes.t, counts=counts))
    codec.sync()
    planes.check("max planes")
    want = {(a, b): torch.maximum(src.t[a], src.t[b]) for a in range(k) for b in range(k)}
    check_pairs(planes.t, want, k, "U8 maxima")
    assert (counts == 2).all() and torch.equal(res[:, 3], rsz)


def test_max_planes16_past_4gib(dv, codec, o16):   # noqa: F811
    """172 U16 max planes of 4096 x 3072 (4.33 GB): groups of 2 over repeated offsets of three full-range U16 frames."""
    import torch
    W, H, k, ng = 4096, 3072, 3, 172
    n = 2 * ng
    src = far.guarded((k, H, W), torch.int16)
    g = torch.Generator(device="cuda").manual_seed(172)
    src.t[:] = torch.randint(-32768, 32768, (k, H, W), dtype=torch.int16, device="cuda", generator=g)
    src.t[1] >>= 5   # (arithmetic: values on both sides of 2^15, smaller depths)
    cap = k * int(codec.L.dbde16_hip_max_frame_bytes(W, H))
    stream = far.guarded((cap,), torch.uint8)
    offs, sizes = codec.encode_frames16(src.t, W, H, k, stream.buf, stream.lead, cap)
    codec.sync()
    total = int((offs[-1] + sizes[-1]).item())
    reps = (n + k - 1) // k
    rep, rsz = offs.repeat(reps)[:n].contiguous(), sizes.repeat(reps)[:n]
    plan = dv.project_groups16_plan(W, H, n, group_frames=2, stats=("max",))
    assert plan["max_bytes"] == 2 * ng * W * H and plan["max_bytes"] > G32
    planes = far.guarded((ng, H, W), torch.int16)
    counts = torch.zeros(ng, dtype=torch.int32, device="cuda")
    _, res = codec.project_groups16(stream.buf, stream.lead, total, rep, W, H, n, group_frames=2,
                                    out=dv.GroupProjection(max=planes.t, counts=counts))
    codec.sync()
    planes.check("U16 max planes")
    u = src.t.to(torch.int32) & 0xFFFF
    want = {(a, b): torch.maximum(u[a], u[b]).to(torch.int16) for a in range(k) for b in range(k)}
    check_pairs(planes.t, want, k, "U16 maxima")
    assert (counts == 2).all() and torch.equal(res[:, 3], rsz)
