"""GPU: the window encoder with source frames and output slots at byte offsets past 2^31 and 2^32.

The buffers are far.guarded allocations (tests/far.py: a sentinel lead of 2^31 + 2^26 bytes -- 2^33 for U16 -- in front
of what the kernel is given, a tail behind it), so an offset narrowed to 32 bits lands inside the test's own memory
and shows as wrong bytes, not as a fault.  Source: 72 frames at frame_stride 2^26, so frame f and frame f - 64 alias
under a 32-bit offset, and they hold different `mixed` images.  Window 200 x 123.  Output: one slot per frame at
slot_stride 2^26, so slots pass 2^31 and 2^32.  Expected frames are the oracle's; offsets, sizes, and the sentinel in
front of, between and behind the frames are checked.
"""
import numpy as np
import pytest

import far
import wenc_gpu as wg
import wenc_ref as wr
from test_gpu_far_offsets import check_untouched, codec, device_memory, dv   # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
STRIDE = 1 << 26
N, W, H, X, Y, RW, RH = 72, 260, 150, 33, 17, 200, 123


@pytest.mark.parametrize("bits", [8, 16])
def test_far_source_frames_and_far_output_slots(dv, codec, oracle, bits):   # noqa: F811
    import torch
    px = bits // 8
    pitch = (W + 7) * px
    if bits == 8:
        host = np.stack([oracle.synth_frame(1, far.SYNTH_SEED, f, W, H) for f in range(N)])
    else:
        host = wg.noise(np.random.default_rng(16), N, H, W, 16)
    assert all(not np.array_equal(host[f], host[f - 64]) for f in range(64, N))
    nbytes = (N - 1) * STRIDE + (H - 1) * pitch + W * px
    assert nbytes > far.G32 and H * pitch < STRIDE
    dtype = torch.uint8 if bits == 8 else torch.int16
    src = far.guarded((nbytes // px,), dtype)
    view = torch.as_strided(src.t, (N, H, W), (STRIDE // px, pitch // px, 1))
    view.copy_(torch.from_numpy(host.view(np.uint8 if bits == 8 else np.int16)).cuda())
    maxf = wr.max_frame_bytes(RW, RH, bits)
    cap = (N - 1) * STRIDE + maxf
    out = far.guarded((cap,), torch.uint8)
    fn = codec.encode_window if bits == 8 else codec.encode_window16
    first = far.G32 - 3                     # indices cross 2^32
    offs, sizes = fn(view, out.buf, out.lead, cap, x=X, y=Y, rw=RW, rh=RH, first_index=first, slot_stride=STRIDE)
    codec.sync()
    o, s = offs.cpu().numpy(), sizes.cpu().numpy()
    assert [int(v) for v in o] == [f * STRIDE for f in range(N)]
    assert int(o[33]) > far.G31 and int(o[65]) > far.G32
    pack = wr.packer(oracle, bits)
    for f in range(N):
        want = pack(first + f, host[f, Y:Y + RH, X:X + RW])
        assert int(s[f]) == len(want), f
        got = out.t[int(o[f]): int(o[f]) + len(want)].cpu().numpy()
        assert got.tobytes() == want.tobytes(), f"frame {f} (source offset {f * STRIDE}, slot at {int(o[f])})"
    check_untouched(out.buf, out.lead, [(int(a), int(a) + int(c)) for a, c in zip(o, s)], f"{bits}-bit window encode")
    out.check(f"{bits}-bit window encode")
    # the source is only read: its lead and tail, and the bytes between the images, keep the sentinel
    src.check("source")
    assert far.all_equal(src.buf[src.lead + H * pitch: src.lead + STRIDE], far.SENTINEL)
