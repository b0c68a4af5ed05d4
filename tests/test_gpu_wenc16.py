"""GPU: dbde16_hip_encode_window (U16 pixels in, DBDE16 frames out) against the oracle's frames of the windows (tests/wenc_ref.py is the model, tests/wenc_gpu.py
holds the cases shared with the DBDE twin): every edge-tile margin and narrow window at every output alignment, every
row alignment, crafted windows inside hostile surroundings, the ends of the readable extent, per-frame origins, both
record levels under static chunk order, tickets and three workgroups, the argument rules, the forwarding case, the
round trip and the Python wrapper."""
import numpy as np
import pytest

import wenc_gpu as wg
import wenc_ref as wr

pytestmark = pytest.mark.gpu
BITS = 16


@pytest.fixture(scope="module")
def dv():
    import dbde_video_cpp_amd as dv
    dv.build()
    return dv


@pytest.fixture(scope="module")
def codec(dv):
    c = dv.Codec(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def pack(oracle):
    return wr.packer(oracle, BITS)


def test_margins_narrow_windows_layouts_and_output_alignment(codec, pack):
    wg.margins(codec, pack, BITS)


def test_every_row_alignment(codec, pack):
    wg.alignment(codec, pack, BITS)


@pytest.mark.parametrize("rw,rh", [(33, 31), (72, 72)])
def test_crafted_windows_do_not_see_their_surroundings(codec, pack, rw, rh):
    wg.surroundings(codec, pack, BITS, rw, rh)


def test_edges_of_the_buffer(codec, pack):
    wg.buffer_edges(codec, pack, BITS)


def test_per_frame_origins_are_clamped(codec, pack):
    wg.origins(codec, pack, BITS)


@pytest.fixture(scope="module", params=["chunks", "frames"])
def level_case(request, codec, pack, dv):
    return wg.record_levels(codec, pack, dv, BITS, request.param)


@pytest.mark.parametrize("flags", [0, 1, 1024, 1025])
def test_record_levels_static_tickets_and_three_workgroups(dv, codec, level_case, flags):
    c = codec if flags == 0 else wg.experiment_codec(dv, flags)
    try:
        wg.check_record_levels(c, level_case, BITS)
    finally:
        if flags:
            c.close()


@pytest.mark.parametrize("case", wg.ERROR_CASES)
def test_argument_rules(codec, pack, case):
    wg.errors(codec, pack, BITS, case)


def test_no_frames_does_nothing(codec):
    src = wr.Source(np.zeros(64, np.uint8), 0, 40, 29, 0, BITS)
    r = wr.run(codec, src, 5, 3, 17, 9)
    assert r.rc == 0
    wr.untouched(r, spans=[])


def test_whole_compact_frames_forward_to_encode_frames16(codec, dv):
    import torch
    W, H, n = 200, 123, 5
    assert dv.window_encode16_plan(W, H, n)["forwards"] == 1
    rng = np.random.default_rng(4)
    imgs = torch.from_numpy(wg.noise(rng, n, H, W, BITS).view(np.int16)).cuda()
    cap = n * int(codec.L.dbde16_hip_max_frame_bytes(W, H))
    a = torch.full((32 + cap + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    b = a.clone()
    oa, sa = codec.encode_frames16(imgs, W, H, n, a, 32, cap, first_index=3)
    ob, sb = codec.encode_window16(imgs, b, 32, cap, first_index=3)
    codec.sync()
    assert torch.equal(oa, ob) and torch.equal(sa, sb) and torch.equal(a, b)


@pytest.mark.parametrize("W,H,rw,rh,n", [(90, 50, 33, 31, 4), (1500, 1460, 1456, 1448, 2)])
def test_round_trip(codec, dv, W, H, rw, rh, n):
    import torch
    rng = np.random.default_rng(W)
    frames = torch.from_numpy(wg.noise(rng, n, H, W, BITS).view(np.int16)).cuda()
    x, y = W - rw - 3, 5
    maxf = int(codec.L.dbde16_hip_max_frame_bytes(rw, rh))
    buf = torch.full((32 + n * maxf + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    offs, sizes = codec.encode_window16(frames, buf, 32, n * maxf, x=x, y=y, rw=rw, rh=rh)
    back, res = codec.decode_frames16(buf, 32, n * maxf, offs, rw, rh, n)
    codec.sync()
    assert torch.equal(back, frames[:, y:y + rh, x:x + rw])


def test_python_takes_views_as_they_are(codec, dv, pack):
    import torch
    rng = np.random.default_rng(2)
    host = rng.integers(0, 65536, (4, 40, 61)).astype(np.uint16)
    frames = torch.from_numpy(host.view(np.int16)).cuda()
    view = frames[:, 3:34, 5:38]
    maxf = int(codec.L.dbde16_hip_max_frame_bytes(33, 31))
    buf = torch.full((32 + 4 * maxf + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    offs, sizes = codec.encode_window16(view, buf, 32, 4 * maxf, first_index=2)
    one_o, one_s = codec.encode_window16(frames[1], buf, 32 + 2 * maxf, 2 * maxf, x=5, y=3, rw=33, rh=31, first_index=8)
    codec.sync()
    got, o, s = buf.cpu().numpy(), offs.cpu().numpy(), sizes.cpu().numpy()
    assert got[32: 32 + o[0] + s[0]].tobytes() == pack(2, host[0, 3:34, 5:38]).tobytes()
    at = 32 + 2 * maxf
    assert got[at: at + int(one_s[0])].tobytes() == pack(8, host[1, 3:34, 5:38]).tobytes()
    with pytest.raises(dv.DbdeError, match="innermost stride"):
        codec.encode_window16(frames.transpose(1, 2), buf, 32, 4 * maxf)
    with pytest.raises(dv.DbdeError, match="int16"):
        codec.encode_window16(frames.to(torch.uint8), buf, 32, 4 * maxf)
