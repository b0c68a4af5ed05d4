"""GPU: dbde_hip_encode_window against the oracle's frames of the windows (tests/wenc_ref.py is the model, tests/wenc_gpu.py
holds the cases shared with the DBDE16 twin): every edge-tile margin and narrow window at every output alignment, every
row alignment, crafted windows inside hostile surroundings, the ends of the readable extent, per-frame origins, both
record levels under static chunk order, tickets and three workgroups, the argument rules, the forwarding case, the
round trip and the Python wrapper."""
import numpy as np
import pytest

import wenc_gpu as wg
import wenc_ref as wr

pytestmark = pytest.mark.gpu
BITS = 8


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


def test_indices_and_elapsed_ns(codec, pack):
    rng = np.random.default_rng(1)
    src = wg.source(rng, 40, 29, 3, BITS, pitch=43, base=1)
    wr.run_and_check(codec, pack, src, 5, 3, 21, 13, indices=[2 ** 63 + 5, 7, 2 ** 40], elapsed_ns=[0, 123456789, 2 ** 53 + 2])


def test_no_frames_does_nothing(codec):
    src = wr.Source(np.zeros(64, np.uint8), 0, 40, 29, 0, BITS)
    r = wr.run(codec, src, 5, 3, 17, 9)
    assert r.rc == 0
    wr.untouched(r, spans=[])


def test_whole_compact_frames_forward_to_encode_frames(codec, dv):
    """Whole frame, compact pitch and stride, no origins: byte for byte encode_frames' output (the plan says it forwards)."""
    import torch
    W, H, n = 200, 123, 5
    assert dv.window_encode_plan(W, H, n)["forwards"] == 1
    assert dv.window_encode_plan(W, H, n, pitch=W + 1)["forwards"] == 0
    imgs = codec.synth_frames("mixed", 5, 0, n, W, H)
    cap = n * dv.max_frame_bytes(W, H)
    a = torch.full((32 + cap + 64,), 0xEE, dtype=torch.uint8, device="cuda")
    b = a.clone()
    oa, sa = codec.encode_frames(imgs, W, H, n, a, 32, cap, first_index=3)
    ob, sb = codec.encode_window(imgs, b, 32, cap, first_index=3)
    codec.sync()
    assert torch.equal(oa, ob) and torch.equal(sa, sb) and torch.equal(a, b)


@pytest.mark.parametrize("W,H,rw,rh,n", [(90, 50, 33, 31, 4), (1500, 1460, 1456, 1448, 2)])
def test_round_trip(codec, dv, W, H, rw, rh, n):
    import torch
    frames = codec.synth_frames("mixed", 9, 0, n, W, H)
    x, y = W - rw - 3, 5
    buf, lead, cap = codec.alloc_stream(rw, rh, n)
    offs, sizes = codec.encode_window(frames, buf, lead, cap, x=x, y=y, rw=rw, rh=rh)
    back, res = codec.decode_frames(buf, lead, cap, offs, rw, rh, n)
    codec.sync()
    assert torch.equal(back, frames[:, y:y + rh, x:x + rw])
    assert [r[0] for r in codec.parse_results(res)] == [2] * n


def test_python_takes_views_as_they_are(codec, dv, pack):
    import torch
    rng = np.random.default_rng(2)
    host = rng.integers(0, 256, (4, 40, 61)).astype(np.uint8)
    frames = torch.from_numpy(host).cuda()
    view = frames[:, 3:34, 5:38]
    buf, lead, cap = codec.alloc_stream(33, 31, 4)
    offs, sizes = codec.encode_window(view, buf, lead, cap, first_index=2)
    codec.sync()
    got, o, s = buf.cpu().numpy(), offs.cpu().numpy(), sizes.cpu().numpy()
    for f in range(4):
        want = pack(2 + f, host[f, 3:34, 5:38])
        assert got[lead + o[f]: lead + o[f] + s[f]].tobytes() == want.tobytes(), f
    # a window of a view, and a single (H, W) image
    offs, sizes = codec.encode_window(view, buf, lead, cap, x=4, y=2, rw=20, rh=12)
    one_o, one_s = codec.encode_window(frames[1, 3:34, 5:38], buf, lead + int(cap) // 2, cap // 2, first_index=8)
    codec.sync()
    got, o, s = buf.cpu().numpy(), offs.cpu().numpy(), sizes.cpu().numpy()
    assert got[lead + o[3]: lead + o[3] + s[3]].tobytes() == pack(3, host[3, 5:17, 9:29]).tobytes()
    at = lead + int(cap) // 2
    assert got[at: at + int(one_s[0])].tobytes() == pack(8, host[1, 3:34, 5:38]).tobytes()
    # what the C call would reject is rejected before it, by name
    for bad, word in ((frames.transpose(1, 2), "innermost stride"), (frames.expand(4, 40, 61)[:, :, :].as_strided((4, 40, 61), (2440, 0, 1)), "pitch"),
                      (frames.as_strided((4, 40, 61), (100, 61, 1)), "frame stride"), (frames.to(torch.int16), "uint8")):
        with pytest.raises(dv.DbdeError, match=word):
            codec.encode_window(bad, buf, lead, cap)
    with pytest.raises(dv.DbdeError, match="origin"):
        codec.encode_window(frames, buf, lead, cap, x=30, y=0, rw=40, rh=10)
    with pytest.raises(dv.DbdeError, match="capacity"):
        codec.encode_window(frames, buf, lead, 100)
