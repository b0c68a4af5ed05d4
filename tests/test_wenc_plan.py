"""CPU: dbde_hip_window_encode_plan / dbde16_hip_window_encode_plan (pure host arithmetic) against a Python
restatement of include/dbde_hip.h, every argument rule broken once, the forwarding case, and a 4096 x 3072 window."""
import ctypes as C

import pytest

import wenc_ref as wr


@pytest.fixture(scope="module")
def dv():
    import dbde_video_cpp_amd as dv
    import os
    if not os.path.exists(dv.LIB_PATH):
        dv.build()
    return dv


THREADS, GROUP, PER_CU = 256, 64, 4


def restated(bits, W, H, n, x, y, rw, rh, pitch=0, frame_stride=0, slot_stride=0, has_origins=False, n_cu=256):
    px = bits // 8
    p, s = wr.compact(W, H, bits, pitch, frame_stride)
    w, h = (rw + 7) // 8, (rh + 7) // 8
    maxf = wr.max_frame_bytes(rw, rh, bits)
    out = dict(tiles_x=w, tiles_y=h, tiles=w * h, pitch=p, frame_stride=s,
               min_image_bytes=wr.min_image_bytes(W, H, n, bits, pitch, frame_stride), max_out_frame_bytes=maxf,
               out_capacity=((n - 1) * slot_stride + maxf if slot_stride else n * maxf) if n else 0)
    fwd = not has_origins and (rw, rh) == (W, H) and p == W * px and s == H * W * px
    lpr = (w + 1) // 2 if bits == 8 else w
    cpf = (h * lpr + THREADS - 1) // THREADS
    gpf = (cpf + GROUP - 1) // GROUP
    kernel = dict(forwards=0, lanes_per_row=lpr, chunks_per_frame=cpf, chunk_tiles=512 if bits == 8 else 256,
                  record_group=GROUP, threads=THREADS, grid=min(n * cpf, PER_CU * n_cu),
                  workspace_bytes=16 + 8 * (n * cpf + n * gpf + n + (n + GROUP - 1) // GROUP))
    off = dict(forwards=1, lanes_per_row=0, chunks_per_frame=0, chunk_tiles=0, record_group=0, threads=0, grid=0,
               workspace_bytes=0, lds_bytes=0)
    out.update(off if fwd else kernel)
    return out


GEOMETRIES = [(40, 29, 3, 5, 3, 17, 9, 43, 0), (40, 29, 3, 5, 3, 1, 9, 43, 2000), (100, 20, 2, 15, 2, 64, 16, 113, 0),
              (1500, 1460, 3, 31, 7, 1456, 1448, 0, 0), (47, 19, 130, 13, 5, 20, 12, 0, 0), (4096, 3072, 8, 0, 0, 4096, 3072, 4160, 0),
              (4096, 3072, 1024, 1003, 697, 2045, 2043, 0, 0), (200, 123, 5, 0, 0, 200, 123, 0, 0), (8, 8, 0, 0, 0, 8, 8, 0, 0)]


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("W,H,n,x,y,rw,rh,pitch,stride", GEOMETRIES)
def test_plan_equals_the_restatement(dv, bits, W, H, n, x, y, rw, rh, pitch, stride):
    px = bits // 8
    plan = dv.window_encode_plan if bits == 8 else dv.window_encode16_plan
    for slot in (0, wr.max_frame_bytes(rw, rh, bits) + 24):
        for org, n_cu in ((False, 256), (True, 3)):
            got = plan(W, H, n, x, y, rw, rh, pitch=pitch * px, frame_stride=stride * px, slot_stride=slot, has_origins=org, n_cu=n_cu)
            want = restated(bits, W, H, n, x, y, rw, rh, pitch * px, stride * px, slot, org, n_cu)
            assert {k: got[k] for k in want} == want


def test_record_level_geometries_and_the_full_frame(dv):
    """The sizes tests/test_gpu_wenc*.py rely on, from the plan: 1456 x 1448 has more chunks than one group of records
    holds; a 4096 x 3072 window is admitted, also at 1,024 frames a call."""
    a = dv.window_encode_plan(1500, 1460, 3, 31, 7, 1456, 1448)
    assert (a["tiles"], a["chunk_tiles"], a["chunks_per_frame"], a["record_group"]) == (32942, 512, 65, 64)
    b = dv.window_encode16_plan(1500, 1460, 3, 31, 7, 1456, 1448)
    assert (b["chunk_tiles"], b["chunks_per_frame"]) == (256, 129)
    for plan in (dv.window_encode_plan, dv.window_encode16_plan):
        c = plan(4096 + 64, 3072 + 8, 1024, 64, 8, 4096, 3072)
        assert c["forwards"] == 0 and c["tiles"] == 196608 and c["grid"] == 1024
        assert plan(4096, 3072, 1024, pitch=(4096 + 64) * (1 if plan is dv.window_encode_plan else 2))["forwards"] == 0


def test_forwarding_case(dv):
    for plan, px in ((dv.window_encode_plan, 1), (dv.window_encode16_plan, 2)):
        assert plan(200, 123, 5)["forwards"] == 1
        assert plan(200, 123, 5, pitch=200 * px, frame_stride=200 * 123 * px)["forwards"] == 1
        assert plan(200, 123, 5, has_origins=True)["forwards"] == 0
        assert plan(200, 123, 5, pitch=202 * px)["forwards"] == 0
        assert plan(200, 123, 5, frame_stride=200 * 123 * px + 2)["forwards"] == 0
        assert plan(200, 123, 5, 0, 0, 199, 123)["forwards"] == 0
        assert plan(200, 123, 5, 0, 0, 200, 122)["forwards"] == 0


def raw(dv, bits, W=40, H=29, n=3, x=5, y=3, rw=17, rh=9, pitch=None, stride=0, image_bytes=None, address=0, cap=0, slot=0):
    px = bits // 8
    pitch = 43 * px if pitch is None else pitch
    if image_bytes is None:
        image_bytes = wr.min_image_bytes(W, H, n, bits, pitch, stride)
    pl = dv.WindowEncodePlan()
    fn = dv.lib().dbde_hip_window_encode_plan if bits == 8 else dv.lib().dbde16_hip_window_encode_plan
    return fn(address, image_bytes, W, H, pitch, stride, n, x, y, rw, rh, 0, cap, slot, 256, C.byref(pl))


@pytest.mark.parametrize("bits", [8, 16])
def test_every_argument_rule(dv, bits):
    px = bits // 8
    W, H, n, rw, rh = 40, 29, 3, 17, 9
    maxf = wr.max_frame_bytes(rw, rh, bits)
    ARG, CAP = dv.ERR_ARG, dv.ERR_CAPACITY
    assert raw(dv, bits) == 0
    assert raw(dv, bits, pitch=W * px) == 0 and raw(dv, bits, pitch=W * px - px) == ARG          # pitch below W * PIX
    assert raw(dv, bits, pitch=43 * px + 1) == (0 if bits == 8 else ARG)                         # odd pitch: U16 only
    assert raw(dv, bits, stride=43 * px * H + 1) == (0 if bits == 8 else ARG)                    # odd stride: U16 only
    assert raw(dv, bits, address=4097) == (0 if bits == 8 else ARG)                              # odd base: U16 only
    least = (H - 1) * 43 * px + W * px
    assert raw(dv, bits, stride=least) == 0 and raw(dv, bits, stride=least - px) == ARG           # stride too small
    need = wr.min_image_bytes(W, H, n, bits, 43 * px)
    assert raw(dv, bits, image_bytes=need) == 0 and raw(dv, bits, image_bytes=need - 1) == ARG    # one byte short
    assert raw(dv, bits, x=W - rw) == 0 and raw(dv, bits, x=W - rw + 1) == ARG                    # origin outside
    assert raw(dv, bits, y=H - rh + 1) == ARG and raw(dv, bits, x=-1) == ARG and raw(dv, bits, y=-1) == ARG
    assert raw(dv, bits, x=0, rw=W) == 0 and raw(dv, bits, x=0, rw=W + 1) == ARG                  # rw > W
    assert raw(dv, bits, y=0, rh=H + 1) == ARG and raw(dv, bits, rw=0) == ARG and raw(dv, bits, rh=0) == ARG
    assert raw(dv, bits, n=-1) == ARG and raw(dv, bits, n=0) == 0
    assert raw(dv, bits, cap=n * maxf) == 0 and raw(dv, bits, cap=n * maxf - 1) == CAP            # capacity one byte short
    assert raw(dv, bits, slot=maxf, cap=2 * maxf + maxf) == 0
    assert raw(dv, bits, slot=maxf, cap=3 * maxf - 1) == CAP
    assert raw(dv, bits, slot=maxf - 1) == (ARG if bits == 8 else CAP)                            # slot_stride below the maximum: as each frame encoder reports it
    assert raw(dv, bits, W=0) == ARG and raw(dv, bits, H=0) == ARG
    with pytest.raises(ValueError):
        (dv.window_encode_plan if bits == 8 else dv.window_encode16_plan)(W, H, n, W - rw + 1, 0, rw, rh)


def test_too_many_chunks_in_one_call(dv):
    # 2^31 chunks: 2^26 frames of 32 chunks (512 x 2048 pixels: 64 x 256 tiles, 32 lanes a row, 8192 lanes a frame)
    assert raw(dv, 8, W=512, H=2048, n=(1 << 26) - 1, x=0, y=0, rw=512, rh=2048, pitch=513) == 0
    assert raw(dv, 8, W=512, H=2048, n=1 << 26, x=0, y=0, rw=512, rh=2048, pitch=513) == dv.ERR_ARG
