"""GPU: DBDE16 window (region-of-interest) decode -- dbde16_hip_decode_roi.

Every window is compared pixel for pixel with two crops of the whole frame: the DBDE16 oracle's decode
(dbde16_oracle_unpack_image, the extension's specification) and dbde16_hip_decode_frames.  Rejections are compared
with what dbde16_hip_decode_frames reports for the same batch.
"""
import numpy as np
import pytest

from test_gpu_roi import clamp, windows_for
from test_gpu_u16 import make_images
from test_oracle_u16 import o16, unpack16   # noqa: F401  (fixture + helper)

pytestmark = pytest.mark.gpu

KINDS = ("full", "mixed", "small", "depth0", "depth16")
GUARD = 40        # pixels of 0xEEEE on either side of the windows
FILL = -4370      # 0xEEEE as int16


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


def images16(rng, n, W, H, kind):
    """make_images' kinds, plus depth 0 everywhere (one value per tile) and depth 16 everywhere (0 and 65535 in every
    tile that has two pixels)."""
    if kind == "depth0":
        v = rng.integers(0, 65536, size=(n, (H + 7) // 8, (W + 7) // 8))
        return np.ascontiguousarray(np.repeat(np.repeat(v, 8, axis=1), 8, axis=2)[:, :H, :W].astype(np.uint16))
    if kind == "depth16":
        img = rng.integers(0, 65536, size=(n, H, W)).astype(np.uint16)
        img[:, 0::8, 0::8] = 0
        img[:, 7::8, 7::8] = 65535
        img[:, 0::8, 1::8] = 65535
        return np.ascontiguousarray(img)
    return make_images(rng, n, W, H, kind)


class Batch16:
    """n DBDE16 frames encoded on the device, re-placed at byte `shift` of a fresh buffer (stream bases at any residue
    mod 16), with the oracle's and dbde16_hip_decode_frames' full decodes of every frame."""

    def __init__(self, codec, o16, imgs_h, first=0, slot_stride=0, shift=0, junk=0xA5):
        import torch
        n, H, W = imgs_h.shape
        maxf = int(codec.L.dbde16_hip_max_frame_bytes(W, H))
        cap = (n - 1) * slot_stride + maxf if slot_stride else n * maxf
        enc = torch.full((32 + cap + 64,), junk, dtype=torch.uint8, device="cuda")
        imgs = torch.from_numpy(imgs_h.view(np.int16)).cuda()
        offs, sizes = codec.encode_frames16(imgs, W, H, n, enc, 32, cap, first_index=first, slot_stride=slot_stride)
        codec.sync()
        o, s = offs.cpu().numpy(), sizes.cpu().numpy()
        self.total = int(o[-1] + s[-1])
        lead = 64 + shift
        self.buf = torch.full((lead + self.total + 80,), junk, dtype=torch.uint8, device="cuda")
        self.buf[lead:lead + self.total] = enc[32:32 + self.total]
        self.lead, self.offs, self.sizes = lead, offs, s
        host = self.buf.cpu().numpy()
        self.packed = [host[lead + o[f]: lead + o[f] + s[f]].copy() for f in range(n)]
        self.full = []
        for f in range(n):
            used, img = unpack16(o16, self.packed[f], W, H)
            assert used == len(self.packed[f]) - 20 and (img == imgs_h[f]).all()
            self.full.append(img)
        back, res = codec.decode_frames16(self.buf, lead, self.total, offs, W, H, n)
        codec.sync()
        self.gpu_full = back.cpu().numpy().view(np.uint16)
        self.W, self.H, self.n, self.first = W, H, n, first


def make_batch(codec, o16, rng, kind, W, H, n, **kw):
    return Batch16(codec, o16, images16(rng, n, W, H, kind), **kw)


def run_roi16(codec, b, x, y, rw, rh, origins=None, out_misalign=0, stream_bytes=None, offs=None, buf=None):
    """Decodes into a 0xEEEE canvas with guard bands (out_misalign pixels: the output base at 2 * that mod 16 bytes);
    checks the guards; -> (windows uint16 (n, rh, rw), parsed results)."""
    import torch
    n = b.n
    canvas = torch.full((n * rw * rh + 2 * GUARD + out_misalign,), FILL, dtype=torch.int16, device="cuda")
    out = canvas[GUARD + out_misalign: GUARD + out_misalign + n * rw * rh].view(n, rh, rw)
    org = None
    if origins is not None:
        org = torch.tensor(np.asarray(origins, np.int32).reshape(n, 2), dtype=torch.int32, device="cuda")
    got, res = codec.decode_roi16(b.buf if buf is None else buf, b.lead, b.total if stream_bytes is None else stream_bytes,
                                  b.offs if offs is None else offs, b.W, b.H, n, x, y, rw, rh, origins=org, out=out)
    assert got.data_ptr() == out.data_ptr() and got.dtype == torch.int16
    codec.sync()
    c = canvas.cpu().numpy().view(np.uint16)
    assert (c[:GUARD + out_misalign] == 0xEEEE).all(), "wrote in front of the windows"
    assert (c[GUARD + out_misalign + n * rw * rh:] == 0xEEEE).all(), "wrote behind the windows"
    return c[GUARD + out_misalign: GUARD + out_misalign + n * rw * rh].reshape(n, rh, rw), codec.parse_results(res)


def check_windows(codec, b, x, y, rw, rh, origins=None, out_misalign=0):
    got, res = run_roi16(codec, b, x, y, rw, rh, origins=origins, out_misalign=out_misalign)
    for f in range(b.n):
        ox, oy = (x, y) if origins is None else (clamp(origins[f][0], 0, b.W - rw), clamp(origins[f][1], 0, b.H - rh))
        for name, full in (("oracle", b.full[f]), ("decode_frames16", b.gpu_full[f])):
            want = full[oy:oy + rh, ox:ox + rw]
            if not np.array_equal(got[f], want):
                bad = np.argwhere(got[f] != want)
                raise AssertionError(f"{b.W}x{b.H} frame {f} window {rw}x{rh} at ({ox},{oy}): {len(bad)} pixels differ "
                                     f"from the {name} crop, first at {tuple(bad[0])}")
    assert all(r == (2, b.first + f, 0, len(b.packed[f])) for f, r in enumerate(res))


GEOMETRIES = [(1, 1, 3), (8, 8, 2), (10, 10, 3), (33, 31, 3), (200, 123, 2), (7, 300, 2), (1024, 40, 2), (4104, 16, 2),
              (4096, 3072, 1)]


@pytest.mark.parametrize("W,H,n", GEOMETRIES)
def test_windows_match_both_full_decodes(codec, o16, W, H, n):
    rng = np.random.default_rng(W * 7919 + H * 31 + n)
    for i, kind in enumerate(KINDS):
        b = make_batch(codec, o16, rng, kind, W, H, n, first=5 + i)
        wins = [(x, y, rw, rh) for (x, y, rw, rh) in windows_for(W, H, rng) if x + rw <= W and y + rh <= H]
        if W > 4096:   # across the 512-tile index piece boundary (column 4096) and the last 128-tile window piece
            wins += [(4090, 0, W - 4090, H), (4095, 1, 2, min(H - 1, 3)), (4000, 0, W - 4000, H)]
        for k, (x, y, rw, rh) in enumerate(wins):
            if k < 2 or k % len(KINDS) == i:   # full frame and a corner pixel for every kind, the rest dealt round-robin
                check_windows(codec, b, x, y, rw, rh, out_misalign=k % 8)


@pytest.mark.parametrize("slot", [False, True])
@pytest.mark.parametrize("shift", [0, 1, 2, 3, 5, 7, 8, 9, 11, 13, 14, 15])
def test_stream_layouts_and_bases(codec, o16, slot, shift):
    """Concatenated and slotted streams whose base sits at every residue mod 16 (the minima and payload then start at
    every alignment); windows across tile and piece boundaries."""
    W, H, n = 1031, 45, 3
    rng = np.random.default_rng(100 + shift + 50 * slot)
    maxf = None
    if slot:
        from dbde_video_cpp_amd import lib
        maxf = int(lib().dbde16_hip_max_frame_bytes(W, H))
    b = make_batch(codec, o16, rng, "mixed", W, H, n, first=1, slot_stride=((maxf + 255) // 256 * 256 + 24) if slot else 0,
                   shift=shift)
    for (x, y, rw, rh) in [(0, 0, W, H), (3, 5, 1021, 33), (1020, 40, 11, 5), (517, 7, 1, 1), (8, 8, 512, 16)]:
        check_windows(codec, b, x, y, rw, rh, out_misalign=shift % 8)


def test_per_frame_origins_are_clamped(codec, o16):
    W, H, n = 300, 211, 6
    rng = np.random.default_rng(77)
    b = make_batch(codec, o16, rng, "mixed", W, H, n, first=2)
    for rw, rh in [(64, 48), (1, 1), (W, H), (200, 7), (9, 211)]:
        origins = [(-5, -9), (W, H), (W - rw, 0), (17, 100), (2 ** 31 - 1, -(2 ** 31)), (int(rng.integers(W)), 3)]
        check_windows(codec, b, 0, 0, rw, rh, origins=origins, out_misalign=3)


def test_rejections_match_decode_frames16(codec, o16):
    """Depth byte 17, nm == T (an 8-bit frame), an n64 mismatch and a truncated last frame: each frame reports what
    dbde16_hip_decode_frames reports and leaves its window untouched; the good frames decode."""
    import torch
    W, H, n = 61, 37, 5
    rng = np.random.default_rng(9)
    b = make_batch(codec, o16, rng, "mixed", W, H, n, first=40)
    T = ((W + 7) // 8) * ((H + 7) // 8)
    o = b.offs.cpu().numpy()
    host = b.buf.cpu().numpy()
    base = b.lead
    host[base + o[0] + 24 + 3] = 17                     # frame 0: depth byte 17
    host[base + o[1] + 24 + T: base + o[1] + 28 + T] = np.frombuffer(np.int32(T).tobytes(), np.uint8)   # frame 1: nm = T
    n64 = base + o[3] + 28 + 3 * T                      # frame 3: n64 + 1
    host[n64: n64 + 4] = np.frombuffer(np.int32(int(host[n64: n64 + 4].view("<i4")[0]) + 1).tobytes(), np.uint8)
    buf = torch.from_numpy(host).cuda()
    truncated = b.total - 1                             # frame 4 ends one byte past the readable extent
    for (x, y, rw, rh) in [(0, 0, W, H), (5, 3, 17, 30), (60, 36, 1, 1)]:
        got, res = run_roi16(codec, b, x, y, rw, rh, buf=buf, stream_bytes=truncated)
        _, want = codec.decode_frames16(buf, b.lead, truncated, b.offs, W, H, n)
        codec.sync()
        assert res == codec.parse_results(want)
        for f in range(n):
            if f == 2:
                assert res[f] == (2, 42, 0, len(b.packed[f]))
                assert np.array_equal(got[f], b.full[f][y:y + rh, x:x + rw])
            else:
                assert res[f][0] == 0xFFFFFFFF, (f, res[f])
                assert (got[f] == 0xEEEE).all(), f"rejected frame {f} wrote its window"


def test_stream_bytes_end_at_the_last_frame(codec, o16):
    """The readable extent ends exactly at the last frame's last byte, with junk behind it, at every residue of the
    end mod 16."""
    W, H, n = 203, 19, 2
    for shift in range(16):
        rng = np.random.default_rng(300 + shift)
        b = make_batch(codec, o16, rng, "full", W, H, n, first=0, shift=shift, junk=0x5A + shift)
        check_windows(codec, b, 0, 0, W, H)
        check_windows(codec, b, W - 9, H - 3, 9, 3, out_misalign=shift % 8)


def test_zero_frames_timing_hook_and_argument_errors(codec, o16, dv):
    import torch
    W, H = 64, 40
    rng = np.random.default_rng(4)
    b = make_batch(codec, o16, rng, "mixed", W, H, 2)
    codec.timing(True)
    codec.timing_read(reset=True)
    check_windows(codec, b, 3, 4, 30, 20)
    t = codec.timing_read(reset=True)
    assert t["decode_index"][1] == 1 and t["decode"][1] == 1 and t["encode"][1] == 0
    assert t["decode_index"][0] > 0 and t["decode"][0] > 0
    # n = 0: nothing launched, nothing written
    out = torch.full((4,), FILL, dtype=torch.int16, device="cuda")
    codec.decode_roi16(b.buf, b.lead, b.total, b.offs, W, H, 0, 0, 0, 1, 1, out=out)
    codec.sync()
    t = codec.timing_read(reset=True)
    codec.timing(False)
    assert t["decode_index"][1] == 0 and t["decode"][1] == 0
    assert (out.cpu().numpy().view(np.uint16) == 0xEEEE).all()
    L, h = codec.L, codec.h
    ptr = b.buf.data_ptr() + b.lead
    for args in [(0, 0, 65, 1), (0, 0, 1, 41), (64, 0, 1, 1), (0, -1, 1, 1), (0, 0, 0, 1)]:
        assert L.dbde16_hip_decode_roi(h, ptr, b.total, b.offs.data_ptr(), W, H, 2, *args, None, out.data_ptr(),
                                       None) == dv.ERR_ARG
    assert L.dbde16_hip_decode_roi(h, ptr, b.total, b.offs.data_ptr(), W, H, 2, 0, 0, 1, 1, None, None, None) == dv.ERR_ARG
    assert L.dbde16_hip_decode_roi(h, None, b.total, b.offs.data_ptr(), W, H, 2, 0, 0, 1, 1, None, out.data_ptr(),
                                   None) == dv.ERR_ARG
    assert L.dbde16_hip_decode_roi(h, ptr, b.total, b.offs.data_ptr(), 40000, 40000, 1, 0, 0, 8, 8, None, out.data_ptr(),
                                   None) == dv.ERR_ARG
    codec.sync()
    assert (out.cpu().numpy().view(np.uint16) == 0xEEEE).all()


def test_seeded_fuzz(codec, o16):
    """About 200 random cases: geometry, content, layout, stream base, window, per-frame origins, output alignment."""
    rng = np.random.default_rng(0xF022)
    for case in range(200):
        W = int(rng.choice([int(rng.integers(1, 40)), int(rng.integers(40, 700)), int(rng.integers(1020, 1100))]))
        H = int(rng.integers(1, 60))
        n = int(rng.integers(1, 4))
        kind = KINDS[int(rng.integers(len(KINDS)))]
        slot = 0
        if rng.integers(2):
            from dbde_video_cpp_amd import lib
            slot = (int(lib().dbde16_hip_max_frame_bytes(W, H)) + 7) // 8 * 8 + 8 * int(rng.integers(0, 5))
        b = make_batch(codec, o16, rng, kind, W, H, n, first=case, slot_stride=slot, shift=int(rng.integers(16)))
        rw, rh = int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))
        x, y = int(rng.integers(W - rw + 1)), int(rng.integers(H - rh + 1))
        origins = None
        if rng.integers(3) == 0:
            origins = [(int(rng.integers(-20, W + 20)), int(rng.integers(-20, H + 20))) for _ in range(n)]
            x = y = 0
        try:
            check_windows(codec, b, x, y, rw, rh, origins=origins, out_misalign=int(rng.integers(8)))
        except AssertionError as e:
            raise AssertionError(f"fuzz case {case}: {W}x{H} n={n} {kind} slot={slot} window {rw}x{rh} at ({x},{y}) "
                                 f"origins={origins}: {e}") from None
