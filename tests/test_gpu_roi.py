"""GPU: window (region-of-interest) decode -- dbde_hip_decode_roi and dbde_hip_unpack_image_roi.

Every window is compared byte for byte with the oracle's decode of the whole frame, cropped in numpy; rejections are
compared with what dbde_hip_decode_frames reports for the same batch.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MODES = ("noise8", "mixed", "flat", "smooth")
SEED = 0x5EED2016
GUARD = 48


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


class Batch:
    """n synthetic frames encoded on the device, and the oracle's full decode of each packed frame."""

    def __init__(self, codec, oracle, mode, W, H, n, first=0, slot_stride=0, misalign=0):
        imgs = codec.synth_frames(mode, SEED, first, n, W, H)
        buf, lead, cap = codec.alloc_stream(W, H, n, slot_stride=slot_stride, lead=48)
        lead += misalign
        buf.fill_(0xA5)
        offs, sizes = codec.encode_frames(imgs, W, H, n, buf, lead, cap, first_index=first, slot_stride=slot_stride)
        codec.sync()
        host = buf.cpu().numpy()
        o, s = offs.cpu().numpy(), sizes.cpu().numpy()
        self.packed = [host[lead + o[f]: lead + o[f] + s[f]].copy() for f in range(n)]
        self.full = []
        for f in range(n):
            used, fh, img = oracle.unpack_frame(self.packed[f], W, H)
            assert used == len(self.packed[f]) and fh[0] == 2
            self.full.append(img)
        self.buf, self.lead, self.offs, self.sizes = buf, lead, offs, s
        self.total = int(o[-1] + s[-1])
        self.W, self.H, self.n, self.first = W, H, n, first


def clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def run_roi(codec, b, x, y, rw, rh, origins=None, out_misalign=0, stream_bytes=None, offs=None, buf=None, lead=None):
    """Decodes the windows into a 0xEE canvas with guard bands; checks the guards; -> (windows (n, rh, rw), results)."""
    import torch
    n = b.n
    canvas = torch.full((n * rw * rh + 2 * GUARD + out_misalign,), 0xEE, dtype=torch.uint8, device="cuda")
    out = canvas[GUARD + out_misalign: GUARD + out_misalign + n * rw * rh].view(n, rh, rw)
    org = None
    if origins is not None:
        org = torch.tensor(np.asarray(origins, np.int32).reshape(n, 2), dtype=torch.int32, device="cuda")
    _, res = codec.decode_roi(b.buf if buf is None else buf, b.lead if lead is None else lead,
                              b.total if stream_bytes is None else stream_bytes, b.offs if offs is None else offs,
                              b.W, b.H, n, x, y, rw, rh, origins=org, out=out)
    codec.sync()
    c = canvas.cpu().numpy()
    assert (c[:GUARD + out_misalign] == 0xEE).all(), "wrote in front of the windows"
    assert (c[GUARD + out_misalign + n * rw * rh:] == 0xEE).all(), "wrote behind the windows"
    return c[GUARD + out_misalign: GUARD + out_misalign + n * rw * rh].reshape(n, rh, rw), codec.parse_results(res)


def check_windows(codec, b, x, y, rw, rh, origins=None, out_misalign=0):
    got, res = run_roi(codec, b, x, y, rw, rh, origins=origins, out_misalign=out_misalign)
    for f in range(b.n):
        ox, oy = (x, y) if origins is None else (clamp(origins[f][0], 0, b.W - rw), clamp(origins[f][1], 0, b.H - rh))
        want = b.full[f][oy:oy + rh, ox:ox + rw]
        if not np.array_equal(got[f], want):
            bad = np.argwhere(got[f] != want)
            raise AssertionError(f"{b.W}x{b.H} frame {f} window {rw}x{rh} at ({ox},{oy}): {len(bad)} bytes differ, "
                                 f"first at {tuple(bad[0])}")
    assert all(r == (2, b.first + f, 0, len(b.packed[f])) for f, r in enumerate(res))


def windows_for(W, H, rng):
    """The windows every geometry is checked with: (x, y, rw, rh)."""
    wins = [(0, 0, W, H), (W - 1, H - 1, 1, 1), (int(rng.integers(W)), int(rng.integers(H)), 1, 1)]
    if W >= 16 and H >= 16:
        wins.append((8, 8, 8 * max(1, (W - 8) // 16), 8 * max(1, (H - 8) // 16)))   # tile-aligned
    for r in range(8):                                                       # every residue of x and of rw
        rw = clamp(W // 3 + r, 1, W)
        x = clamp(r + 8 * int(rng.integers(max(1, (W - rw) // 8 + 1))), 0, W - rw)
        rh = clamp(H // 4 + (7 - r), 1, H)
        y = int(rng.integers(H - rh + 1))
        wins.append((x, y, rw, rh))
    wins.append((W - min(W, 37), H - min(H, 21), min(W, 37), min(H, 21)))  # touching the right and bottom edges
    wins.append((W - min(W, 3), 0, min(W, 3), H))                            # right edge, full height
    wins.append((0, H - min(H, 5), W, min(H, 5)))                            # bottom edge, full width
    wins.append((8 * ((W - 1) // 16), 0, min(8, W - 8 * ((W - 1) // 16)), H))  # one tile column
    wins.append((0, 8 * ((H - 1) // 16), W, min(8, H - 8 * ((H - 1) // 16))))  # one tile row
    if W > 4096:                                                             # across the 512-tile piece boundary
        wins += [(4090, 0, 20, H), (4095, 0, 2, min(H, 3)), (4000, 0, W - 4000, H)]
    return wins


GEOMETRIES = [(4096, 3072, 2), (1921, 1081, 2), (1920, 1080, 2), (720, 1283, 2), (2048, 2048, 2), (8200, 9, 3),
              (513, 17, 4), (72, 72, 5), (10, 10, 3), (1, 1, 3)]


@pytest.mark.parametrize("W,H,n", GEOMETRIES)
def test_windows_match_cropped_full_decode(codec, oracle, W, H, n):
    rng = np.random.default_rng(W * 7919 + H)
    for i, mode in enumerate(MODES):
        b = Batch(codec, oracle, mode, W, H, n, first=3 + i)
        wins = windows_for(W, H, rng)
        # every mode gets the full frame and a pixel; the other windows are dealt round-robin over the modes
        for k, (x, y, rw, rh) in enumerate(wins):
            if k < 2 or k % len(MODES) == i:
                check_windows(codec, b, x, y, rw, rh, out_misalign=k % 4)


@pytest.mark.parametrize("slot_stride_extra,misalign", [(0, 1), (0, 3), (13, 0), (13, 5)])
def test_concatenated_slotted_and_odd_base_streams(codec, oracle, dv, slot_stride_extra, misalign):
    W, H, n = 1921, 97, 4
    slot = dv.max_frame_bytes(W, H) + slot_stride_extra if slot_stride_extra else 0
    b = Batch(codec, oracle, "mixed", W, H, n, first=11, slot_stride=slot, misalign=misalign)
    for (x, y, rw, rh) in [(0, 0, W, H), (3, 5, 1000, 50), (1913, 89, 8, 8), (100, 0, 257, 97)]:
        check_windows(codec, b, x, y, rw, rh, out_misalign=misalign)


def test_per_frame_origins_are_clamped(codec, oracle):
    W, H, n, rw, rh = 1000, 500, 8, 120, 64
    b = Batch(codec, oracle, "mixed", W, H, n, first=1)
    origins = [(-5, H), (W, -3), (10 ** 6, 10 ** 6), (-(10 ** 6), 7), (3, 5), (W - rw, H - rh), (W - rw + 1, 0),
               (437, 211)]
    check_windows(codec, b, 0, 0, rw, rh, origins=origins)
    # (-5, H) decodes as (0, H - rh)
    got, _ = run_roi(codec, b, 0, 0, rw, rh, origins=origins)
    assert np.array_equal(got[0], b.full[0][H - rh:H, 0:rw])
    # every residue of the origin mod 8 in one batch, wide enough for two workgroups per tile row
    b = Batch(codec, oracle, "noise8", 4096, 40, n, first=2)
    origins = [(251 * k, (5 * k) % 24) for k in range(n)]   # x = 0, 251, ..., 1757: residues 0, 3, 6, 1, 4, 7, 2, 5
    check_windows(codec, b, 0, 0, 2100, 17, origins=origins)


def test_golden_packed_frames(codec, golden):
    """Frames the reference made (tests/golden): the host-pointer form against crops of the reference's images."""
    manifest, arrays = golden
    for e in manifest["frames"]:
        img, packed = arrays[e["name"] + ".image"], arrays[e["name"] + ".packed"]
        W, H = e["W"], e["H"]
        for (x, y, rw, rh) in {(0, 0, W, H), (W - 1, H - 1, 1, 1), (W // 3, H // 3, W - W // 3, H - H // 3),
                               (0, H // 2, max(1, W // 2), H - H // 2)}:
            n, win = codec.unpack_image_roi(packed[20:], W, H, x, y, rw, rh)
            assert n == len(packed) - 20, e["name"]
            assert np.array_equal(win, img[y:y + rh, x:x + rw]), (e["name"], x, y, rw, rh)


def test_rejections_match_decode_frames(codec, oracle):
    """One corrupted frame per rejection kind: the results equal decode_frames', and only that frame's window stays at
    the canvas."""
    import torch
    W, H, n = 200, 123, 8
    b = Batch(codec, oracle, "mixed", W, H, n, first=20)
    T = ((W + 7) // 8) * ((H + 7) // 8)
    o = b.offs.cpu().numpy()
    L = b.lead
    b.buf[L + int(o[1]) + 20] += 1                     # nb != T
    b.buf[L + int(o[2]) + 24 + T] += 1                 # nm != T
    b.buf[L + int(o[3]) + 28 + 2 * T] += 1             # n64 != sum(depth)
    b.buf[L + int(o[4]) + 24 + 5] = 9                  # a depth byte > 8
    offs = b.offs.clone()
    offs[5] = 2 ** 62                                   # a wild offset
    offs[6] = b.total + 1000                            # a frame outside stream_bytes
    bad = {1, 2, 3, 4, 5, 6}
    full_canvas = torch.full((n, H, W), 0xEE, dtype=torch.uint8, device="cuda")
    _, res_full = codec.decode_frames(b.buf, L, b.total, offs, W, H, n, images=full_canvas)
    codec.sync()
    want_res = codec.parse_results(res_full)
    for (x, y, rw, rh) in [(0, 0, W, H), (13, 7, 100, 50), (199, 122, 1, 1)]:
        got, res = run_roi(codec, b, x, y, rw, rh, offs=offs)
        assert res == want_res, (x, y, rw, rh)
        for f in range(n):
            if f in bad:
                assert res[f][0] == 0xFFFFFFFF and res[f][3] == 20 and (got[f] == 0xEE).all(), f
            else:
                assert np.array_equal(got[f], b.full[f][y:y + rh, x:x + rw]), f


@pytest.mark.parametrize("W,H,n,mode", [(64, 64, 3, "noise8"), (1921, 17, 2, "mixed"), (8200, 9, 2, "noise8"),
                                        (10, 10, 4, "smooth")])
def test_windows_read_nothing_past_stream_bytes(codec, oracle, W, H, n, mode):
    """stream_bytes is the readable extent: the stream ends at every residue mod 16 with junk behind it, the windows
    are identical; one byte short rejects the last frame only."""
    import torch
    b = Batch(codec, oracle, mode, W, H, n, first=3)
    rw, rh = max(1, W - 3), max(1, H - 2)
    x, y = W - rw, H - rh                              # the window reaches the last tile of the last frame
    for pad in range(16):
        for junk in (0xA5, 0x00, 0xFF):
            t = torch.full((pad + b.total + 48,), junk, dtype=torch.uint8, device="cuda")
            t[pad:pad + b.total] = b.buf[b.lead:b.lead + b.total]
            got, res = run_roi(codec, b, x, y, rw, rh, buf=t, lead=pad)
            for f in range(n):
                assert np.array_equal(got[f], b.full[f][y:y + rh, x:x + rw]), (pad, junk, f)
            assert all(r == (2, 3 + f, 0, len(b.packed[f])) for f, r in enumerate(res))
        got, res = run_roi(codec, b, x, y, rw, rh, buf=t, lead=pad, stream_bytes=b.total - 1)
        assert res[-1][0] == 0xFFFFFFFF and (got[-1] == 0xEE).all()
        for f in range(n - 1):
            assert res[f][0] == 2 and np.array_equal(got[f], b.full[f][y:y + rh, x:x + rw])


def test_timing_hook_zero_frames_and_argument_errors(codec, oracle, dv):
    import torch
    b = Batch(codec, oracle, "mixed", 300, 200, 2)
    codec.timing(True)
    codec.timing_read(reset=True)
    run_roi(codec, b, 10, 10, 100, 100)
    t = codec.timing_read(reset=True)
    codec.timing(False)
    assert t["decode_index"][1] == 1 and t["decode"][1] == 1 and t["encode"][1] == 0
    out = torch.full((4,), 0xEE, dtype=torch.uint8, device="cuda")
    rc = codec.L.dbde_hip_decode_roi(codec.h, b.buf.data_ptr() + b.lead, b.total, b.offs.data_ptr(), 300, 200, 0,
                                     0, 0, 2, 2, None, out.data_ptr(), None)
    codec.sync()
    assert rc == dv.OK and (out == 0xEE).all()
    scratch = torch.full((64,), 0xEE, dtype=torch.uint8, device="cuda")   # (rejected before anything is launched)
    for (x, y, rw, rh) in [(0, 0, 0, 5), (0, 0, 5, 0), (0, 0, 301, 5), (0, 0, 5, 201), (-1, 0, 5, 5), (296, 0, 5, 5),
                           (0, 196, 5, 5)]:
        with pytest.raises(dv.DbdeError, match="decode_roi"):
            codec.decode_roi(b.buf, b.lead, b.total, b.offs, 300, 200, 2, x, y, rw, rh, out=scratch)
    codec.sync()
    assert (scratch == 0xEE).all()
    # the host-pointer form: a rejected frame leaves the window untouched
    bad = b.packed[0][20:].copy()
    bad[4 + 3] = 9        # a depth byte > 8 (found on the device)
    n, win = codec.unpack_image_roi(bad, 300, 200, 5, 5, 50, 40)
    assert n == 0 and (win == 0xEE).all()


def test_seeded_fuzz(codec, oracle):
    """A few hundred random (geometry, window, origin) cases."""
    rng = np.random.default_rng(0xF022)
    for case in range(400):
        W = int(rng.choice([int(rng.integers(1, 80)), int(rng.integers(80, 700)), int(rng.integers(2000, 4400))]))
        H = int(rng.integers(1, 90)) if W > 2000 else int(rng.integers(1, 260))
        n = int(rng.integers(1, 4))
        mode = MODES[int(rng.integers(4))]
        b = Batch(codec, oracle, mode, W, H, n, first=case)
        rw, rh = int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))
        x, y = int(rng.integers(0, W - rw + 1)), int(rng.integers(0, H - rh + 1))
        origins = None
        if rng.integers(3) == 0:
            origins = [(int(rng.integers(-10, W + 10)), int(rng.integers(-10, H + 10))) for _ in range(n)]
        try:
            check_windows(codec, b, x, y, rw, rh, origins=origins, out_misalign=int(rng.integers(16)))
        except AssertionError as e:
            raise AssertionError(f"case {case}: {W}x{H} n={n} {mode} window {rw}x{rh} at ({x},{y}) "
                                 f"origins={origins}: {e}") from None
