"""GPU: patch moments of DBDE16 streams -- dbde16_hip_patch_moments (Codec.patch_moments16).

As tests/test_gpu_moments.py with U16 pixels: expected values are tests/moments_ref.py's over the images
dbde16_hip_decode_frames writes for the same frames (for crafted frames: crafted.decode_frame's), compared exactly.
Also the 64-bit witness (the largest sums a patch can have), and tracking.follow on a DBDE16 stream.
"""
import numpy as np
import pytest

import moments_ref as mr
import patch_ref as pr
from test_gpu_mask16 import Batch16
from test_gpu_moments import bands_for, check_moments, crafted_bands, run_moments
from test_gpu_patches import origins_for, sizes_for
from test_gpu_project16 import Crafted16

pytestmark = pytest.mark.gpu

TOP = 65535


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


@pytest.mark.parametrize("W,H,n", [(4096, 24, 2), (8200, 17, 2), (513, 17, 2), (1921, 25, 2), (72, 72, 2), (10, 10, 2),
                                   (1, 1, 2)])
def test_moments16_match_moments_ref(codec, W, H, n):
    import torch
    rng = np.random.default_rng(W * 31 + H + 1)
    batches = [Batch16(codec, kind, W, H, n) for kind in ("mixed", "full")]
    bands = [bands_for(rng, list(b.images), TOP) for b in batches]
    for j, (pw, ph) in enumerate(sizes_for(W, H) + [(3, 512)]):
        b, bd = batches[j % 2], bands[j % 2]
        frames = list(b.images)
        org = origins_for(rng, W, H, pw, ph, n)
        K = org.shape[1]
        counts = [None, [K] * n, [0] * n, [K + 5, 1, K // 2, 0][:n], None][j % 5]
        lo, hi = bd[(3 * j) % len(bd)]
        res = check_moments(codec, b, frames, W, H, pw, ph, org, lo, hi, j % 4, counts, pr.FILL, bits=16, what="fill")
        assert torch.equal(res, b.results)
        if pw <= W and ph <= H:
            lo, hi = bd[(3 * j + 1) % len(bd)]
            check_moments(codec, b, frames, W, H, pw, ph, org, lo, hi, (j + 1) % 4, counts, pr.CLAMP, bits=16, what="clamp")


@pytest.mark.parametrize("kind", ("mixed", "full"))
def test_threshold_sites_of_the_header_shortcut16(codec, kind):
    W, H, n = 72, 41, 2
    rng = np.random.default_rng(len(kind))
    b = Batch16(codec, kind, W, H, n)
    org = np.array([[(x, y) for x in (-3, 0, 21, 45) for y in (-2, 7, 15)]] * n)
    for i, (lo, hi) in enumerate(bands_for(rng, list(b.images), TOP, tiles=8)):
        check_moments(codec, b, list(b.images), W, H, 32, 30, org, lo, hi, i % 4, None, pr.FILL, bits=16, what=f"sites {kind}")


@pytest.mark.parametrize("W,H,n,how", [(64, 48, 7, "concat"), (200, 123, 5, "residues")])
def test_crafted16_and_rejected_frames(codec, W, H, n, how):
    """Every depth 0..16 at every payload byte alignment, wrapping minima, broken frames between good ones."""
    import torch
    rng = np.random.default_rng(W * 7919 + H)
    s = Crafted16(rng, W, H, n, how)
    assert any(im is None for im in s.images) and any(im is not None for im in s.images)
    _, want_res = codec.decode_frames16(s.buf, s.lead, s.total, s.offs, W, H, n)
    pw, ph = 32, min(H, 32)
    org = np.array([[(x, y) for x in (-5, 19, W - 9) for y in (-3, H - 6)]] * n)
    for i, (lo, hi) in enumerate(crafted_bands(s, W, H, 2, rng)):
        res = check_moments(codec, s, s.images, W, H, pw, ph, org, lo, hi, i % 4, None, pr.FILL if i % 3 else pr.CLAMP,
                            bits=16, what=f"crafted16 {how}")
        assert torch.equal(res, want_res)
    for j, (pw, ph) in enumerate(((9, 9), (58, min(H, 58)))):
        org = origins_for(rng, W, H, pw, ph, n)
        for m in (pr.CLAMP, pr.FILL):
            check_moments(codec, s, s.images, W, H, pw, ph, org, (0, 20000)[j], (TOP, 50000)[j], (j + m) % 4, None, m,
                          bits=16, what=f"crafted16 {how}")


def test_the_largest_sums_fit_64_bits(codec):
    """One 512 x 512 frame of all 65535, a 505 x 512 patch, weight VALUE: every sum equals its closed form (Syy, the
    largest, is 65535 * 505 * sum i^2, about 2^50.4; the bound 65535 * 511^2 * 505 * 512 < 2^63 of the header takes 511^2
    for every row).  The same patch at (-7, -7) in FILL mode: every tile offset is negative or odd."""
    import torch
    W = H = 512
    img = np.full((1, H, W), TOP, np.uint16)
    cap = int(codec.L.dbde16_hip_max_frame_bytes(W, H))
    buf = torch.full((64 + cap,), 0xA5, dtype=torch.uint8, device="cuda")
    offs, sizes = codec.encode_frames16(torch.from_numpy(img.view(np.int16)).cuda(), W, H, 1, buf, 48, cap)
    codec.sync()
    total = int((offs[-1] + sizes[-1]).item())
    pw, ph = 505, 512
    s1 = lambda k: sum(range(k))                    # noqa: E731
    s2 = lambda k: sum(i * i for i in range(k))     # noqa: E731
    mom, box, _, _ = run_moments(codec, buf, 48, total, offs, W, H, 1, pw, ph, [[(0, 0)]], 0, TOP, mr.VALUE, None, pr.CLAMP, 16)
    want = [pw * ph, TOP * pw * ph, TOP * ph * s1(pw), TOP * pw * s1(ph), TOP * ph * s2(pw), TOP * s1(pw) * s1(ph),
            TOP * pw * s2(ph), TOP * TOP * pw * ph]
    assert mom[0, 0].tolist() == want and want[6] > 2 ** 50 and box[0, 0].tolist() == [0, 0, pw - 1, ph - 1]
    assert want == mr.moments(img[0], W, H, pw, ph, 0, 0, pr.CLAMP, 0, TOP, mr.VALUE)[0]
    mom, box, _, _ = run_moments(codec, buf, 48, total, offs, W, H, 1, pw, ph, [[(-7, -7)]], 0, TOP, mr.VALUE, None, pr.FILL, 16)
    m, bx, _ = mr.moments(img[0], W, H, pw, ph, -7, -7, pr.FILL, 0, TOP, mr.VALUE)
    assert mom[0, 0].tolist() == m and tuple(box[0, 0]) == bx == (7, 7, pw - 1, ph - 1)
    ss = lambda a, k: sum(range(a, k))              # noqa: E731
    assert m[2] == TOP * (ph - 7) * ss(7, pw) and m[6] == TOP * (pw - 7) * (s2(ph) - s2(7))
    # ABOVE a level of 0 is VALUE
    mom2, _, _, _ = run_moments(codec, buf, 48, total, offs, W, H, 1, pw, ph, [[(-7, -7)]], 0, TOP, mr.ABOVE, None, pr.FILL, 16)
    assert np.array_equal(mom, mom2)


def test_stream_end_and_follow16(codec, dv):
    """The stream ends exactly at the last frame (one byte short rejects only the last frame), and tracking.follow with
    bits=16 equals the same recurrence in numpy."""
    import torch
    from dbde_video_cpp_amd import tracking
    W, H, n, pw, ph, lo, hi = 120, 67, 6, 20, 18, 3000, 60000
    rng = np.random.default_rng(16)
    imgs = rng.integers(100, 900, size=(n, H, W)).astype(np.uint16)
    yy, xx = np.mgrid[0:H, 0:W]
    start, step = np.array([(30.0, 20.0), (90.0, 40.0)]), np.array([(2.0, 1.0), (-1.0, 2.0)])
    for f in range(n):
        for (x0, y0), (dx, dy) in zip(start, step):
            blob = (xx - x0 - f * dx) ** 2 + (yy - y0 - f * dy) ** 2 <= 8.0
            imgs[f][blob] = 20000 + 37 * ((xx * 3 + yy)[blob] % 200)
    cap = n * int(codec.L.dbde16_hip_max_frame_bytes(W, H))
    buf = torch.full((51 + cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    offs, sizes = codec.encode_frames16(torch.from_numpy(imgs.view(np.int16)).cuda(), W, H, n, buf, 51, cap)
    codec.sync()
    total = int((offs[-1] + sizes[-1]).item())
    frames = list(imgs)
    org = np.array([[(W - pw, H - ph), (25, 12), (-4, -4)]] * n)

    class S:
        pass
    for pad in range(16):
        t = torch.full((pad + total + 48,), (0xA5, 0x00, 0xFF)[pad % 3], dtype=torch.uint8, device="cuda")
        t[pad:pad + total] = buf[51:51 + total]
        check_moments(codec, S, frames, W, H, pw, ph, org, lo, hi, pad % 4, None, pr.FILL, bits=16, stream=(t, pad, total, offs))
        res = check_moments(codec, S, frames[:-1] + [None], W, H, pw, ph, org, lo, hi, pad % 4, None, pr.FILL, bits=16,
                            stream=(t, pad, total - 1, offs))
        assert codec.parse_results(res)[-1][0] == 0xFFFFFFFF
    centres, pm = tracking.follow(codec, buf, 51, total, offs, W, H, n, start, pw, ph, lo, hi, weight="value", bits=16)
    codec.sync()
    c = start.copy()
    for f in range(n):
        o = dv.origins_from_centres(c[None], pw, ph)[0]
        for k in range(2):
            m = mr.moments(imgs[f], W, H, pw, ph, o[k, 0], o[k, 1], pr.FILL, lo, hi, mr.VALUE)[0]
            assert pm.moments.cpu().numpy()[f, k].tolist() == m
            if m[1]:
                c[k] = (np.float64(o[k, 0]) + np.float64(m[2]) / np.float64(m[1]), np.float64(o[k, 1]) + np.float64(m[3]) / np.float64(m[1]))
        assert np.array_equal(centres.cpu().numpy()[f], c)
    assert np.abs(c - (start + (n - 1) * step)).max() < 1.0
