"""GPU: count projections on tests/crafted.py's streams (wrapping minima, every depth pattern), both pixel sizes, with
rejected frames between accepted ones: the planes and d_count exclude the rejected frames, the result rows are the
oracle's, and with maximum thresholds every pixel equals the accepted count."""
import numpy as np
import pytest

import counts_gpu as cg
import crafted as cr
import wproject_gpu as wg
from test_oracle_u16 import o16, unpack16   # noqa: F401  (fixture + helper)

pytestmark = pytest.mark.gpu

WINDOWS = [(0, 0, 72, 40), (3, 5, 41, 27), (37, 38, 1, 1)]


@pytest.fixture(scope="module")
def codec():
    import dbde_video_cpp_amd as m
    c = m.Codec(0)
    yield c
    c.close()


def crafted_stream(rng, W, H, n, bits, bad):
    """wproject_gpu.crafted_stream, keeping the frames' bytes for the oracle."""
    import torch
    T = cr.tiles(W, H)
    frames, images = [], []
    for f in range(n):
        fr = cr.craft(rng, W, H, bits, cr.DEPTHS[f % len(cr.DEPTHS)], cr.MINIMA[f % len(cr.MINIMA)],
                      cr.PAYLOADS[f % len(cr.PAYLOADS)])
        if f in bad:
            fr = cr.break_rule(fr, cr.BREAKS[f % len(cr.BREAKS)], bits, tile=int(rng.integers(0, T)))
        img = cr.decode_frame(fr, W, H, bits)[2]
        assert (img is None) == (f in bad), (f, "a crafted frame's verdict")
        frames.append(fr)
        images.append(img)
    buf, lead, offs, total = cr.layout(frames, "concat", lead=32)
    return wg.Stream(torch.from_numpy(buf).cuda(), lead, total, torch.from_numpy(offs).cuda(), W, H, images), frames


def oracle_rows(oracle, o16, frames, W, H, bits):   # noqa: F811
    rows = []
    for fr in frames:
        _, fh = oracle.unpack_frame_header(fr)
        used = oracle.unpack_frame(fr, W, H)[0] - 20 if bits == 8 else unpack16(o16, fr, W, H)[0]
        rows.append((fh[0] if used else 0xFFFFFFFF, fh[1], fh[2], 20 + used))
    return rows


@pytest.mark.parametrize("bits,bad", [(8, (1, 5, 6, 11)), (16, (0, 5, 6, 12)), (8, (0, 1, 2, 3, 8, 12))])
def test_rejected_frames_count_nothing(codec, oracle, o16, bits, bad):   # noqa: F811
    W, H, n = 72, 40, 13
    s, frames = crafted_stream(np.random.default_rng(5 + bits + len(bad)), W, H, n, bits, bad)
    call = codec.project_counts if bits == 8 else codec.project_counts16
    N = n - len(bad)
    want_rows = oracle_rows(oracle, o16, frames, W, H, bits)
    assert sum(r[3] == 20 for r in want_rows) == len(bad)
    rng = np.random.default_rng(6)
    top = (1 << bits) - 1
    for win in WINDOWS:
        for K in (1, 7, 8):
            for maps in (False, True):
                thr = cg.draw(rng, s.images, win, K, bits, maps)
                out, res = cg.check(call, s, thr, win, what=f"crafted {bits}-bit")
                assert int(out.count.item()) == N
                assert codec.parse_results(res) == want_rows
        for shape in ((2,), (2, win[3], win[2])):
            out, _ = cg.check(call, s, np.full(shape, top, cg.np_dtype(bits)), win, what="maximum thresholds")
            assert (cg.planes(out) == N).all()


@pytest.mark.parametrize("bits", (8, 16))
def test_every_frame_rejected(codec, bits):
    """accumulate=False: zero planes and count 0; accumulate=True: the planes and the count stay as they were."""
    import torch
    import dbde_video_cpp_amd as dv
    W, H, n = 72, 40, 7
    s, _ = crafted_stream(np.random.default_rng(8), W, H, n, bits, bad=range(n))
    call = codec.project_counts if bits == 8 else codec.project_counts16
    top = (1 << bits) - 1
    for win in WINDOWS[:2]:
        thr = np.full((3, win[3], win[2]), top, cg.np_dtype(bits))
        out, _ = cg.check(call, s, thr, win, what="all rejected")
        assert (out.out == 0).all() and int(out.count.item()) == 0
        prior = torch.randint(-2 ** 31, 2 ** 31 - 1, (3, win[3], win[2]), dtype=torch.int32, device="cuda")
        out = dv.CountProjection(prior.clone(), torch.full((1,), 5, dtype=torch.int64, device="cuda"))
        call(s.buf, s.lead, s.total, s.offs, W, H, n, cg.device(thr), *win, out=out, accumulate=True)
        codec.sync()
        assert torch.equal(out.out, prior) and int(out.count.item()) == 5
