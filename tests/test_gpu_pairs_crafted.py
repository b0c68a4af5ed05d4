"""GPU: pair projections on tests/crafted.py's streams (wrapping minima, every depth pattern, payloads that end with the
stream), both pixel sizes, at every edge-tile margin, with rejected frames between accepted ones: the planes and d_count
exclude the rejected frames and the result rows are the oracle's."""
import numpy as np
import pytest

import pairs_gpu as pg
import pairs_ref as pref
from test_gpu_counts_crafted import crafted_stream, oracle_rows
from test_oracle_u16 import o16   # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

# frame widths and heights of every margin 1..8 of the last tile column / row (65..72 x 33..40), two at a time
MARGINS = [(65 + m, 33 + (m * 3 + 1) % 8) for m in range(8)]


@pytest.fixture(scope="module")
def codec():
    import dbde_video_cpp_amd as m
    c = m.Codec(0)
    yield c
    c.close()


def windows(W, H):
    return [(0, 0, W, H), (3, 5, W - 9, H - 7), (W - 3, H - 3, 3, 3), (W - 1, H - 1, 1, 1)]


@pytest.mark.parametrize("bits,bad", [(8, (1, 5, 6, 11)), (16, (0, 5, 6, 12)), (8, (0, 1, 2, 3, 8, 12))])
def test_rejected_frames_add_nothing(codec, oracle, o16, bits, bad):   # noqa: F811
    W, H, n = 72, 40, 13
    s, frames = crafted_stream(np.random.default_rng(5 + bits + len(bad)), W, H, n, bits, bad)
    call = codec.project_pairs if bits == 8 else codec.project_pairs16
    want_rows = oracle_rows(oracle, o16, frames, W, H, bits)
    assert sum(r[3] == 20 for r in want_rows) == len(bad)
    for win in windows(W, H):
        for mask in pg.MASKS:
            out, res = pg.check(call, s, mask, win, what=f"crafted {bits}-bit", cap=False)
            assert int(out.count.item()) == n - len(bad)
            assert codec.parse_results(res) == want_rows
    pg.distinct(pref.pairs(s.images, 15, 0, 0, W, H)[0], pg.sumsq(s.images, (0, 0, W, H)))


@pytest.mark.parametrize("bits", (8, 16))
@pytest.mark.parametrize("W,H", MARGINS)
def test_every_edge_tile_margin(codec, bits, W, H):
    """Every depth pattern, minimum family and payload family of tests/crafted.py (13 frames walk them), the last
    frame's payload ending with the stream (the tail loads), one rejected frame."""
    n = 13
    s, _ = crafted_stream(np.random.default_rng(W * 41 + H + bits), W, H, n, bits, bad=(7,))
    call = codec.project_pairs if bits == 8 else codec.project_pairs16
    for win in windows(W, H):
        for mask in (15, 3, 1):
            out, _ = pg.check(call, s, mask, win, what=f"margins {bits}-bit", cap=False)
            assert int(out.count.item()) == n - 1


@pytest.mark.parametrize("bits", (8, 16))
def test_every_frame_rejected(codec, bits):
    """accumulate=False: zero planes and count 0; accumulate=True: the planes and the count stay as they were."""
    import torch
    import dbde_video_cpp_amd as dv
    W, H, n = 72, 40, 7
    s, _ = crafted_stream(np.random.default_rng(8), W, H, n, bits, bad=range(n))
    call = codec.project_pairs if bits == 8 else codec.project_pairs16
    for win in windows(W, H)[:2]:
        out, _ = pg.check(call, s, 15, win, what="all rejected", cap=False)
        assert (out.out == 0).all() and int(out.count.item()) == 0
        prior = torch.randint(-2 ** 62, 2 ** 62, (4, win[3], win[2]), dtype=torch.int64, device="cuda")
        out = dv.PairProjection(prior.clone(), torch.full((1,), 5, dtype=torch.int64, device="cuda"), dv.PAIR_OFFSETS)
        call(s.buf, s.lead, s.total, s.offs, W, H, n, 8, *win, out=out, accumulate=True)
        codec.sync()
        assert torch.equal(out.out, prior) and int(out.count.item()) == 5
