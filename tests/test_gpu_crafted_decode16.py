"""GPU: the DBDE16 decoders (dbde16_hip_decode_frames, dbde16_hip_decode_roi) on crafted streams (tests/crafted.py).

U16 minima that wrap (min + value > 65535) at the boundary set of every depth 0..16, payloads of all ones, arbitrary
headers, and frames that break exactly one rule at its edge.  Runs of 256 tiles (the decoder's chunk) that are all
depth 16, with frames at every byte offset mod 16, take both the swizzled all-depth-16 path (payload at a multiple of
8 bytes) and the general path.  Expected values: the DBDE16 oracle (the extension's specification) and the oracle's
header read.  MARGIN_CASES give the decoder every right and bottom margin of a cut tile.
"""
import numpy as np
import pytest

import crafted as cr
from test_oracle_u16 import o16, unpack16   # noqa: F401  (fixture + helper)

pytestmark = pytest.mark.gpu

PAD = 128          # canvas pixels of 0xEEEE in front of and behind the images
FILL = 0xEEEE

# (W, H, n, how frames are placed): "offsets" puts frame k at byte k mod 16
CASES = [(8, 8, 40, "offsets"), (61, 37, 20, "residues"), (200, 123, 32, "offsets"), (1024, 768, 16, "offsets"),
         (2048, 1024, 3, "concat")]
# The one decode form (runs of 256 tiles, one index workgroup per frame) at every right margin rm = W mod 8 and bottom
# margin dm = H mod 8 in 1..7: frames of one chunk (2 x 2 tiles), and of two, 33 tiles across, so that tile rows
# straddle the chunk boundary (33 does not divide 256).  A batch of 6 holds valid bodies only (Stream16 cuts its pool
# to the batch), so the two-chunk frames come once more as batches of 20 with the rejected frames mixed in.
MARGIN_CASES = [(8 + m, 16 - m, 20, ("offsets", "residues", "concat")[m % 3]) for m in range(1, 8)] \
    + [(256 + m, 72 - m, 6, ("offsets", "residues", "concat")[m % 3]) for m in range(1, 8)] \
    + [(256 + m, 64 + m, 20, ("residues", "concat", "offsets")[m % 3]) for m in range(1, 8)]


@pytest.fixture(scope="module")
def codec():
    import dbde_video_cpp_amd as dv
    c = dv.Codec(0)
    assert c.arch.startswith("gfx950")
    yield c
    c.close()


class Stream16:
    """n crafted DBDE16 frames with random headers, placed in one device buffer; the oracle's row and image of each."""

    def __init__(self, o16, oracle, rng, W, H, n, how, device="cuda"):
        import torch
        T = cr.tiles(W, H)
        good = [cr.all_pairs_frame(rng, p, "random", T, bits=16) for p in ("ones", "random")]
        good += [cr.craft(rng, W, H, 16, d, m, p) for d, m, p in (
            ("max", "boundary", "random"), ("runs256", "boundary", "ones"), ("odd", "max", "ones"),
            ("max", "max", "zeros"), ("random", "random", "random"), ("zero", "boundary", "zeros"))]
        good = good[:n]
        pool = list(good)
        if n > 1:
            pool += [cr.break_rule(good[k % len(good)], how_, 16, tile=min(T, 256) - 1)
                     for k, how_ in enumerate(cr.BREAKS)]
            pool.append(cr.craft(rng, W, H, 8))                  # an 8-bit frame: nm = T, not 2T
        order = rng.permutation(np.resize(np.arange(len(pool)), n))
        order[0] = order[-1] = 0
        m = 16 if n >= 24 else 8     # an all-depth-16 frame at m consecutive places: its payload at every residue mod 8
        if n > m + 1:
            order[1:m + 1] = 2
        want = [unpack16(o16, p, W, H) for p in pool]
        self.frames, self.rows, self.images = [], [], []
        for k in order:
            fr = pool[k].copy()
            fr[:20] = cr.frame_header(*cr.random_header(rng))
            _, fh = oracle.unpack_frame_header(fr)
            used, img = want[k]
            self.frames.append(fr)
            self.rows.append((fh[0] if used else 0xFFFFFFFF, fh[1], fh[2], 20 + used))
            self.images.append(img if used else None)
        buf, self.lead, offs, self.total = cr.layout(self.frames, how, lead=32)
        self.buf = torch.from_numpy(buf).to(device)
        self.offs = torch.from_numpy(offs).to(device)
        self.W, self.H, self.n = W, H, n


def check(got, rows, s, what):
    for f in range(s.n):
        assert rows[f] == s.rows[f], f"{what}: frame {f} result {rows[f]} != oracle {s.rows[f]}"
        if s.images[f] is None:
            assert (got[f] == FILL).all(), f"{what}: rejected frame {f} wrote its image"
        elif not np.array_equal(got[f], s.images[f]):
            bad = np.argwhere(got[f] != s.images[f])
            raise AssertionError(f"{what}: frame {f}: {len(bad)} pixels differ from the oracle, first at "
                                 f"{tuple(bad[0])}: {got[f][tuple(bad[0])]} != {s.images[f][tuple(bad[0])]}")


@pytest.mark.parametrize("W,H,n,how", CASES + MARGIN_CASES,
                         ids=[f"{c[0]}x{c[1]}x{c[2]}" for c in CASES + MARGIN_CASES])
def test_crafted_frames_decode_like_the_oracle(codec, o16, oracle, W, H, n, how):   # noqa: F811
    import torch
    rng = np.random.default_rng(W * 4099 + H * 17 + n)
    s = Stream16(o16, oracle, rng, W, H, n, how)
    size = n * H * W
    canvas = torch.full((PAD + size + PAD,), FILL - 65536, dtype=torch.int16, device="cuda")
    images = canvas[PAD: PAD + size].view(n, H, W)
    _, res = codec.decode_frames16(s.buf, s.lead, s.total, s.offs, W, H, n, images=images)
    codec.sync()
    c = canvas.cpu().numpy().view(np.uint16)
    assert (c[:PAD] == FILL).all() and (c[PAD + size:] == FILL).all(), "wrote outside the images"
    check(c[PAD: PAD + size].reshape(n, H, W), codec.parse_results(res), s, f"{W}x{H} x{n}")


@pytest.mark.parametrize("W,H,n,how", CASES[:4], ids=[f"{c[0]}x{c[1]}x{c[2]}" for c in CASES[:4]])
def test_windows_of_crafted_frames(codec, o16, oracle, W, H, n, how):   # noqa: F811
    import torch
    rng = np.random.default_rng(W * 97 + n)
    s = Stream16(o16, oracle, rng, W, H, n, how)
    windows = [(0, 0, W, H), (W // 4, H // 3, max(1, W // 2), max(1, H // 2)), (W - 1, H - 1, 1, 1)]
    for (x, y, rw, rh) in windows:
        for per_frame in (False, True):
            org = None
            if per_frame:
                org = np.stack([rng.integers(-3, W + 3, n), rng.integers(-3, H + 3, n)], 1).astype(np.int32)
            size = n * rw * rh
            canvas = torch.full((PAD + size + PAD,), FILL - 65536, dtype=torch.int16, device="cuda")
            out = canvas[PAD: PAD + size].view(n, rh, rw)
            _, res = codec.decode_roi16(s.buf, s.lead, s.total, s.offs, W, H, n, x, y, rw, rh,
                                        origins=None if org is None else torch.from_numpy(org).cuda(), out=out)
            codec.sync()
            c = canvas.cpu().numpy().view(np.uint16)
            assert (c[:PAD] == FILL).all() and (c[PAD + size:] == FILL).all(), "wrote outside the windows"
            got = c[PAD: PAD + size].reshape(n, rh, rw)
            rows = codec.parse_results(res)
            for f in range(n):
                ox, oy = (x, y) if org is None else (min(max(int(org[f, 0]), 0), W - rw),
                                                     min(max(int(org[f, 1]), 0), H - rh))
                assert rows[f] == s.rows[f], (W, H, f, x, y, rw, rh, per_frame)
                if s.images[f] is None:
                    assert (got[f] == FILL).all(), f"rejected frame {f} wrote its window"
                else:
                    assert np.array_equal(got[f], s.images[f][oy:oy + rh, ox:ox + rw]), (W, H, f, ox, oy, rw, rh)
