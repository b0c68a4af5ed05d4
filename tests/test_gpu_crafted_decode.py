"""GPU: the 8-bit decoders on crafted streams (tests/crafted.py) -- frames no encoder writes.

Minima that wrap (min + value > 255, depth-8 tiles with minima of 128 and more), every (depth, minimum) pair, payloads
of all ones, arbitrary headers (u64s other than 2, elapsed NaN, infinite, negative, 2^64 and above), and frames that
break exactly one rule at its edge, mixed into the streams.  Every case asserts the kernel form that
dbde_hip_decode_plan picks for it, so that a change of the default planner shows up here as a failure rather than as
lost coverage.  The experiment contexts ($DBDE_HIP_EXPERIMENT 16 and 1024) decode the same streams; decode_plan
describes the default context only, so for them the assertion names the geometry's default form, not the launch
their flags change.
Expected values come from the oracle (tests/test_crafted_streams.py ties it to the reference on such frames).
The geometries here are a handful; tests/test_decode_forms.py holds DECODE_CASES, the table with a row for every
decoder form at every edge-tile margin, and tests/test_gpu_decode_forms.py runs it with this file's streams and checks.
"""
import os

import numpy as np
import pytest

import crafted as cr

pytestmark = pytest.mark.gpu

PAD = 256          # canvas bytes of 0xEE in front of and behind the images
FILL = 0xEE

MID = dict(kernel=3)
CHUNK = dict(kernel=0)
DIRECT, STAGED, TILES = 0, 1, 2
TABLE, SELF, FUSED = 0, 1, 2

# (W, H, n, the form decode_plan picks on 256 CUs, how frames are placed, contexts besides the default)
CASES = [
    (8, 8, 500, dict(MID, threads=256), "residues", ("three",)),
    (72, 72, 200, dict(MID, threads=256), "concat", ("three",)),
    (150, 150, 20, dict(MID, threads=512), "residues", ("three",)),
    (180, 180, 20, dict(MID, threads=1024), "offsets", ("three",)),
    (200, 123, 13, dict(CHUNK, image_mode=STAGED, index_mode=SELF), "residues", ()),
    (384, 384, 1, dict(CHUNK, image_mode=DIRECT, index_mode=SELF), "concat", ()),
    (384, 384, 64, dict(CHUNK, image_mode=DIRECT, index_mode=SELF), "residues", ()),
    (1024, 768, 6, dict(CHUNK, image_mode=DIRECT, index_mode=FUSED), "offsets", ("fused",)),
    (1024, 768, 200, dict(CHUNK, image_mode=DIRECT, index_mode=TABLE), "concat", ()),
    (720, 1280, 32, dict(CHUNK, image_mode=STAGED, index_mode=FUSED), "residues", ("fused",)),
    (1080, 1920, 16, dict(CHUNK, image_mode=STAGED, index_mode=TABLE), "residues", ()),
    (1366, 768, 32, dict(CHUNK, image_mode=STAGED, index_mode=TABLE, threads=192), "offsets", ()),
    (2200, 1000, 16, dict(CHUNK, image_mode=TILES), "residues", ()),
    (4096, 3072, 1, dict(CHUNK, image_mode=DIRECT, index_mode=FUSED), "concat", ("fused",)),
]
BASES_1080P = (1, 8, 64)      # 1920 x 1080 x 64: staged through LDS in 480-tile chunks at these image bases
FORM_1080P = dict(CHUNK, image_mode=STAGED, index_mode=TABLE, chunk_tiles=480)


@pytest.fixture(scope="module")
def dv():
    import dbde_video_cpp_amd as m
    return m


def _codec(dv, flags=None):
    if flags is not None:
        os.environ["DBDE_HIP_EXPERIMENT"] = str(flags)
    try:
        c = dv.Codec(0)
    finally:
        os.environ.pop("DBDE_HIP_EXPERIMENT", None)
    assert c.arch.startswith("gfx950")
    return c


@pytest.fixture(scope="module")
def codecs(dv):
    """The default context, the fused decoder's fallback forced (bit 4: odd chunks publish nothing) and the mid-size
    decoder on three workgroups (bit 10)."""
    cs = {"default": _codec(dv), "fused": _codec(dv, 16), "three": _codec(dv, 1024)}
    yield cs
    for c in cs.values():
        c.close()


@pytest.fixture(scope="module")
def codec(codecs):
    return codecs["default"]


def valid_pool(rng, W, H, limit):
    """Up to `limit` distinct valid-structure frames, most telling first: every (depth, minimum) pair (cycled, in a
    random order unless the frame has exactly 2304 tiles), then the depth / minima / payload patterns."""
    T = cr.tiles(W, H)
    perm = None if T == 2304 else rng.permutation(2304)
    specs = [lambda p=p: cr.all_pairs_frame(rng, p, perm, T) for p in ("random", "ones", "zeros")]
    specs[1:1] = [lambda: cr.craft(rng, W, H, 8, "runs512", "boundary", "random")]
    specs += [lambda d=d, m=m, p=p: cr.craft(rng, W, H, 8, d, m, p)
              for d, m, p in (("max", "boundary", "ones"), ("odd", "boundary", "random"), ("runs256", "max", "ones"),
                              ("zero", "max", "zeros"), ("random", "boundary", "random"), ("max", "random", "zeros"))]
    return [s() for s in specs[:max(1, limit)]]


def bad_pool(rng, W, H, chunk_tiles, good):
    """Each rule broken at its edge (the bad depth in the last tile of the first chunk), and a DBDE16 frame."""
    T = cr.tiles(W, H)
    last = min(T, chunk_tiles or T) - 1
    bad = [cr.break_rule(good[k % len(good)], how, 8, tile=last) for k, how in enumerate(cr.BREAKS)]
    return bad + [cr.craft(rng, W, H, 16, "random", "boundary", "random")]


POOL = 10 + len(cr.BREAKS) + 1     # the whole pool: valid_pool's ten bodies, a frame per broken rule, a DBDE16 frame


class Stream:
    """n crafted frames (a pool of distinct bodies, each frame with its own random header), placed in one device
    buffer, with the oracle's verdict, result row and image of every frame.  `select`: the entries of the whole pool
    (0 .. POOL-1: valid bodies, then bad_pool's frames) that the stream holds, in that order and cycled over the n
    frames, whatever n is -- how a batch smaller than the pool gets every body and every break, a few per stream.
    `used`: the pool entries the stream holds; `depths`: the depth bytes of every frame."""

    def __init__(self, oracle, rng, W, H, n, how="concat", bad=True, chunk_tiles=0, u64s=None, select=None,
                 device="cuda"):
        import torch
        if select is None:
            good = valid_pool(rng, W, H, n)
            pool = good + (bad_pool(rng, W, H, chunk_tiles, good) if bad and n > 1 else [])
            order = rng.permutation(np.resize(np.arange(len(pool)), n))
            order[0] = 0                      # the first frame decodes, so does the last
            order[-1] = 0
            if n >= 12 and len(good) > 4:     # the all-depth-8 frame at 8 consecutive places: payloads at every residue
                order[1:9] = 4
            self.used = {int(k) if k < len(good) else int(k) - len(good) + POOL - len(cr.BREAKS) - 1 for k in order}
        else:
            good = valid_pool(rng, W, H, POOL)
            whole = good + bad_pool(rng, W, H, chunk_tiles, good)
            assert len(whole) == POOL
            pool = [whole[k] for k in select]
            order = np.arange(n) % len(pool)
            self.used = {int(select[k]) for k in order}
        want = [oracle.unpack_frame(p, W, H) for p in pool]
        self.frames, self.rows, self.images = [], [], []
        for k in order:
            fr = pool[k].copy()
            fr[:20] = cr.frame_header(*cr.random_header(rng, u64s))
            _, fh = oracle.unpack_frame_header(fr)
            adv = want[k][0]
            self.frames.append(fr)
            self.rows.append((fh[0] if adv > 20 else 0xFFFFFFFF, fh[1], fh[2], adv))
            self.images.append(want[k][2] if adv > 20 else None)
        buf, self.lead, offs, self.total = cr.layout(self.frames, how, lead=32)
        self.buf = torch.from_numpy(buf).to(device)
        self.offs = torch.from_numpy(offs).to(device)
        self.offs_h = offs
        self.W, self.H, self.n = W, H, n

    @property
    def depths(self):
        T = cr.tiles(self.W, self.H)
        return [fr[24:24 + T] for fr in self.frames]


def images_of(c, s, base):
    """The (n, H, W) images of canvas `c` (host bytes), after the check that the guards in front of and behind them
    still hold the fill."""
    size = s.n * s.H * s.W
    assert len(c) == PAD + base + size + PAD
    assert (c[:PAD + base] == FILL).all(), "wrote in front of the images"
    assert (c[PAD + base + size:] == FILL).all(), "wrote behind the images"
    return c[PAD + base: PAD + base + size].reshape(s.n, s.H, s.W)


def decode_into(codec, s, base):
    """decode_frames into a 0xEE canvas at image base residue `base`; -> (images (n, H, W), rows, image address)."""
    import torch
    size = s.n * s.H * s.W
    canvas = torch.full((PAD + base + size + PAD,), FILL, dtype=torch.uint8, device="cuda")
    images = canvas[PAD + base: PAD + base + size].view(s.n, s.H, s.W)
    _, res = codec.decode_frames(s.buf, s.lead, s.total, s.offs, s.W, s.H, s.n, images=images)
    codec.sync()
    return images_of(canvas.cpu().numpy(), s, base), codec.parse_results(res), images.data_ptr()


def check_decode(got, rows, s, what):
    for f in range(s.n):
        assert rows[f] == s.rows[f], f"{what}: frame {f} result {rows[f]} != oracle {s.rows[f]}"
        if s.images[f] is None:
            assert (got[f] == FILL).all(), f"{what}: rejected frame {f} wrote its image"
        elif not np.array_equal(got[f], s.images[f]):
            bad = np.argwhere(got[f] != s.images[f])
            raise AssertionError(f"{what}: frame {f}: {len(bad)} pixels differ from the oracle, first at "
                                 f"{tuple(bad[0])}: {got[f][tuple(bad[0])]} != {s.images[f][tuple(bad[0])]}")


def assert_form(dv, W, H, n, address, form):
    plan = dv.decode_plan(W, H, n, address)
    assert {k: plan[k] for k in form} == form, f"{W}x{H} x{n}: decode_plan {plan} is not {form}"


@pytest.mark.parametrize("W,H,n,form,how,extra", CASES, ids=[f"{c[0]}x{c[1]}x{c[2]}" for c in CASES])
def test_crafted_frames_decode_like_the_oracle(dv, codecs, oracle, W, H, n, form, how, extra):
    rng = np.random.default_rng(W * 65537 + H * 257 + n)
    plan = dv.decode_plan(W, H, n)
    s = Stream(oracle, rng, W, H, n, how, chunk_tiles=plan["chunk_tiles"])
    for name in ("default",) + extra:
        got, rows, addr = decode_into(codecs[name], s, 0)
        assert_form(dv, W, H, n, addr, form)
        check_decode(got, rows, s, f"{W}x{H} x{n} {name}")


def test_full_hd_at_image_bases(dv, codec, oracle):
    """1920 x 1080 x 64 at image bases 1, 8 and 64: tile rows staged through LDS, 480-tile chunks."""
    W, H, n = 1920, 1080, 64
    rng = np.random.default_rng(1080)
    s = Stream(oracle, rng, W, H, n, "residues", chunk_tiles=480)
    for base in BASES_1080P:
        got, rows, addr = decode_into(codec, s, base)
        assert_form(dv, W, H, n, addr, FORM_1080P)
        check_decode(got, rows, s, f"1920x1080 base {base}")


ROI_CASES = [(8, 8, 40), (72, 72, 30), (200, 123, 13), (1024, 768, 6)]


@pytest.mark.parametrize("W,H,n", ROI_CASES)
def test_windows_of_crafted_frames(codec, oracle, W, H, n):
    """decode_roi equals a crop of the oracle's image; rejected frames leave their window untouched."""
    import torch
    rng = np.random.default_rng(W * 31 + n)
    s = Stream(oracle, rng, W, H, n, "residues", chunk_tiles=512)
    windows = [(0, 0, W, H), (W // 3, H // 5, max(1, W // 2), max(1, H // 3)), (W - 1, H - 1, 1, 1),
               (1, 0, W - 1, min(H, 9))]
    for (x, y, rw, rh) in windows:
        for per_frame in (False, True):
            org = None
            if per_frame:
                org = np.stack([rng.integers(-3, W + 3, n), rng.integers(-3, H + 3, n)], 1).astype(np.int32)
            canvas = torch.full((n * rw * rh + 2 * PAD,), FILL, dtype=torch.uint8, device="cuda")
            out = canvas[PAD: PAD + n * rw * rh].view(n, rh, rw)
            _, res = codec.decode_roi(s.buf, s.lead, s.total, s.offs, W, H, n, x, y, rw, rh,
                                      origins=None if org is None else torch.from_numpy(org).cuda(), out=out)
            codec.sync()
            c = canvas.cpu().numpy()
            assert (c[:PAD] == FILL).all() and (c[PAD + n * rw * rh:] == FILL).all(), "wrote outside the windows"
            got = c[PAD: PAD + n * rw * rh].reshape(n, rh, rw)
            rows = codec.parse_results(res)
            for f in range(n):
                ox, oy = (x, y) if org is None else (min(max(int(org[f, 0]), 0), W - rw),
                                                     min(max(int(org[f, 1]), 0), H - rh))
                assert rows[f] == s.rows[f], (W, H, f, x, y, rw, rh, per_frame)
                if s.images[f] is None:
                    assert (got[f] == FILL).all(), f"rejected frame {f} wrote its window"
                else:
                    assert np.array_equal(got[f], s.images[f][oy:oy + rh, ox:ox + rw]), (W, H, f, ox, oy, rw, rh)


@pytest.mark.parametrize("W,H", [(8, 8), (61, 37), (384, 384)])
def test_host_pointer_calls_on_crafted_frames(codec, oracle, W, H):
    """unpack_frame, unpack_image and unpack_image_roi on crafted frames, good and bad, against the oracle."""
    rng = np.random.default_rng(W + 7 * H)
    s = Stream(oracle, rng, W, H, 18, "concat")
    for f, fr in enumerate(s.frames):
        adv, fh, img = codec.unpack_frame(fr, W, H)
        o_adv, o_fh, o_img = oracle.unpack_frame(fr, W, H)
        assert (adv, fh) == (o_adv, o_fh), (W, H, f)
        assert np.array_equal(img, o_img), (W, H, f)
        n, img = codec.unpack_image(fr[20:], W, H)
        o_n, o_img = oracle.unpack_image(fr[20:], W, H)
        assert n == o_n and np.array_equal(img, o_img), (W, H, f)
        x, y = int(rng.integers(0, W)), int(rng.integers(0, H))
        rw, rh = int(rng.integers(1, W - x + 1)), int(rng.integers(1, H - y + 1))
        n, win = codec.unpack_image_roi(fr[20:], W, H, x, y, rw, rh)
        assert n == o_n, (W, H, f)
        if n:
            assert np.array_equal(win, o_img[y:y + rh, x:x + rw]), (W, H, f, x, y, rw, rh)
        else:
            assert (win == FILL).all()


def test_tile_calls_at_odd_strides(codec, oracle):
    """unpack_8x8 / unpack_8x8_partial: every depth, the boundary minima, all three payload patterns, odd strides."""
    rng = np.random.default_rng(88)
    mins = cr.boundary_minima(8)
    for d in range(9):
        for p in cr.PAYLOADS:
            packed = cr.payload_bytes(rng, p, 8 * d)
            for mv in rng.choice(mins, 4, replace=False):
                stride = int(rng.choice([9, 11, 13, 17, 23, 37]))
                off = int(rng.integers(0, 8))
                size = 8 * stride + 16
                got = codec.unpack_8x8(d, int(mv), packed, stride, np.full(size, FILL, np.uint8), off)
                want = oracle.unpack_8x8(d, int(mv), packed, stride, np.full(size, FILL, np.uint8), off)
                assert np.array_equal(got, want), (d, p, mv, stride, off)
                rm, dm = int(rng.integers(1, 9)), int(rng.integers(1, 9))
                got = codec.unpack_8x8_partial(d, int(mv), packed, stride, rm, dm, np.full(size, FILL, np.uint8), off)
                want = oracle.unpack_8x8_partial(d, int(mv), packed, stride, rm, dm, np.full(size, FILL, np.uint8),
                                                 off)
                assert np.array_equal(got, want), (d, p, mv, stride, off, rm, dm)


@pytest.mark.parametrize("W,H,n", [(72, 72, 40), (200, 123, 13), (1024, 768, 9)])
def test_index_stream_finds_crafted_frames(codec, oracle, W, H, n):
    """The frame-to-frame walk over back-to-back crafted frames finds the offsets the depths give."""
    rng = np.random.default_rng(W * 3 + n)
    s = Stream(oracle, rng, W, H, n, "concat", bad=False, u64s=2)
    want = np.concatenate([[0], np.cumsum([20 + 12 + 2 * cr.tiles(W, H) + 8 * int(fr[24:24 + cr.tiles(W, H)].sum(
        dtype=np.int64)) for fr in s.frames])[:-1]])
    assert np.array_equal(want, s.offs_h)
    offs, count = codec.index_stream(s.buf, s.lead, s.total, W, H, n + 4)
    assert count == n and np.array_equal(offs.cpu().numpy(), want)


def test_file_of_crafted_frames(dv, codec, oracle, tmp_path):
    """A .dbde file of crafted frames (any index and elapsed) read back through the batched reader."""
    W, H, n = 133, 45, 23
    rng = np.random.default_rng(133)
    s = Stream(oracle, rng, W, H, n, "concat", bad=False, u64s=2)
    path = str(tmp_path / "crafted.dbde")
    with open(path, "wb") as fh:
        fh.write(dv.pack_video_header(3, H, W, 30.0).tobytes())
        for fr in s.frames:
            fh.write(fr.tobytes())
    got_imgs, got_heads = [], []
    with codec.open_reader(path, batch_frames=5) as r:
        for imgs, heads in r:
            got_imgs.extend(imgs.cpu().numpy())
            got_heads.extend(heads)
    assert len(got_heads) == n
    for f in range(n):
        assert got_heads[f] == s.rows[f][:3], f
        assert np.array_equal(got_imgs[f], s.images[f]), f
