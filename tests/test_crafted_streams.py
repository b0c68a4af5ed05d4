"""CPU: crafted streams (tests/crafted.py) -- frames an encoder never writes, decoded by the oracles and the reference.

- The numpy decoder of crafted.py, written from the format alone, equals the 8-bit oracle and the DBDE16 oracle on
  crafted frames: wrapping minima, every depth pattern and payload pattern, and frames that break one rule.
- The oracle equals the real reference on crafted 8-bit frames and headers (needs oracle/_ref).
- The host header read (dbde_hip_unpack_frame_header) converts the F64 elapsed as the reference's x86-64 build does,
  pinned on the doubles where compilers differ.
"""
import ctypes as C

import numpy as np
import pytest

import crafted as cr
from test_oracle_u16 import o16, unpack16   # noqa: F401  (fixture + helper)

SHAPES = [(1, 1), (8, 8), (7, 13), (64, 24), (69, 41), (130, 17)]

# elapsed bits -> what the reference (g++ -O3 -march=corei7, x86-64) reads, recorded from oracle/_ref/libdbde_ref.so
PINNED_ELAPSED = {
    0x0000000000000000: 0x0000000000000000,
    0x8000000000000000: 0x0000000000000000,   # -0.0
    0x3FE0000000000000: 0x0000000000000000,   # 0.5
    0x3FF8000000000000: 0x0000000000000001,   # 1.5
    0xBFE0000000000000: 0x0000000000000000,   # -0.5
    0xBFF0000000000000: 0xFFFFFFFFFFFFFFFF,   # -1.0
    0x0000000000000001: 0x0000000000000000,   # smallest subnormal
    0x43DFFFFFFFFFFFFF: 0x7FFFFFFFFFFFFC00,   # 2^63 - 1024
    0x43E0000000000000: 0x8000000000000000,   # 2^63
    0x43E0000000000001: 0x8000000000000800,   # 2^63 + 2048
    0x43EFFFFFFFFFFFFF: 0xFFFFFFFFFFFFF800,   # 2^64 - 2048
    0x43F0000000000000: 0x0000000000000000,   # 2^64
    0x43F0000000000001: 0x0000000000000000,   # 2^64 + 4096
    0x7E37E43C8800759C: 0x0000000000000000,   # 1e300
    0x7FEFFFFFFFFFFFFF: 0x0000000000000000,   # largest finite
    0x7FF0000000000000: 0x0000000000000000,   # +inf
    0xFFF0000000000000: 0x8000000000000000,   # -inf
    0x7FF8000000000000: 0x8000000000000000,   # NaN
    0xFFF8000000000000: 0x8000000000000000,   # -NaN
    0x7FF0000000000001: 0x8000000000000000,   # signalling NaN
    0xC3E0000000000000: 0x8000000000000000,   # -2^63
    0xC3E0000000000001: 0x8000000000000000,   # below -2^63
    0xFE37E43C8800759C: 0x8000000000000000,   # -1e300
}


@pytest.fixture(scope="module")
def dv():
    import dbde_video_cpp_amd as m
    return m


def crafted_frames(rng, W, H, bits):
    """Every depth, minima and payload pattern once (the random ones drawn twice), plus each broken rule."""
    out = []
    for depth in cr.DEPTHS:
        for minima in cr.MINIMA:
            out.append(cr.craft(rng, W, H, bits, depth, minima, cr.PAYLOADS[len(out) % 3]))
    for payload in cr.PAYLOADS:
        out.append(cr.craft(rng, W, H, bits, "max", "max", payload))
    for how in cr.BREAKS:
        out.append(cr.break_rule(cr.craft(rng, W, H, bits), how, bits))
    return out


def test_model_of_the_x86_conversion():
    for bits, want in PINNED_ELAPSED.items():
        assert cr.f64_to_u64_x86(bits) == want, hex(bits)


@pytest.mark.parametrize("W,H", SHAPES)
def test_numpy_decoder_equals_the_oracle(oracle, W, H):
    rng = np.random.default_rng(W * 1009 + H)
    for k, fr in enumerate(crafted_frames(rng, W, H, 8)):
        adv, fh, img = cr.decode_frame(fr, W, H, 8)
        o_adv, o_fh, o_img = oracle.unpack_frame(fr, W, H)
        assert (adv, fh) == (o_adv, o_fh), (W, H, k)
        if img is None:
            assert (o_img == 0xEE).all(), (W, H, k)
        else:
            assert np.array_equal(img, o_img), (W, H, k)


@pytest.mark.parametrize("W,H", SHAPES)
def test_numpy_decoder_equals_the_dbde16_oracle(o16, W, H):   # noqa: F811
    rng = np.random.default_rng(W * 2003 + H)
    for k, fr in enumerate(crafted_frames(rng, W, H, 16)):
        adv, _, img = cr.decode_frame(fr, W, H, 16)
        n, o_img = unpack16(o16, fr, W, H)
        assert adv == 20 + n, (W, H, k)
        if img is None:
            assert (o_img == 0xEEEE).all()
        else:
            assert np.array_equal(img, o_img), (W, H, k)
    # every (depth, boundary minimum) pair decodes with the wrap
    bm = cr.boundary_minima(16)
    d = np.repeat(np.arange(17), len(bm)).astype(np.uint8)
    m = np.tile(bm, 17)
    fr = cr.frame(d, m, np.full(8 * int(d.astype(np.int64).sum()), 0xFF, np.uint8), bits=16)
    Wd = 8 * len(d)
    adv, _, img = cr.decode_frame(fr, Wd, 8, 16)
    n, o_img = unpack16(o16, fr, Wd, 8)
    assert adv == 20 + n and np.array_equal(img, o_img)
    top = (m + (1 << d.astype(np.int64)) - 1) & 0xFFFF      # all-ones payload: every pixel is min + 2^d - 1
    assert np.array_equal(img[0, ::8].astype(np.int64), top)


RULE_OF = {"depth": "depth", "nm+1": "nm", "nm-1": "nm", "n64+1": "n64", "n64-1": "n64", "T+1": "T", "T-1": "T"}


@pytest.mark.parametrize("bits", (8, 16))
def test_each_broken_frame_breaks_exactly_one_rule(bits):
    """So that each rejection the decoder tests expect can only come from the check they mean: a depth above the
    maximum keeps n64 == sum(depth), at any tile and from any depth it replaces."""
    rng = np.random.default_rng(bits)
    for W, H in SHAPES + [(200, 123), (1024, 40)]:
        T = cr.tiles(W, H)
        tiles_at = sorted({0, T - 1, min(T, 256) - 1, min(T, 512) - 1, min(T, 480) - 1})
        for depth in cr.DEPTHS:
            fr = cr.craft(rng, W, H, bits, depth, "boundary")
            assert cr.broken_rules(fr[20:], W, H, bits) == set()
            for how in cr.BREAKS:
                for t in (tiles_at if how == "depth" else [None]):
                    g = cr.break_rule(fr, how, bits, tile=t)
                    assert cr.broken_rules(g[20:], W, H, bits) == {RULE_OF[how]}, (W, H, depth, how, t)
                    if how == "depth":
                        assert len(g) == 20 + 12 + (1 + bits // 8) * T + 8 * int(g[24:24 + T].sum(dtype=np.int64))


def test_all_pairs_frame_wraps_every_minimum(oracle):
    """384 x 384 = 2304 tiles: every (depth 0..8, minimum 0..255) pair once; all-ones payload gives min + 2^d - 1."""
    rng = np.random.default_rng(7)
    fr = cr.all_pairs_frame(rng, "ones")
    adv, fh, img = cr.decode_frame(fr, 384, 384)
    assert (adv, fh) == oracle.unpack_frame(fr, 384, 384)[:2]
    assert np.array_equal(img, oracle.unpack_frame(fr, 384, 384)[2])
    t = img.reshape(48, 8, 48, 8).transpose(0, 2, 1, 3).reshape(2304, 64)
    d, m = np.repeat(np.arange(9), 256), np.tile(np.arange(256), 9)
    assert (t == ((m + (1 << d) - 1) & 255)[:, None]).all()


def test_layout_places_payloads_at_every_residue():
    rng = np.random.default_rng(3)
    frames = [cr.craft(rng, 40, 24) for _ in range(20)]
    buf, lead, offs, total = cr.layout(frames, "residues", lead=32)
    starts = [(lead + o + cr.payload_start(f)) % 16 for o, f in zip(offs, frames)]
    assert starts == [k % 16 for k in range(20)]
    for o, f in zip(offs, frames):
        assert np.array_equal(buf[lead + o: lead + o + len(f)], f)
    assert total == offs[-1] + len(frames[-1])
    buf, lead, offs, _ = cr.layout(frames, "offsets", lead=32)
    assert [(lead + o) % 16 for o in offs] == [k % 16 for k in range(20)]


def test_oracle_equals_reference_on_crafted_frames(oracle, reference):
    """No depth above 8 here: the reference does not check depths and would read out of bounds."""
    rng = np.random.default_rng(2016)
    for it in range(400):
        W, H = int(rng.integers(1, 70)), int(rng.integers(1, 70))
        fr = cr.craft(rng, W, H, 8, cr.DEPTHS[it % 6], cr.MINIMA[it % 3], cr.PAYLOADS[(it // 3) % 3])
        if it % 10 == 9:
            fr = cr.break_rule(fr, cr.BREAKS[1 + (it // 10) % (len(cr.BREAKS) - 1)])
        r_adv, r_fh, r_img = reference.unpack_frame(fr, W, H)
        o_adv, o_fh, o_img = oracle.unpack_frame(fr, W, H)
        assert (r_adv, r_fh) == (o_adv, o_fh), it
        assert np.array_equal(r_img, o_img), it


def test_oracle_equals_reference_on_crafted_headers(oracle, reference):
    rng = np.random.default_rng(4)
    heads = [(u, int(rng.integers(0, 1 << 62)), b) for u in cr.U64S for b in cr.SPECIAL_ELAPSED]
    heads += [cr.random_header(rng) for _ in range(3000)]
    for h in heads:
        hb = cr.frame_header(*h)
        assert reference.unpack_frame_header(hb) == oracle.unpack_frame_header(hb) == (20, cr.parse_header(hb)), h


def test_host_header_read_matches_the_pinned_reference(dv):
    """dbde_hip_unpack_frame_header (host code, no device) reads the F64 elapsed as the reference does."""
    for bits, want in PINNED_ELAPSED.items():
        for u64s in (2, 3):
            n, fh = dv.unpack_frame_header(cr.frame_header(u64s, 0x0123456789ABCDEF, bits))
            assert (n, fh) == (20, (2 if u64s == 2 else 0xFFFFFFFF, 0x0123456789ABCDEF, want)), hex(bits)


def test_host_header_read_matches_the_reference_live(dv, reference):
    rng = np.random.default_rng(5)
    heads = [cr.random_header(rng) for _ in range(4000)]
    heads += [(2, 1, b) for b in cr.SPECIAL_ELAPSED]
    for h in heads:
        hb = cr.frame_header(*h)
        assert dv.unpack_frame_header(hb) == reference.unpack_frame_header(hb), h


def test_shim_header_read_matches_the_pinned_reference(dv):
    """The dbde_util.h shim's dbde_unpack_frame_header forwards to the same host read."""
    class FH(C.Structure):
        _fields_ = [("u64s", C.c_uint32), ("index", C.c_uint64), ("elapsed_ns", C.c_uint64)]
    lib = C.CDLL(dv.SHIM_PATH)
    fn = getattr(lib, "_Z24dbde_unpack_frame_headerPPh")
    fn.restype = FH
    fn.argtypes = [C.POINTER(C.c_void_p)]
    for bits, want in PINNED_ELAPSED.items():
        hb = np.ascontiguousarray(cr.frame_header(2, 77, bits))
        cur = C.c_void_p(hb.ctypes.data)
        fh = fn(C.byref(cur))
        assert cur.value - hb.ctypes.data == 20
        assert (fh.u64s, fh.index, fh.elapsed_ns) == (2, 77, want), hex(bits)
