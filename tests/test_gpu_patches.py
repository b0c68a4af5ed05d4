"""GPU: patch decode -- dbde_hip_decode_patches (Codec.decode_patches): K small windows per frame in one call.

Every patch is compared byte for byte with tests/patch_ref.py over the oracle's decode of the whole frame (for crafted
frames: crafted.decode_frame's), decoded into a 0xEE canvas with guard bands in front of and behind the patches and
the used origins; rejections are compared with what dbde_hip_decode_frames reports for the same batch.
"""
import numpy as np
import pytest

import patch_ref as pr
from test_gpu_project import Crafted
from test_gpu_roi import MODES, Batch

pytestmark = pytest.mark.gpu

GUARD = 64
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


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


def run_patches(codec, buf, lead, total, offs, W, H, n, pw, ph, origins, counts=None, mode=pr.CLAMP, fill=0,
                out_misalign=0, bits=8):
    """Decodes into 0xEE canvases with guard bands; checks the guards -> (patches (n, K, ph, pw), used (n, K, 2),
    results tensor).  out_misalign: in pixels."""
    import torch
    pix = bits // 8
    origins = np.asarray(origins, np.int64).reshape(n, -1, 2)
    K = origins.shape[1]
    d_org = torch.from_numpy(origins.astype(np.int32)).cuda()
    d_cnt = None if counts is None else torch.from_numpy(np.asarray(counts, np.int64).astype(np.uint32).view(np.int32)).cuda()
    npx = n * K * ph * pw
    lo = GUARD + pix * out_misalign
    canvas = torch.full((npx * pix + 2 * GUARD + 32,), 0xEE, dtype=torch.uint8, device="cuda")
    out = canvas[lo: lo + npx * pix]
    out = out if bits == 8 else out.view(torch.int16)
    ucanvas = torch.full((2 * n * K + 2 * GUARD,), pr.UNTOUCHED_ORIGIN, dtype=torch.int32, device="cuda")
    used = ucanvas[GUARD: GUARD + 2 * n * K]
    fn = codec.decode_patches if bits == 8 else codec.decode_patches16
    got, res = fn(buf, lead, total, offs, W, H, n, pw, ph, d_org, counts=d_cnt, edge="clamp" if mode == pr.CLAMP else "fill",
                  fill=fill, out=out, used=used)
    codec.sync()
    c = canvas.cpu().numpy()
    assert (c[:lo] == 0xEE).all(), "wrote in front of the patches"
    assert (c[lo + npx * pix:] == 0xEE).all(), "wrote behind the patches"
    u = ucanvas.cpu().numpy()
    assert (u[:GUARD] == pr.UNTOUCHED_ORIGIN).all() and (u[GUARD + 2 * n * K:] == pr.UNTOUCHED_ORIGIN).all(), \
        "wrote outside the used origins"
    patches = c[lo: lo + npx * pix].view(np.uint8 if bits == 8 else np.uint16).reshape(n, K, ph, pw)
    return patches, u[GUARD: GUARD + 2 * n * K].reshape(n, K, 2), res


def check_patches(codec, src, frames, W, H, pw, ph, origins, counts=None, mode=pr.CLAMP, fill=0, out_misalign=0, bits=8,
                  stream=None, what=""):
    """src: anything with buf, lead, total, offs.  frames: the expected images, None for rejected frames."""
    n = len(frames)
    buf, lead, total, offs = stream if stream is not None else (src.buf, src.lead, src.total, src.offs)
    got, used, res = run_patches(codec, buf, lead, total, offs, W, H, n, pw, ph, origins, counts, mode, fill, out_misalign,
                                 bits)
    canvas = 0xEE if bits == 8 else 0xEEEE
    want, want_used, _ = pr.expected(frames, W, H, pw, ph, origins, counts, mode, fill, untouched=canvas,
                                     dtype=np.uint8 if bits == 8 else np.uint16)
    if not np.array_equal(got, want):
        f, k, r, c = np.argwhere(got != want)[0]
        o = np.asarray(origins).reshape(n, -1, 2)[f, k]
        raise AssertionError(f"{what} {W}x{H} patch {pw}x{ph} mode {mode}: frame {f} patch {k} origin {tuple(o)}: "
                             f"{int((got != want).sum())} pixels differ, first at ({r},{c}): got {got[f, k, r, c]} want "
                             f"{want[f, k, r, c]}")
    assert np.array_equal(used, want_used), f"{what} {W}x{H} patch {pw}x{ph} mode {mode}: used origins"
    return res


def origins_for(rng, W, H, pw, ph, n):
    """(n, K, 2): corners and edges, coinciding and overlapping patches, several in one tile row, every residue of x
    and y mod 8, origins outside the frame and at the ends of int32, random ones; a different order per frame."""
    mx, my = max(W - pw, 0), max(H - ph, 0)
    base = [(0, 0), (W - pw, 0), (0, H - ph), (W - pw, H - ph), (mx // 2, 0), (0, my // 2), (W - pw, my // 2),
            (mx // 2, H - ph),
            (mx // 3, my // 3), (mx // 3, my // 3),                      # two identical
            (mx // 3 + 1, my // 3 + 1), (mx // 3 + pw // 2, my // 3),   # overlapping
            (1, my // 2), (1 + pw, my // 2), (3 + 2 * pw, my // 2),     # several in one tile row
            (-3, -2), (W - 2, H - 1), (W + 5, 5), (-pw - 1, 0), (-pw + 1, -ph + 1), (5, H), (W, H), (-pw, -ph),
            (4090 - pw // 2, 0), (4095, 1), (4096 - pw, 0),             # (the 512-tile piece boundary of wide frames)
            (I32_MIN, I32_MAX), (I32_MAX, I32_MIN), (I32_MIN, 0), (0, I32_MAX), (I32_MAX, I32_MAX), (I32_MIN, I32_MIN)]
    for r in range(8):
        base.append((r + 8 * int(rng.integers(0, mx // 8 + 1)), (7 - r) + 8 * int(rng.integers(0, my // 8 + 1))))
        base.append((8 * int(rng.integers(0, mx // 8 + 1)) - r, 8 * int(rng.integers(0, my // 8 + 1)) + r))
    for _ in range(8):
        base.append((int(rng.integers(-pw, W + 1)), int(rng.integers(-ph, H + 1))))
    out = np.array(base, np.int64)
    return np.stack([out[rng.permutation(len(out))] for _ in range(n)])


SIZES = [(1, 1), (8, 8), (9, 9), (32, 32), (57, 57), (58, 58), (505, 3), (3, 300), (16, 7)]

# 4096x24: 512 tiles across (prefixes up to 511 bytes); 8200x17: 512-tile chunk pieces; 16x262152: more tile rows than
# the index has chunks, so plain 512-tile chunks (roi_index_geometry's else branch)
GEOMETRIES = [(4096, 24, 3), (8200, 17, 2), (513, 17, 3), (1921, 25, 3), (72, 72, 4), (10, 10, 3), (1, 1, 3)]


def sizes_for(W, H):
    s = list(SIZES)
    if W <= 505:
        s += [(W, H), (W, 1), (1, H)]
    return s


@pytest.mark.parametrize("W,H,n", GEOMETRIES)
def test_patches_match_patch_ref(codec, oracle, dv, W, H, n):
    rng = np.random.default_rng(W * 7919 + H)
    batches = [Batch(codec, oracle, mode, W, H, n, first=3 + i, misalign=(0, 1, 3, 6)[i]) for i, mode in enumerate(MODES)]
    for j, (pw, ph) in enumerate(sizes_for(W, H)):
        b = batches[j % len(batches)]   # the sizes are dealt round-robin over the content modes
        org = origins_for(rng, W, H, pw, ph, n)
        K = org.shape[1]
        counts = [None, [K] * n, [0] * n, [K + 5, 1, K // 2, 0][:n], None][j % 5]
        check_patches(codec, b, b.full, W, H, pw, ph, org, counts, pr.FILL, fill=(0x5A, 0, 0xFF)[j % 3], out_misalign=j % 16,
                      what=f"fill {MODES[j % 4]}")
        if pw <= W and ph <= H:
            res = check_patches(codec, b, b.full, W, H, pw, ph, org, counts, pr.CLAMP, out_misalign=(j + 7) % 16,
                                what=f"clamp {MODES[j % 4]}")
            assert all(r == (2, b.first + f, 0, len(b.packed[f])) for f, r in enumerate(codec.parse_results(res)))


def test_plain_chunk_index_fallback(codec, oracle, dv):
    """16 x 262152: 32769 tile rows, one more than the index has chunks per frame: plain 512-tile chunks."""
    W, H, n = 16, 262152, 2
    plan = dv.patches_plan(W, H, n, 9, 9, 4)
    assert plan["chunk_pieces"] == 0 and plan["chunk_tiles"] == 512
    b = Batch(codec, oracle, "mixed", W, H, n, first=1)
    rng = np.random.default_rng(5)
    for pw, ph in ((9, 9), (16, 58), (3, 300)):
        org = origins_for(rng, W, H, pw, ph, n)
        org[:, :4, 1] = [H - ph - 4097, 4091, 131072 - ph // 2, H - 8 * 511 - 3]
        check_patches(codec, b, b.full, W, H, pw, ph, org, None, pr.CLAMP, out_misalign=3)
        check_patches(codec, b, b.full, W, H, pw, ph, org, None, pr.FILL, fill=7, out_misalign=5)


@pytest.mark.parametrize("mode", (pr.CLAMP, pr.FILL))
def test_every_output_alignment_and_origin_residue(codec, oracle, mode):
    W, H, n = 200, 123, 2
    b = Batch(codec, oracle, "noise8", W, H, n, first=9)
    org = np.array([[(x0 + 8 * (x0 % 3), y0 + 8 * (y0 % 5)) for x0 in range(8) for y0 in range(8)]] * n)
    for mis in range(16):
        pw, ph = (32, 32) if mis % 2 else (13 + mis, 11)
        check_patches(codec, b, b.full, W, H, pw, ph, org + (mis - 8 if mode == pr.FILL else 0), None, mode, fill=0x11,
                      out_misalign=mis)


def test_clamp_patches_equal_decode_roi(codec, oracle):
    import torch
    W, H, n = 1921, 97, 3
    b = Batch(codec, oracle, "mixed", W, H, n, first=2)
    rng = np.random.default_rng(11)
    for pw, ph in ((32, 32), (58, 58), (505, 3), (7, 97)):
        org = origins_for(rng, W, H, pw, ph, n)
        got, used, _ = run_patches(codec, b.buf, b.lead, b.total, b.offs, W, H, n, pw, ph, org)
        for k in range(0, org.shape[1], 5):
            d_o = torch.from_numpy(org[:, k].astype(np.int32)).cuda()
            win, _ = codec.decode_roi(b.buf, b.lead, b.total, b.offs, W, H, n, 0, 0, pw, ph, origins=d_o)
            codec.sync()
            assert np.array_equal(win.cpu().numpy(), got[:, k]), (pw, ph, k)


@pytest.mark.parametrize("W,H,n,mode", [(64, 64, 3, "noise8"), (1921, 17, 2, "mixed"), (10, 10, 4, "smooth")])
def test_patches_read_nothing_past_stream_bytes(codec, oracle, W, H, n, mode):
    """stream_bytes ends exactly at the last frame's end, at every residue mod 16, with junk behind it; one byte short
    rejects the last frame only, whose patches and used origins stay untouched."""
    import torch
    b = Batch(codec, oracle, mode, W, H, n, first=3)
    pw, ph = min(W, 33), min(H, 9)
    org = np.array([[(W - pw, H - ph), (W - 3, H - 2), (0, 0), (W - pw - 1, H - ph)]] * n)
    for pad in range(16):
        junk = (0xA5, 0x00, 0xFF)[pad % 3]
        t = torch.full((pad + b.total + 48,), junk, dtype=torch.uint8, device="cuda")
        t[pad:pad + b.total] = b.buf[b.lead:b.lead + b.total]
        for m in (pr.CLAMP, pr.FILL):
            check_patches(codec, b, b.full, W, H, pw, ph, org, None, m, fill=9, stream=(t, pad, b.total, b.offs))
            res = check_patches(codec, b, b.full[:-1] + [None], W, H, pw, ph, org, None, m, fill=9,
                                stream=(t, pad, b.total - 1, b.offs))
            assert codec.parse_results(res)[-1][0] == 0xFFFFFFFF


@pytest.mark.parametrize("W,H,n,how", [(64, 48, 40, "concat"), (200, 123, 23, "residues"), (1921, 17, 9, "slots"),
                                       (4200, 9, 7, "concat")])
def test_crafted_and_rejected_frames(codec, W, H, n, how):
    """Every depth 0..8 at every payload byte alignment, wrapping minima, frames with one rule broken between good
    ones: a rejected frame's patches and used origins keep the canvas, results are decode_frames', neighbours exact."""
    import torch
    rng = np.random.default_rng(W * 7919 + H)
    s = Crafted(rng, W, H, n, how)
    assert any(im is None for im in s.images) and any(im is not None for im in s.images)
    _, want_res = codec.decode_frames(s.buf, s.lead, s.total, s.offs, W, H, n)
    for pw, ph in ((32, min(H, 32)), (9, 9), (min(W, 505), 3), (58, min(H, 58))):
        org = origins_for(rng, W, H, pw, ph, n)
        for m in (pr.CLAMP, pr.FILL):
            res = check_patches(codec, s, s.images, W, H, pw, ph, org, None, m, fill=0xC3, out_misalign=pw % 16,
                                what=f"crafted {how}")
            assert torch.equal(res, want_res)


def test_timing_hook_zero_frames_and_argument_errors(codec, oracle, dv):
    import torch
    W, H, n = 300, 200, 2
    b = Batch(codec, oracle, "mixed", W, H, n)
    org = torch.zeros((n, 3, 2), dtype=torch.int32, device="cuda")
    codec.timing(True)
    codec.timing_read(reset=True)
    codec.decode_patches(b.buf, b.lead, b.total, b.offs, W, H, n, 32, 32, org)
    t = codec.timing_read(reset=True)
    codec.timing(False)
    assert t["decode_index"][1] == 1 and t["decode"][1] == 1 and t["encode"][1] == 0
    out = torch.full((64,), 0xEE, dtype=torch.uint8, device="cuda")
    rc = codec.L.dbde_hip_decode_patches(codec.h, b.buf.data_ptr() + b.lead, b.total, b.offs.data_ptr(), W, H, 0, 2, 2, 3,
                                         org.data_ptr(), None, 0, 0, out.data_ptr(), None, None)
    codec.sync()
    assert rc == dv.OK and (out == 0xEE).all()
    big = torch.full((n * 3 * 8 * 8,), 0xEE, dtype=torch.uint8, device="cuda")
    for kw in (dict(pw=506), dict(pw=0), dict(ph=0), dict(pw=301), dict(ph=201), dict(edge=2), dict(fill=256),
               dict(pw=301, edge="fill", fill=256)):
        a = dict(pw=8, ph=8, edge="clamp", fill=0)
        a.update(kw)
        with pytest.raises(dv.DbdeError, match="decode_patches"):
            codec.decode_patches(b.buf, b.lead, b.total, b.offs, W, H, n, a["pw"], a["ph"], org, edge=a["edge"],
                                 fill=a["fill"], out=None if a["pw"] != 8 or a["ph"] != 8 else big)
    rc = codec.L.dbde_hip_decode_patches(codec.h, b.buf.data_ptr() + b.lead, b.total, b.offs.data_ptr(), W, H, n, 8, 8, 3,
                                         None, None, 0, 0, big.data_ptr(), None, None)
    assert rc == dv.ERR_ARG
    codec.sync()
    assert (big == 0xEE).all()
    for bad in (org.to(torch.int64), org[:, :, :1], org.permute(1, 0, 2), org[:1]):
        with pytest.raises(ValueError, match="origins"):
            codec.decode_patches(b.buf, b.lead, b.total, b.offs, W, H, n, 8, 8, bad)
    # pw > W is legal in fill mode
    check_patches(codec, b, b.full, W, H, 400, 3, np.array([[(-50, 100), (0, 199), (-99, -1)]] * n), None, pr.FILL, fill=1)

