"""Shared by the GPU tests of the patch match (dbde_hip_match_patches / dbde16_hip_match_patches): frames given in numpy
encoded on the device, the call into 0xEE canvases with guard bands, and the exact comparison with tests/match_ref.py.
"""
import numpy as np

import match_ref as mr
import patch_ref as pr

GUARD = 64


class Encoded:
    """n numpy frames (uint8, or uint16 for bits=16) encoded on the device: buf, lead, total, offs, and the frames."""

    def __init__(self, codec, frames, bits=8, misalign=3):
        import torch
        frames = np.ascontiguousarray(frames)
        n, H, W = frames.shape
        self.W, self.H, self.n, self.bits, self.frames = W, H, n, bits, frames
        if bits == 8:
            buf, lead, cap = codec.alloc_stream(W, H, n, lead=48)
            self.lead = lead + misalign
            buf.fill_(0xA5)
            self.offs, sizes = codec.encode_frames(torch.from_numpy(frames).cuda(), W, H, n, buf, self.lead, cap)
        else:
            cap = n * int(codec.L.dbde16_hip_max_frame_bytes(W, H))
            self.lead = 48 + misalign
            buf = torch.full((self.lead + cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            self.offs, sizes = codec.encode_frames16(torch.from_numpy(frames.view(np.int16)).cuda(), W, H, n, buf, self.lead, cap)
        codec.sync()
        self.buf = buf
        self.total = int((self.offs[-1] + sizes[-1]).item())

    @property
    def stream(self):
        return self.buf, self.lead, self.total, self.offs


def dev_templates(T, bits):
    import torch
    T = np.ascontiguousarray(T)
    return torch.from_numpy(T if bits == 8 else T.view(np.int16)).cuda()


def run_match(codec, stream, W, H, n, T, S, origins, counts=None, mode=pr.CLAMP, fill=0, stats=7, bits=8, give_all=False):
    """Runs into 0xEE canvases with guard bands and checks the guards -> (prod, sum, sq (n, K, D, D) int64 -- all
    UNTOUCHED where not requested --, used (n, K, 2), results tensor).  give_all: the surfaces outside `stats` are
    passed too (through the C call: the Python call passes NULL for them) and must come back untouched."""
    import torch
    buf, lead, total, offs = stream
    origins = np.asarray(origins, np.int64).reshape(n, -1, 2)
    K, D = origins.shape[1], 2 * S + 1
    d_org = torch.from_numpy(origins.astype(np.int32)).cuda()
    d_cnt = None if counts is None else torch.from_numpy(np.asarray(counts, np.int64).astype(np.uint32).view(np.int32)).cuda()
    d_T = dev_templates(T, bits)
    per = K * D * D
    canv = [torch.full((n * per + 2 * GUARD,), mr.UNTOUCHED, dtype=torch.int64, device="cuda") for _ in range(3)]
    views = [c[GUARD: GUARD + n * per] for c in canv]
    ucanvas = torch.full((2 * n * K + 2 * GUARD,), pr.UNTOUCHED_ORIGIN, dtype=torch.int32, device="cuda")
    used = ucanvas[GUARD: GUARD + 2 * n * K]
    res = torch.empty((n, 4), dtype=torch.int64, device="cuda")
    edge = "clamp" if mode == pr.CLAMP else "fill"
    if give_all:
        fn = codec.L.dbde_hip_match_patches if bits == 8 else codec.L.dbde16_hip_match_patches
        rc = fn(codec.h, buf.data_ptr() + lead, total, offs.data_ptr(), W, H, n, T.shape[2], T.shape[1], S, K, d_org.data_ptr(),
                None if d_cnt is None else d_cnt.data_ptr(), mode, fill, d_T.data_ptr(), T.shape[0], stats,
                views[0].data_ptr(), views[1].data_ptr(), views[2].data_ptr(), used.data_ptr(), res.data_ptr())
        assert rc == 0, rc
    else:
        fn = codec.match_patches if bits == 8 else codec.match_patches16
        out = {nm: views[i] for i, nm in enumerate(mr.NAMES) if stats >> i & 1}
        pm, res = fn(buf, lead, total, offs, W, H, n, d_T, S, d_org, counts=d_cnt, edge=edge, fill=fill, stats=stats,
                     out=out, used=used, results=res)
        assert [getattr(pm, nm) is not None for nm in mr.NAMES] == [bool(stats >> i & 1) for i in range(3)]
        T64 = T.astype(np.int64)
        assert pm.t_sum.cpu().tolist() == T64.sum((1, 2)).tolist() and pm.t_sq.cpu().tolist() == (T64 * T64).sum((1, 2)).tolist()
    codec.sync()
    got = []
    for c, nm in zip(canv, mr.NAMES):
        h = c.cpu().numpy()
        assert (h[:GUARD] == mr.UNTOUCHED).all(), f"wrote in front of {nm}"
        assert (h[-GUARD:] == mr.UNTOUCHED).all(), f"wrote behind {nm}"
        got.append(h[GUARD:-GUARD].reshape(n, K, D, D))
    u = ucanvas.cpu().numpy()
    assert (u[:GUARD] == pr.UNTOUCHED_ORIGIN).all() and (u[-GUARD:] == pr.UNTOUCHED_ORIGIN).all(), "wrote outside the used origins"
    return got[0], got[1], got[2], u[GUARD:-GUARD].reshape(n, K, 2), res


def check_match(codec, stream, frames, W, H, T, S, origins, counts=None, mode=pr.CLAMP, fill=0, stats=7, bits=8,
                give_all=False, what=""):
    """frames: the expected images, None for rejected frames.  Exact equality of every surface (the unrequested ones
    and the dead entries: untouched) and of the used origins with tests/match_ref.py."""
    n = len(frames)
    got = run_match(codec, stream, W, H, n, T, S, origins, counts, mode, fill, stats, bits, give_all)
    want = mr.expected(frames, W, H, T, S, origins, counts, mode, fill)
    where = f"{what} {W}x{H} template {T.shape[2]}x{T.shape[1]} S {S} mode {mode} stats {stats} bits {bits}"
    for i, nm in enumerate(mr.NAMES):
        w = want[i] if stats >> i & 1 else np.full_like(want[i], mr.UNTOUCHED)
        if not np.array_equal(got[i], w):
            f, k, r, c = np.argwhere(got[i] != w)[0]
            o = np.asarray(origins).reshape(n, -1, 2)[f, k]
            raise AssertionError(f"{where}: {nm}: frame {f} patch {k} origin {tuple(o)}: {int((got[i] != w).sum())} entries "
                                 f"differ, first at dy {r - S} dx {c - S}: got {got[i][f, k, r, c]} want {w[f, k, r, c]}")
    assert np.array_equal(got[3], want[3]), f"{where}: used origins"
    return got[4]


# ---- the bodies of tests/test_gpu_match.py (bits = 8) and tests/test_gpu_match16.py (bits = 16) ----------------------
def run_case(codec, c, bits):
    """One case of tests/match_cases.py: its content encoded, matched and compared."""
    import match_cases as mc
    frames, T, org, counts = mc.content(c, bits)
    e = Encoded(codec, frames, bits)
    res = check_match(codec, e.stream, list(frames), c["W"], c["H"], T, c["S"], org, counts, c["mode"], mc.fill_of(c, bits),
                      c["stats"], bits, give_all=c["stats"] != 7, what=c["name"])
    if c["stats"] != 7:   # the same through the Python call, which passes NULL for the surfaces outside the mask
        check_match(codec, e.stream, list(frames), c["W"], c["H"], T, c["S"], org, counts, c["mode"], mc.fill_of(c, bits),
                    c["stats"], bits, what=c["name"] + " NULL")
    return res


def crafted_stream(rng, W, H, n, bad, bits):
    """n crafted frames, those in `bad` with one validity rule broken (crafted.break_rule) -> (stream, images with None
    for the broken ones)."""
    import torch
    import crafted as cr
    frames, images = [], []
    for f in range(n):
        fr = cr.craft(rng, W, H, bits, cr.DEPTHS[f % len(cr.DEPTHS)], cr.MINIMA[f % len(cr.MINIMA)], cr.PAYLOADS[f % len(cr.PAYLOADS)])
        if f in bad:
            fr = cr.break_rule(fr, bad[f], bits, tile=int(rng.integers(0, cr.tiles(W, H))))
        frames.append(fr)
        images.append(cr.decode_frame(fr, W, H, bits)[2])
    buf, lead, offs, total = cr.layout(frames, "residues", lead=32)
    return (torch.from_numpy(buf).cuda(), lead, total, torch.from_numpy(offs).cuda()), images


def run_rejected(codec, bits):
    """Crafted streams with a bad-header frame first, in the middle and last, and a last frame cut short by
    stream_bytes: their surfaces and used origins keep the canvas, the results are decode_frames', neighbours exact."""
    import torch
    W, H, n, S = 139, 99, 5, 2
    rng = np.random.default_rng(91 + bits)
    top = 255 if bits == 8 else 65535
    T = rng.integers(0, top + 1, size=(4, 12, 16)).astype(np.uint8 if bits == 8 else np.uint16)
    org = np.array([[(-3, -2), (60, 40), (W - 17, H - 13), (33, 70)]] * n)
    decode = codec.decode_frames if bits == 8 else codec.decode_frames16
    for bad in ({0: "T+1"}, {2: "n64-1"}, {n - 1: "depth"}, {0: "nm+1", 2: "depth", n - 1: "T-1"}):
        stream, images = crafted_stream(rng, W, H, n, bad, bits)
        assert [im is None for im in images] == [f in bad for f in range(n)]
        _, want_res = decode(stream[0], stream[1], stream[2], stream[3], W, H, n)
        for mode in (pr.CLAMP, pr.FILL):
            res = check_match(codec, stream, images, W, H, T, S, org, None, mode, 5, 7, bits, what=f"rejected {sorted(bad)}")
            assert torch.equal(res, want_res)
    stream, images = crafted_stream(rng, W, H, n, {}, bits)   # truncated: one byte short rejects the last frame only
    cut = (stream[0], stream[1], stream[2] - 1, stream[3])
    res = check_match(codec, cut, images[:-1] + [None], W, H, T, S, org, [4, 2, 9, 0, 4], pr.FILL, 1, 7, bits, what="truncated")
    assert codec.parse_results(res)[-1][0] == 0xFFFFFFFF
    check_match(codec, stream, images, W, H, T, S, org, None, pr.CLAMP, 0, 7, bits, what="whole")


def run_overflow_witness(codec, bits):
    """128 x 128 at S = 16 on all-maximum content with an all-maximum template, against the closed form: prod = sq =
    128^2 top^2 (8 bits: 1,065,369,600 < 2^32, the U32 chain's bound; 16 bits: about 2^46), sum = 128^2 top."""
    top = 255 if bits == 8 else 65535
    dt = np.uint8 if bits == 8 else np.uint16
    W, H, n, S = 200, 163, 2, 16
    frames = np.full((n, H, W), top, dt)
    T = np.full((1, 128, 128), top, dt)
    org = np.array([[(0, 0), (40, 3), (17, 1)]] * n)
    e = Encoded(codec, frames, bits)
    prod, sm, sq, _, _ = run_match(codec, e.stream, W, H, n, T, S, org, None, pr.CLAMP, 0, 7, bits)
    assert (prod == 128 * 128 * top * top).all() and (sq == 128 * 128 * top * top).all() and (sm == 128 * 128 * top).all()
    # and with the patch hanging over the frame's edge into a fill of the maximum: the same
    prod, sm, sq, _, _ = run_match(codec, e.stream, W, H, n, T, S, org - 30, None, pr.FILL, top, 7, bits)
    assert (prod == 128 * 128 * top * top).all() and (sq == 128 * 128 * top * top).all() and (sm == 128 * 128 * top).all()


def run_cross_check(codec, bits):
    """The library's own cross-check: decode_patches of the search patches, then the surfaces in torch (unfold, int64)."""
    import torch
    import match_cases as mc
    c = next(c for c in mc.CASES if c["name"] == "t16x12_S8")
    frames, T, org, _ = mc.content(c, bits)
    W, H, n, S, tw, th = c["W"], c["H"], c["n"], c["S"], c["tw"], c["th"]
    e = Encoded(codec, frames, bits)
    d_org = torch.from_numpy(org.astype(np.int32)).cuda()
    d_T = dev_templates(T, bits)
    edge = "clamp" if c["mode"] == pr.CLAMP else "fill"
    fill = mc.fill_of(c, bits)
    match, dec = (codec.match_patches, codec.decode_patches) if bits == 8 else (codec.match_patches16, codec.decode_patches16)
    pm, _ = match(*e.stream, W, H, n, d_T, S, d_org, edge=edge, fill=fill)
    P, _ = dec(*e.stream, W, H, n, tw + 2 * S, th + 2 * S, d_org, edge=edge, fill=fill)
    P = P.to(torch.int64) & (255 if bits == 8 else 65535)
    T64 = d_T.to(torch.int64) & (255 if bits == 8 else 65535)
    win = P.unfold(2, th, 1).unfold(3, tw, 1)                  # (n, K, D, D, th, tw)
    Tk = T64.expand(P.shape[1], th, tw)[None, :, None, None]
    assert torch.equal(pm.prod, (win * Tk).sum((4, 5))) and torch.equal(pm.sum, win.sum((4, 5)))
    assert torch.equal(pm.sq, (win * win).sum((4, 5)))
    assert torch.equal(pm.ssd(), ((win - Tk) ** 2).sum((4, 5)))
    z = pm.zncc()
    wf, tf = win.to(torch.float64), Tk.to(torch.float64)
    wz, tz = wf - wf.mean((4, 5), keepdim=True), tf - tf.mean((4, 5), keepdim=True)
    want = (wz * tz).sum((4, 5)) / torch.sqrt((wz * wz).sum((4, 5)) * (tz * tz).sum((4, 5)))
    assert torch.allclose(z, want, rtol=0, atol=1e-9)   # float64 sums of at most 192 centred products: far below 1e-9
