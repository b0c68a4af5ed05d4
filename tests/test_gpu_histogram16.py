"""GPU: DBDE16 per-frame histograms -- dbde16_hip_histogram (Codec.histogram16).

Expected values are exact integer counts: torch.bincount of the windows of dbde16_hip_decode_frames' images (and of
the DBDE16 oracle's), v >> shift clamped into the last bin.  Depths 0-16, 12-bit content, every binning rule.
"""
import numpy as np
import pytest

from family_refs import hist_expect16 as expect16
from test_gpu_roi16 import KINDS, Batch16, images16
from test_oracle_u16 import o16, unpack16   # noqa: F401  (fixture + helper)

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0x5A5A5A5A


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


def twelve_bit(rng, n, W, H):
    base = rng.integers(0, 4096, size=(n, 1, 1))
    img = (base + rng.integers(-40, 41, size=(n, H, W))).clip(0, 4095)
    img[:, ::5, ::3] = rng.integers(0, 4096, size=img[:, ::5, ::3].shape)
    return np.ascontiguousarray(img.astype(np.uint16))


def run(codec, b, x, y, rw, rh, **kw):
    h, res = codec.histogram16(b.buf, b.lead, kw.pop("stream_bytes", b.total), b.offs, b.W, b.H, b.n, x, y, rw, rh,
                               **kw)
    codec.sync()
    return h, res


BINNINGS = [(0, None), (4, 4096), (0, 4096), (8, 256), (3, 100), (15, 2), (0, 1), (9, 37)]
GEOMETRIES = [(1, 1, 3), (8, 8, 2), (9, 9, 3), (200, 123, 2), (1921, 1081, 2), (4096, 3072, 1)]


@pytest.mark.parametrize("W,H,n", GEOMETRIES)
def test_kinds_and_binnings(dv, codec, o16, W, H, n):
    import torch
    rng = np.random.default_rng(W * 7919 + H * 31 + n)
    kinds = KINDS + ("twelve",)
    for i, kind in enumerate(kinds):
        imgs = twelve_bit(rng, n, W, H) if kind == "twelve" else images16(rng, n, W, H, kind)
        b = Batch16(codec, o16, imgs, first=3 + i, shift=i)
        wins = [(0, 0, W, H), (W - 1, H - 1, 1, 1)]
        if W > 3 and H > 3:
            wins.append((1 + W // 7, 1 + H // 5, max(1, W // 2 - 1), max(1, H // 2 - 1)))
        for k, win in enumerate(wins):
            for j, (shift, bins) in enumerate(BINNINGS):
                if W * H > 100000 and (j + i + k) % 3 != 0:
                    continue
                nb = dv.max_bins(2, shift) if bins is None else bins
                h, res = run(codec, b, *win, shift=shift, bins=bins, total=True)
                want = expect16(b.gpu_full, *win, shift, nb)
                assert torch.equal(expect16(b.full, *win, shift, nb), want)
                got = h.counts.to(torch.int64).cpu()
                assert torch.equal(got, want), f"{kind} {W}x{H} {win} shift {shift} bins {nb}"
                assert (got.sum(1) == win[2] * win[3]).all()
                assert torch.equal(h.total.cpu(), want.sum(0)) and int(h.count.item()) == n
                assert codec.parse_results(res) == [(2, b.first + f, 0, len(b.packed[f])) for f in range(n)]


@pytest.mark.parametrize("slot", [0, 4096 * 3 * 2 + 7])
def test_layouts_and_stream_end(dv, codec, o16, slot):
    import torch
    W, H, n = 203, 19, 3
    for shift in (0, 5, 11):
        rng = np.random.default_rng(300 + shift)
        b = Batch16(codec, o16, images16(rng, n, W, H, "full"), slot_stride=slot, shift=shift, junk=0x5A + shift)
        h, _ = run(codec, b, 0, 0, W, H, bins=4096)
        assert torch.equal(h.counts.to(torch.int64).cpu(), expect16(b.full, 0, 0, W, H, 0, 4096))


def test_rejected_frames_keep_their_rows(dv, codec, o16):
    """Depth byte 17, nm == T, an n64 mismatch and a truncated last frame: rejected rows stay as they were and add
    nothing to the total; results equal dbde16_hip_decode_frames'."""
    import torch
    W, H, n = 61, 37, 5
    rng = np.random.default_rng(9)
    b = Batch16(codec, o16, images16(rng, n, W, H, "mixed"), first=40)
    T = ((W + 7) // 8) * ((H + 7) // 8)
    o = b.offs.cpu().numpy()
    host = b.buf.cpu().numpy()
    base = b.lead
    host[base + o[0] + 24 + 3] = 17
    host[base + o[1] + 24 + T: base + o[1] + 28 + T] = np.frombuffer(np.int32(T).tobytes(), np.uint8)
    n64 = base + o[3] + 28 + 3 * T
    host[n64: n64 + 4] = np.frombuffer(np.int32(int(host[n64: n64 + 4].view("<i4")[0]) + 1).tobytes(), np.uint8)
    buf = torch.from_numpy(host).cuda()
    truncated = b.total - 1
    bins = 300
    out = dv.Histograms(torch.full((n, bins), -3, dtype=torch.int32, device="cuda"),
                        torch.full((bins,), 5, dtype=torch.int64, device="cuda"),
                        torch.full((1,), 5, dtype=torch.int64, device="cuda"))
    h, res = codec.histogram16(buf, b.lead, truncated, b.offs, W, H, n, 5, 3, 17, 30, shift=6, bins=bins, total=True,
                               out=out)
    _, want_res = codec.decode_frames16(buf, b.lead, truncated, b.offs, W, H, n)
    codec.sync()
    assert torch.equal(res, want_res)
    got = h.counts.to(torch.int64).cpu()
    want = expect16(b.full, 5, 3, 17, 30, 6, bins)
    assert torch.equal(got[2], want[2])
    for f in (0, 1, 3, 4):
        assert (got[f] == -3).all(), f
    assert torch.equal(h.total.cpu(), want[2]) and int(h.count.item()) == 1


def test_accumulate_and_guards(dv, codec, o16):
    import torch
    W, H, n, bins = 200, 123, 6, 4096
    rng = np.random.default_rng(77)
    b = Batch16(codec, o16, twelve_bit(rng, n, W, H))
    rows = torch.full((2 * GUARD + n * bins,), SENTINEL, dtype=torch.int32, device="cuda")
    tot = torch.full((2 * GUARD + bins + 1,), SENTINEL, dtype=torch.int64, device="cuda")
    out = dv.Histograms(rows[GUARD:GUARD + n * bins].view(n, bins), tot[GUARD:GUARD + bins],
                        tot[GUARD + bins:GUARD + bins + 1])
    h, _ = codec.histogram16(b.buf, b.lead, b.total, b.offs, W, H, n, 3, 4, 190, 100, bins=bins, total=True, out=out)
    codec.sync()
    want = expect16(b.full, 3, 4, 190, 100, 0, bins)
    assert torch.equal(h.counts.to(torch.int64).cpu(), want)
    assert torch.equal(h.total.cpu(), want.sum(0)) and int(h.count.item()) == n
    r, t = rows.cpu(), tot.cpu()
    assert (r[:GUARD] == SENTINEL).all() and (r[GUARD + n * bins:] == SENTINEL).all()
    assert (t[:GUARD] == SENTINEL).all() and (t[GUARD + bins + 1:] == SENTINEL).all()
    acc = None
    for lo, hi in ((0, 1), (1, 4), (4, 6)):
        acc, _ = codec.histogram16(b.buf, b.lead, b.total, b.offs[lo:hi], W, H, hi - lo, 3, 4, 190, 100, bins=bins,
                                   per_frame=False, total=True, out=acc, accumulate=acc is not None)
    codec.sync()
    assert torch.equal(acc.total.cpu(), want.sum(0)) and int(acc.count.item()) == n
    for q in (0.0, 0.01, 0.5, 0.99, 1.0):
        w = torch.from_numpy(np.asarray(b.full)[:, 4:104, 3:193].reshape(n, -1).astype(np.int64))
        k = int(np.floor(q * (w.shape[1] - 1))) + 1
        assert torch.equal(h.quantile(q).cpu(), torch.kthvalue(w, k, dim=1).values), q


def test_argument_errors(dv, codec, o16):
    rng = np.random.default_rng(1)
    b = Batch16(codec, o16, images16(rng, 2, 64, 48, "mixed"))
    for kw in (dict(shift=16, bins=1), dict(shift=0, bins=4097), dict(shift=5, bins=2049), dict(shift=-1, bins=1),
               dict(per_frame=False, total=False)):
        with pytest.raises((dv.DbdeError, ValueError)):
            codec.histogram16(b.buf, b.lead, b.total, b.offs, 64, 48, 2, **kw)
