"""GPU: registered projections -- dbde_hip_project_registered (Codec.project_registered).

Every plane, the count and origins_used are compared for equality with tests/registered_ref.py -- the definition in
numpy over decoded images -- on streams crafted on the host (tests/registered_cases.py lists the cases;
tests/test_registered_ref.py holds the cap on each of them before any GPU run).  Nothing expected comes from the call
itself, except where a test says that it compares the library with itself.  The bodies live in the `Registered` class
so that tests/test_gpu_registered16.py runs the same ones at 16 bits.
"""
import numpy as np
import pytest

import lag_gpu as lg
import registered_cases as rc
import registered_gpu as rg
import registered_ref as rr
import wproject_gpu as wg

pytestmark = pytest.mark.gpu


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


@pytest.fixture(scope="module")
def cus(codec):
    return wg.cus_of(codec)


def sentinels(dv, rh, rw, bits, value=-77):
    """A Projection whose four planes and count hold a sentinel."""
    out = dv.Projection.empty(rh, rw, rr.STATS, "cuda", pix=bits // 8)
    for k in rr.STATS:
        getattr(out, k).fill_(value if k in ("sum", "sumsq") or bits == 16 else 0xB3)
    out.count.fill_(value)
    return out


class Registered:
    """The cases at one pixel size (BITS)."""
    BITS = 8

    def call(self, codec):
        return rg.call_of(codec, self.BITS)

    def plan(self, dv):
        return dv.registered_plan if self.BITS == 8 else dv.registered16_plan

    def cols(self):
        return 248 if self.BITS == 8 else 120

    @pytest.mark.parametrize("row", range(8))
    def test_each_residue_alone(self, codec, row):
        rg.run(codec, rc.residues_each(self.BITS)[8 * row:8 * row + 8])

    def test_all_residues_in_one_call(self, codec):
        rg.run(codec, rc.residues_all(self.BITS))

    def test_windows(self, dv, codec):
        """The full frame (every origin clamps to (0, 0): project's result), 1 x 1, and a window whose last band has
        fewer than 8 rows at the frame's far corner, with H % 8 != 0 and == 0."""
        import torch
        cases = rc.windows(self.BITS)
        rg.run(codec, cases)
        name, spec, rw, rh, origins, mask = cases[0]
        s = lg.stream(*spec)
        reg, _ = rg.check(codec, cases[0])
        proj = codec.project if self.BITS == 8 else codec.project16
        fixed, _ = proj(s.buf, s.lead, s.total, s.offs, s.W, s.H, s.n)
        codec.sync()
        for k in rr.STATS + ("count",):
            assert torch.equal(getattr(reg, k), getattr(fixed, k)), k

    def test_more_than_one_piece_across(self, dv, codec):
        case = rc.wide(self.BITS)[0]
        p = self.plan(dv)(*rc.WIDE, 7, case[2], case[3])
        assert p["piece_cols"] == self.cols() and p["pieces_x"] == (2 if self.BITS == 8 else 3)
        rg.check(codec, case)

    def test_tile_row_longer_than_an_index_chunk(self, dv, codec):
        case = rc.long_row(self.BITS)[0]
        p = self.plan(dv)(*rc.LONG, 9, case[2], case[3])
        assert p["chunk_pieces"] == 2 and p["chunk_tiles"] == 512
        rg.check(codec, case)

    def test_several_segments(self, dv, codec, cus):
        """The plan cuts S > 1 segments on this device (asserted, not assumed); the reference has no segments."""
        for case in rc.segments(self.BITS) + rc.residues_all(self.BITS):
            _, spec, rw, rh, _, mask = case
            p = self.plan(dv)(spec[2], spec[3], spec[4], rw, rh, stats=mask, n_cu=cus)
            assert p["segments"] > 1 and p["workspace_bytes"] > 0
        rg.run(codec, rc.segments(self.BITS))

    def test_rejected_frames(self, dv, codec, cus):
        """Broken frames at the first, middle and last place and at the segment borders, their origin rows int32
        extremes: they add nothing and their origins_used rows keep the sentinel (rg.check).  Every frame rejected:
        the empty projection and count 0."""
        cases = rc.rejected(self.BITS)
        p = self.plan(dv)(*rc.FRAME, rc.N_ALL, *rc.WINDOW, n_cu=cus)
        if cus == 256:
            assert p["segments"] == 3 and p["frames_per_segment"] == 23
        rg.check(codec, cases[0])
        out, _ = rg.check(codec, cases[1])
        got = rg.planes(out)
        top = 255 if self.BITS == 8 else 65535
        assert int(out.count.item()) == 0 and not got["max"].any() and (got["min"] == top).all()
        assert not got["sum"].any() and not got["sumsq"].any()

    def test_clamping(self, codec):
        """Origins far outside on every side: the result and origins_used are the reference's with clamped origins."""
        rg.run(codec, rc.clamping(self.BITS))

    def test_statistics_masks_touch_only_their_planes(self, dv, codec):
        """Each statistic alone, all four and two mixed masks; the unrequested planes of out= keep their sentinel."""
        import torch
        for case in rc.masks(self.BITS):
            name, spec, rw, rh, origins, mask = case
            rg.check(codec, case)
            inst = self.plan(dv)(spec[2], spec[3], spec[4], rw, rh, stats=mask)["instance"]
            assert inst & mask == mask and inst in (3, 12, 15)
            s = lg.stream(*spec)
            full = sentinels(dv, rh, rw, self.BITS)
            before = {k: getattr(full, k).clone() for k in rr.STATS}
            names = rr.names_of(mask)
            out = dv.Projection(count=full.count, **{k: getattr(full, k) for k in names})
            self.call(codec)(s.buf, s.lead, s.total, s.offs, s.W, s.H, s.n, rw, rh, rg.device_origins(origins), out=out)
            codec.sync()
            want = rr.registered(s.images, origins, rw, rh, self.BITS)
            rg.compare(out, want, names, name)
            for k in rr.STATS:
                if k not in names:
                    assert torch.equal(getattr(full, k), before[k]), (mask, k, "an unrequested plane was written")

    def test_max_and_min_at_odd_addresses(self, dv, codec):
        """max / min planes that start at an odd element of a larger buffer (8 bits: an odd byte address)."""
        import torch
        name, spec, rw, rh, origins, mask = rc.clamping(self.BITS)[0]
        s = lg.stream(*spec)
        dt = torch.uint8 if self.BITS == 8 else torch.int16
        bufs = [torch.full((rw * rh + 2,), 0x5A, dtype=dt, device="cuda") for _ in range(2)]
        out = dv.Projection(max=bufs[0][1:1 + rw * rh].view(rh, rw), min=bufs[1][1:1 + rw * rh].view(rh, rw),
                            count=torch.zeros(1, dtype=torch.int64, device="cuda"))
        self.call(codec)(s.buf, s.lead, s.total, s.offs, s.W, s.H, s.n, rw, rh, rg.device_origins(origins), out=out)
        codec.sync()
        rg.compare(out, rr.registered(s.images, origins, rw, rh, self.BITS), ("max", "min"), "odd addresses")
        for b in bufs:
            assert b[[0, -1]].tolist() == [0x5A, 0x5A]

    @pytest.mark.parametrize("B", (1, 7, 32))
    def test_accumulating_calls_equal_one_call(self, codec, B):
        """The frames and their origin rows split into consecutive accumulating calls of B frames."""
        import torch
        for case in rc.residues_all(self.BITS) + rc.rejected(self.BITS)[:1]:
            name, spec, rw, rh, origins, mask = case
            s = lg.stream(*spec)
            one, _ = rg.check(codec, case)
            org = rg.device_origins(origins)
            used = torch.full((s.n, 2), rg.SENT, dtype=torch.int32, device="cuda")
            parts = None
            for lo in range(0, s.n, B):
                cnt = min(B, s.n - lo)
                parts, _ = self.call(codec)(s.buf, s.lead, s.total, s.offs[lo:], s.W, s.H, cnt, rw, rh, org[lo:],
                                            out=parts, accumulate=parts is not None, origins_used=used[lo:])
            codec.sync()
            for k in rr.STATS + ("count",):
                assert torch.equal(getattr(parts, k), getattr(one, k)), (name, B, k)
            want = rr.registered(s.images, origins, rw, rh, self.BITS)["used"]
            assert all(tuple(r) == want.get(f, (rg.SENT,) * 2) for f, r in enumerate(used.tolist()))

    def test_accumulate_and_empty_calls(self, dv, codec):
        """n = 0: accumulate leaves everything as it is, a plain call writes the empty projection."""
        import torch
        name, spec, rw, rh, origins, mask = rc.clamping(self.BITS)[0]
        s = lg.stream(*spec)
        out = sentinels(dv, rh, rw, self.BITS)
        before = {k: getattr(out, k).clone() for k in rr.STATS}
        org = rg.device_origins(origins)
        self.call(codec)(s.buf, s.lead, s.total, s.offs, s.W, s.H, 0, rw, rh, org, out=out, accumulate=True)
        codec.sync()
        assert all(torch.equal(getattr(out, k), before[k]) for k in rr.STATS) and int(out.count.item()) == -77
        self.call(codec)(s.buf, s.lead, s.total, s.offs, s.W, s.H, 0, rw, rh, org, out=out)
        codec.sync()
        rg.compare(out, rr.registered([], [], rw, rh, self.BITS), rr.STATS, "n = 0")

    def test_against_the_library_itself(self, codec):
        """The planes equal torch reductions over decode_roi(origins=...)'s windows; all-equal origins equal project."""
        import torch
        name, spec, rw, rh, origins, mask = rc.residues_all(self.BITS)[0]
        s = lg.stream(*spec)
        org = rg.device_origins(origins)
        roi = codec.decode_roi if self.BITS == 8 else codec.decode_roi16
        proj = codec.project if self.BITS == 8 else codec.project16
        wins, _ = roi(s.buf, s.lead, s.total, s.offs, s.W, s.H, s.n, 0, 0, rw, rh, origins=org)
        out, _ = self.call(codec)(s.buf, s.lead, s.total, s.offs, s.W, s.H, s.n, rw, rh, org)
        codec.sync()
        v = wins.to(torch.int64) & (255 if self.BITS == 8 else 65535)
        mm = lambda t: t.to(torch.int64) & (255 if self.BITS == 8 else 65535)   # noqa: E731
        assert torch.equal(mm(out.max), v.amax(0)) and torch.equal(mm(out.min), v.amin(0))
        assert torch.equal(out.sum, v.sum(0)) and torch.equal(out.sumsq, (v * v).sum(0))
        same = torch.tensor([[13, 7]] * s.n, dtype=torch.int32, device="cuda")
        a, _ = self.call(codec)(s.buf, s.lead, s.total, s.offs, s.W, s.H, s.n, rw, rh, same)
        b, _ = proj(s.buf, s.lead, s.total, s.offs, s.W, s.H, s.n, 13, 7, rw, rh)
        codec.sync()
        for k in rr.STATS + ("count",):
            assert torch.equal(getattr(a, k), getattr(b, k)), k

    def test_python_forms_and_argument_errors(self, dv, codec):
        import torch
        name, spec, rw, rh, origins, mask = rc.clamping(self.BITS)[0]
        s = lg.stream(*spec)
        W, H, n = s.W, s.H, s.n
        call, args = self.call(codec), (s.buf, s.lead, s.total, s.offs, W, H, n, rw, rh)
        org = rg.device_origins(origins)
        a, _ = call(*args, org, stats="sum")
        codec.sync()
        assert a.max is None and a.sumsq is None
        assert np.array_equal(rg.planes(a)["sum"], rr.registered(s.images, origins, rw, rh, self.BITS)["sum"])
        wide = torch.zeros((n, 3), dtype=torch.int32, device="cuda")
        for bad in (org.to(torch.int64), org.cpu(), org[:n - 1], wide, wide[:, :2], org.reshape(-1), None):
            with pytest.raises(ValueError):
                call(*args, bad)
        with pytest.raises(ValueError):
            call(*args, org, origins_used=org.to(torch.int64))
        with pytest.raises(ValueError):
            call(*args, org, accumulate=True)                       # nothing to continue
        with pytest.raises(ValueError):
            call(*args, org, stats=("median",))
        # the C call: NULL and misaligned pointers, sizes
        L, h = codec.L, codec.h
        fn = L.dbde_hip_project_registered if self.BITS == 8 else L.dbde16_hip_project_registered
        buf = torch.zeros(H * W + 2, dtype=torch.int64, device="cuda")
        p, o = buf.data_ptr(), org.data_ptr()

        def rc_(planes=(p, p, p, p), count=p, origins=o, n=n, rw=rw, rh=rh):
            return fn(h, s.buf.data_ptr() + s.lead, s.total, s.offs.data_ptr(), W, H, n, rw, rh, origins, 0, *planes,
                      count, None, None)
        assert rc_() == dv.OK and rc_(planes=(None, None, p, None)) == dv.OK and rc_(rw=W, rh=H) == dv.OK
        for kw in (dict(origins=None), dict(planes=(None,) * 4), dict(count=None), dict(count=p + 4),
                   dict(planes=(None, None, p + 4, None)), dict(planes=(None, None, None, p + 4)), dict(n=-1),
                   dict(rw=0), dict(rw=W + 1), dict(rh=0), dict(rh=H + 1)):
            assert rc_(**kw) == dv.ERR_ARG, kw
        assert rc_(planes=(p + 1, None, None, None)) == (dv.OK if self.BITS == 8 else dv.ERR_ARG)
        codec.sync()


class TestRegistered(Registered):
    BITS = 8
