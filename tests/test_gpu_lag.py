"""GPU: lag projections -- dbde_hip_project_lag (Codec.project_lag).

Every plane and both scalars are compared for equality with tests/lag_ref.py -- the definition in numpy over decoded
images -- on streams crafted on the host (tests/lag_cases.py lists the cases; tests/test_lag_ref.py holds the cap on
each of them before any GPU run).  Nothing expected comes from the call itself.  The bodies live in the `Lag` class so
that tests/test_gpu_lag16.py runs the same ones at 16 bits.
"""
import numpy as np
import pytest

import far
import lag_cases as lc
import lag_gpu as lg
import lag_ref as lr
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


def sentinels(dv, rh, rw, bits, lag, value=-77):
    """A LagProjection whose five planes and two scalars hold a sentinel."""
    import torch
    out = dv.LagProjection.empty(lr.STATS, rh, rw, "cuda", lag=lag, bits=bits)
    for k in lr.STATS:
        getattr(out, k).fill_(value if k != "maxdiff" or bits == 16 else 0xB3)
    out.pairs.fill_(value)
    out.count.fill_(value)
    return out


class Lag:
    """The cases at one pixel size (BITS)."""
    BITS = 8

    def call(self, codec):
        return codec.project_lag if self.BITS == 8 else codec.project_lag16

    def plan(self, dv):
        return dv.lag_plan if self.BITS == 8 else dv.lag16_plan

    @pytest.mark.parametrize("lag", lg.LAGS)
    def test_every_lag_window_and_count(self, dv, codec, lag):
        lc.run(codec, lc.sweep(self.BITS, lag), self.BITS, "sweep")
        p = self.plan(dv)(*lg.FRAME, 13, lag=lag)
        assert p["segments"] == 1 and p["pieces_x"] == (1 if self.BITS == 8 else 2)

    def test_two_pieces_across(self, dv, codec):
        lc.run(codec, lc.wide(self.BITS), self.BITS, "wide")
        assert self.plan(dv)(*lg.WIDE, 13)["pieces_x"] == (2 if self.BITS == 8 else 3)

    def test_segments_decode_their_history(self, dv, codec, cus):
        """The plan cuts S > 1 segments on this device (asserted, not assumed); the reference has no segments."""
        cases = lc.segments(self.BITS)
        for spec, n, lag, win, lead, mask, _ in cases:
            p = self.plan(dv)(*lg.FRAME, n, *win, lag=lag, lead=lead, stats=mask, n_cu=cus)
            assert p["segments"] > 1 and p["history_frames"] == (p["segments"] - 1) * lag
        lc.run(codec, cases, self.BITS, "segments")

    @pytest.mark.parametrize("lag", (1, 3, 8))
    def test_rejected_frames_void_their_pairs(self, dv, codec, cus, lag):
        cases = lc.rejected(self.BITS, lag)
        p = self.plan(dv)(*lg.FRAME, 33, lag=lag, n_cu=cus)
        if cus == 256:
            assert p["segments"] == 2 and p["frames_per_segment"] == lc.FPS33
        lc.run(codec, cases, self.BITS, "rejected")
        s = lg.stream(*cases[-3][0])          # every frame rejected
        assert all(im is None for im in s.images)
        out, _ = lg.check(codec, s, lag, lg.SMALL, bits=self.BITS)
        assert int(out.pairs.item()) == 0 and int(out.count.item()) == 0 and not lg.planes(out)["sqdiff"].any()

    def test_lead(self, codec):
        lc.run(codec, lc.leads(self.BITS), self.BITS, "lead")

    def test_statistics_masks_touch_only_their_planes(self, dv, codec):
        """Each statistic alone, all five and two mixed masks; the unrequested planes of out= keep their sentinel."""
        import torch
        lc.run(codec, lc.masks(self.BITS), self.BITS, "masks")
        for spec, n, lag, win, lead, mask, _ in lc.masks(self.BITS):
            s = lg.stream(*spec).first(n)
            inst = self.plan(dv)(s.W, s.H, n, *win, lag=lag, stats=mask)["instance"]
            assert inst & mask == mask and inst in (3, 28, 31)
            out = sentinels(dv, win[3], win[2], self.BITS, lag)
            before = {k: getattr(out, k).clone() for k in lr.STATS}
            names = lr.names_of(mask)
            got, _ = self.call(codec)(s.buf, s.lead, s.total, s.offs, s.W, s.H, n, lag, names, lead, *win, out=out)
            codec.sync()
            assert got is out
            want = lr.lag(s.images, lag, *win, lead=lead, bits=self.BITS)
            for k in lr.STATS:
                if k in names:
                    assert np.array_equal(lg.planes(out)[k], want[k]), (mask, k)
                else:
                    assert torch.equal(getattr(out, k), before[k]), (mask, k, "an unrequested plane was written")
            assert int(out.pairs.item()) == want["pairs"] and int(out.count.item()) == want["count"]

    @pytest.mark.parametrize("lag,B", [(1, 1), (1, 7), (3, 3), (3, 7), (3, 32), (7, 7), (8, 8), (8, 32)])
    def test_split_rule(self, dv, codec, cus, lag, B):
        """One call equals the accumulating calls of the header's split rule bit for bit, maxdiff and both scalars
        included; some of the calls run several segments."""
        import torch
        for spec, n, _, win, _, _, _ in lc.splits(self.BITS, lag):
            s = lg.stream(*spec)
            one, _ = lg.check(codec, s, lag, win, bits=self.BITS, what="one call")
            parts = lg.split_on_device(codec, s, lag, win, B, bits=self.BITS)
            for k in lr.STATS + ("pairs", "count"):
                assert torch.equal(getattr(parts, k), getattr(one, k)), (lag, B, win, k)
            assert int(parts.count.item()) == 63

    def test_accumulate_without_a_pair_changes_nothing(self, dv, codec):
        """accumulate=1 with no counted pair (n <= lag, lead = n, every frame rejected) leaves sentinel-filled planes
        and pairs as they are and adds the accepted frames past the lead to count; accumulate=0 writes zeros."""
        import torch
        s = lg.stream(*lc.noise(self.BITS, 13))
        gone = lg.stream(*lc.crafted(self.BITS, 13, bad=tuple(range(13))))
        win, lag = lg.SMALL, 4
        for st, n, lead, count in ((s, 4, 0, 4), (s, 13, 13, 0), (s, 2, 1, 1), (gone, 13, 0, 0), (s, 0, 0, 0)):
            out = sentinels(dv, win[3], win[2], self.BITS, lag)
            before = {k: getattr(out, k).clone() for k in lr.STATS}
            self.call(codec)(st.buf, st.lead, st.total, st.offs, st.W, st.H, n, lag, lr.STATS, lead, *win, out=out,
                             accumulate=True)
            codec.sync()
            for k in lr.STATS:
                assert torch.equal(getattr(out, k), before[k]), (n, lead, k)
            assert int(out.pairs.item()) == -77 and int(out.count.item()) == -77 + count
            self.call(codec)(st.buf, st.lead, st.total, st.offs, st.W, st.H, n, lag, lr.STATS, lead, *win, out=out)
            codec.sync()
            assert all(not getattr(out, k).any() for k in lr.STATS) and int(out.pairs.item()) == 0
            assert int(out.count.item()) == count

    def test_outputs_at_odd_offsets_in_guarded_buffers(self, dv, codec, cus):
        """Every plane starts at an odd element of a far.guarded buffer (one and several segments); nothing outside the
        planes is written; the scalars sit between sentinels."""
        import torch
        full = lg.stream(*lc.noise(self.BITS, 70))
        win, lag = lg.SMALL, 3
        rh, rw = win[3], win[2]
        mx = torch.uint8 if self.BITS == 8 else torch.int16
        for n in (13, 70):
            s = full.first(n)
            assert (self.plan(dv)(s.W, s.H, n, *win, lag=lag, n_cu=cus)["segments"] > 1) == (n == 70)
            gs = {k: far.guarded((rh * rw + 2,), torch.int64 if k != "maxdiff" else mx) for k in lr.STATS}
            scal = torch.full((5,), -7, dtype=torch.int64, device="cuda")
            out = dv.LagProjection(pairs=scal[1:2], count=scal[3:4], lag=lag,
                                   **{k: g.t[1:1 + rh * rw].view(rh, rw) for k, g in gs.items()})
            self.call(codec)(s.buf, s.lead, s.total, s.offs, s.W, s.H, n, lag, lr.STATS, 0, *win, out=out)
            codec.sync()
            want = lg.cap(s.images, lag, win, 0, self.BITS)
            lg.compare(out, want, lr.STATS, f"guarded n={n}")
            for k, g in gs.items():
                g.check(f"{k} n={n}")
                edge = g.t[[0, -1]].cpu().numpy().view(np.uint8)
                assert (edge == far.SENTINEL).all(), (k, "an element next to the plane was written")
            assert scal.tolist() == [-7, want["pairs"], -7, want["count"], -7]
            del gs, out
        far.free()

    def test_extreme_products_and_differences(self, codec):
        """Constant 0 and constant 255 / 65,535 alternating.  At 16 bits and n = 70 the largest per-lane sums are
        35 * 65,535^2 (product, sqdiff) and 69 * 65,535 (pairsum): a U32 pairsum or absdiff accumulator would have to
        wrap to show, which takes more than 32,768 pairs of a segment: the accumulator widths (DBDE16: U64 for
        product, sqdiff and pairsum, 65,536 * 131,070 = 2^33) are tested by tests/test_gpu_bounds.py, whose segments
        count 65,536 pairs."""
        lc.run(codec, lc.extremes(self.BITS), self.BITS, "extremes")

    def test_python_forms_and_argument_errors(self, dv, codec):
        import torch
        s = lg.stream(*lc.noise(self.BITS, 13))
        W, H = s.W, s.H
        call, args = self.call(codec), (s.buf, s.lead, s.total, s.offs, s.W, s.H, s.n)
        a, _ = call(*args)                                          # lag 1, sqdiff alone
        b, _ = call(*args, 1, "sqdiff")
        codec.sync()
        assert a.stats == ("sqdiff",) and a.lag == 1 and torch.equal(a.sqdiff, b.sqdiff) and a.product is None
        assert np.array_equal(lg.planes(a)["sqdiff"], lr.lag(s.images, 1, 0, 0, W, H, bits=self.BITS)["sqdiff"])
        for bad in ((), ("sum",), 0, 32):
            with pytest.raises(ValueError):
                call(*args, 1, bad)
        with pytest.raises(ValueError):
            call(*args, 1, accumulate=True)                         # nothing to continue
        with pytest.raises(ValueError):
            call(*args, 2, out=a)                                   # another lag than out holds
        with pytest.raises(ValueError):
            call(*args, 1, ("product",), out=a)                     # out has no such plane
        with pytest.raises(ValueError):
            call(*args, 1, x=1, out=a)                              # another window
        for lag, lead in ((0, 0), (9, 0), (-1, 0), (1, -1), (1, 14)):
            with pytest.raises(dv.DbdeError):
                call(*args, lag, ("sqdiff",), lead)
        # the C call: NULL and misaligned pointers
        L, h = codec.L, codec.h
        fn = L.dbde_hip_project_lag if self.BITS == 8 else L.dbde16_hip_project_lag
        buf = torch.zeros(H * W + 2, dtype=torch.int64, device="cuda")
        sc = torch.zeros(4, dtype=torch.int64, device="cuda")

        def rc(planes=(buf.data_ptr(),) * 5, pairs=sc.data_ptr(), count=sc.data_ptr() + 8, n=13, lag=1, lead=0, rw=W):
            return fn(h, s.buf.data_ptr() + s.lead, s.total, s.offs.data_ptr(), W, H, n, 0, 0, rw, H, lag, lead, 0,
                      *planes, pairs, count, None)
        assert rc() == dv.OK
        p = buf.data_ptr()
        assert rc(planes=(None, None, None, None, p)) == dv.OK and rc(planes=(None, None, p, None, None)) == dv.OK
        for kw in (dict(planes=(None,) * 5), dict(pairs=None), dict(count=None), dict(pairs=sc.data_ptr() + 4),
                   dict(count=sc.data_ptr() + 4), dict(planes=(p + 4, None, None, None, None)),
                   dict(planes=(None, None, None, p + 2, None)), dict(lag=0), dict(lag=9), dict(lead=-1), dict(lead=14),
                   dict(n=-1), dict(rw=W + 1), dict(rw=0)):
            assert rc(**kw) == dv.ERR_ARG, kw
        assert rc(planes=(None, None, None, None, p + 1)) == (dv.OK if self.BITS == 8 else dv.ERR_ARG)
        for at in (1, 3):     # the stream, the offsets
            a_ = [h, s.buf.data_ptr() + s.lead, s.total, s.offs.data_ptr(), W, H, 13, 0, 0, W, H, 1, 0, 0, p, p, p, p, p,
                  sc.data_ptr(), sc.data_ptr() + 8, None]
            a_[at] = None
            assert fn(*a_) == dv.ERR_ARG, at
        codec.sync()


class TestLag(Lag):
    BITS = 8
