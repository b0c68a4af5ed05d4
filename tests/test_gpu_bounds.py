"""GPU: the segment projections with 65,536 frames in one workgroup -- the per-lane U32 accumulators of project,
project_registered, project_pairs, project_lag and project_groups at the bound their header comments compute
(65,536 * 255^2, 65,536 * 65,535), which no other test comes near: everywhere else the plan cuts a batch into segments of
a few dozen frames.

tests/bound_cases.py has the method: a stream of four palette frames, an offsets tensor of 65,536 or 131,072 entries
pointing into it, and a frame one tile across and 4 * n_cu tile rows high, at which the plan stops cutting (asserted
here on the device's own compute-unit count: frames_per_segment == max_frames_per_segment == 65,536).  Every element of
every output is compared with the counting reference, which tests/test_bound_cases.py checks against the brute-force
references, the bounds and six wrong kernels on the CPU.

Per family and bit depth: 65,536 frames in one segment (the lane's accumulator goes straight into the U64 output); the
same call once more with accumulate (the prior value added to an accumulator beyond 2^31; everything doubles); 131,072
frames in two full segments (U32 partials at the bound through the workspace and the combine kernel, sums beyond 2^32;
lag's second segment decodes its history and counts exactly 65,536 pairs), and that call accumulated too.  Lag runs at
lag 1 over the alternation and at lag 2 over the mixed order, all five statistics.  Grouped projections run a 16 x 64
frame: uniform groups of 65,536 over 131,072 frames, one ragged group [0, 65,536), each accumulated too (the U32 sums
then wrap modulo 2^32, as the header says), the U32 sums read through GroupProjection.sums().

One context and one upload of each palette serve the module; its case count and wall time are printed at teardown.
"""
import time

import numpy as np
import pytest

import bound_cases as bc
import lag_gpu as lg
import pairs_gpu as pg
import wproject_gpu as wg

pytestmark = pytest.mark.gpu

CASES = [(f, b, c, t) for f in bc.FAMILIES for b in bc.BITS for c in bc.cases(f) for t in (1, 2)]
IDS = [f"{f}{b}-{c[0]}" + ("-accumulate" if t == 2 else "") for f, b, c, t in CASES]
T0, SPENT = [None], {}


@pytest.fixture(scope="module")
def dv():
    import dbde_video_cpp_amd as m
    return m


@pytest.fixture(scope="module")
def codec(dv):
    T0[0] = time.time()
    c = dv.Codec(0)
    assert c.arch.startswith("gfx950")
    yield c
    c.close()
    slow = max(SPENT, key=SPENT.get) if SPENT else None
    print(f"\ntest_gpu_bounds: {len(CASES)} cases in {time.time() - T0[0]:.1f} s"
          + (f"; slowest {slow} {SPENT[slow]:.2f} s" if slow else ""))


@pytest.fixture(scope="module")
def cus(codec):
    return wg.cus_of(codec)


@pytest.fixture(scope="module")
def palettes(codec, cus):
    """(family, bits) -> (bound_cases.Setup at the device's compute-unit count, its stream on the device, the slots'
    offsets), built and uploaded once."""
    import torch
    cache = {}

    def get(family, bits):
        if (family, bits) not in cache:
            s = bc.Setup(family, bits, n_cu=cus)
            buf, lead, offs, total = s.stream()
            cache[family, bits] = (s, wg.Stream(torch.from_numpy(buf).cuda(), lead, total, None, s.W, s.H, []), offs)
        return cache[family, bits]
    return get


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not np.array_equal(got, want):
        bad = tuple(np.argwhere(got != want)[0])
        raise AssertionError(f"{what}: differs at {bad}: {got[bad]} != {want[bad]}; {int((got != want).sum())} of "
                             f"{got.size} elements")


def pixels(t, bits):
    """A max / min / maxdiff tensor on the host in the pixel type (int16 tensors hold the U16 bits)."""
    a = t.cpu().numpy()
    return a if bits == 8 else a.view(np.uint16)


def plan_of(dv, family, bits, s, n, lag, cus):
    sfx = "" if bits == 8 else "16"
    if family == "project":
        return getattr(dv, f"project{sfx}_plan")(s.W, s.H, n, n_cu=cus)
    if family == "registered":
        return getattr(dv, f"registered{sfx}_plan")(s.W, s.H, n, s.rw, s.rh, n_cu=cus)
    if family == "pairs":
        return getattr(dv, f"pairs{sfx}_plan")(s.W, s.H, n, pairs=15, n_cu=cus)
    return getattr(dv, f"lag{sfx}_plan")(s.W, s.H, n, lag=lag, stats=31, n_cu=cus)


@pytest.mark.parametrize("family,bits,case,times", CASES, ids=IDS)
def test_accumulators_at_the_bound(dv, codec, cus, palettes, family, bits, case, times):
    import torch
    t0 = time.time()
    name, n, order, lag = case
    s, st, slot_offs = palettes(family, bits)
    slots = bc.order(order, n)
    offs = torch.from_numpy(slot_offs[slots]).cuda()
    rows = torch.from_numpy(s.result_rows(slots))
    sfx = "" if bits == 8 else "16"
    what = f"{family}{sfx} {name} x{times} ({s.W}x{s.H}, n={n}, {cus} CUs)"
    pix = np.uint8 if bits == 8 else np.uint16
    args = (st.buf, st.lead, st.total, offs, s.W, s.H, n)

    if family == "groups":
        p = getattr(dv, f"project_groups{sfx}_plan")(s.W, s.H, n, n_cu=cus, **(
            dict(group_frames=bc.N_SEG) if name == "uniform" else dict(has_group_starts=True, n_groups=1)))
        assert p["max_group_frames"] == bc.N_SEG and p["runs"] * p["groups_per_run"] == n // bc.N_SEG, p
        print(f"\n{what}: runs = {p['runs']}, groups per run = {p['groups_per_run']}")
        kw = dict(group_frames=bc.N_SEG) if name == "uniform" else dict(group_starts=[0, bc.N_SEG])
        call = getattr(codec, f"project_groups{sfx}")
        out, res = call(*args, **kw)
        for _ in range(times - 1):
            out, res = call(*args, accumulate=True, out=out, **kw)
        codec.sync()
        want = bc.expected_groups(s, slots, bc.ranges_of(family, case), times)
        assert out.sum.dtype == torch.int32 and out.sumsq.dtype == torch.int64
        same(out.sums().cpu().numpy(), want["sum"], what + " sum")
        same(out.sumsq.cpu().numpy(), want["sumsq"], what + " sumsq")
        same(pixels(out.max, bits), want["max"].astype(pix), what + " max")
        same(pixels(out.min, bits), want["min"].astype(pix), what + " min")
        same(out.counts.cpu().numpy().view(np.uint32).astype(np.int64), want["counts"], what + " counts")
        if bits == 16 and times == 1:      # a U32 plane beyond 2^31 shows negative in the int32 tensor: sums() must not
            assert int(out.sum.min().item()) < 0 and int(out.sums().max().item()) == bc.bound(16, "sum")
    else:
        p = plan_of(dv, family, bits, s, n, lag, cus)
        assert p["frames_per_segment"] == p["max_frames_per_segment"] == bc.N_SEG and p["segments"] == n // bc.N_SEG, p
        want = bc.expected(s, slots, n, lag=lag, times=times)
        if family in ("project", "registered"):
            if family == "registered":
                org = torch.from_numpy(bc.origins_of(slots)).cuda()
                used = torch.full((n, 2), -1, dtype=torch.int32, device="cuda")
                reg = getattr(codec, f"project_registered{sfx}")
                call = lambda **kw: reg(*args, s.rw, s.rh, org, origins_used=used, **kw)  # noqa: E731
            else:
                call = lambda **kw: getattr(codec, f"project{sfx}")(*args, **kw)  # noqa: E731
            out, res = call()
            for _ in range(times - 1):
                out, res = call(out=out, accumulate=True)
            codec.sync()
            for k in ("sum", "sumsq"):
                assert getattr(out, k).dtype == torch.int64
                same(getattr(out, k).cpu().numpy(), want[k], f"{what} {k}")
            for k in ("max", "min"):
                same(pixels(getattr(out, k), bits), want[k].astype(pix), f"{what} {k}")
            if family == "registered":
                assert torch.equal(used, org), what + " origins_used"
        elif family == "pairs":
            call = getattr(codec, f"project_pairs{sfx}")
            out, res = call(*args, 15)
            for _ in range(times - 1):
                out, res = call(*args, 15, out=out, accumulate=True)
            codec.sync()
            assert tuple(out.offsets) == bc.PAIR_OFFSETS
            same(pg.planes(out), want["product"].astype(np.uint64), what + " product")
        else:
            call = getattr(codec, f"project_lag{sfx}")
            out, res = call(*args, lag, bc.LAG_SUMS + ("maxdiff",))
            for _ in range(times - 1):
                out, res = call(*args, lag, bc.LAG_SUMS + ("maxdiff",), out=out, accumulate=True)
            codec.sync()
            ref = {k: want[k].astype(np.uint64) for k in bc.LAG_SUMS}
            ref.update(maxdiff=want["maxdiff"].astype(pix), pairs=want["pairs"], count=want["count"])
            lg.compare(out, ref, bc.LAG_SUMS + ("maxdiff",), what)
            assert want["pairs"] == times * (n - lag)
        assert int(out.count.item()) == want["count"] == times * n, what + " count"
    assert dv.accepted_frames(res).all() and torch.equal(res.cpu(), rows), what + " results"
    SPENT[what] = time.time() - t0
