"""CPU: the reference of the registered projections (tests/registered_ref.py) against a brute-force per-pixel loop, and
the cap of every case of tests/registered_cases.py before any GPU run: no case passes with the origins ignored,
transposed or off by one (registered_gpu.cap)."""
import numpy as np
import pytest

import registered_cases as rc
import registered_gpu as rg
import registered_ref as rr


@pytest.mark.parametrize("bits", (8, 16))
def test_reference_equals_the_per_pixel_loop(bits):
    for name, spec, rw, rh, origins, mask in rc.clamping(bits) + rc.rejected(bits)[1:] + rc.windows(bits)[1:3]:
        images = rg.images_of(spec)
        _, _, W, H, n, _, _ = spec
        if rw * rh * n > 41 * 27 * 13:
            continue
        want = rr.brute(images, origins, rw, rh, W, H, bits)
        got = rr.registered(images, origins, rw, rh, bits)
        for k in rr.STATS:
            assert got[k].tolist() == want[k], (name, k)
        assert got["count"] == sum(im is not None for im in images)


def test_reference_clamps_and_skips_rejected_frames():
    im = np.arange(6 * 5, dtype=np.uint8).reshape(5, 6)
    got = rr.registered([im, None, im], [(rr.I32_MAX, rr.I32_MIN), (0, 0), (-3, 9)], 2, 2)
    assert got["used"] == {0: (4, 0), 2: (0, 3)} and got["count"] == 2
    assert got["max"].tolist() == [[18, 19], [24, 25]] and got["min"].tolist() == [[4, 5], [10, 11]]
    assert got["sum"].tolist() == [[22, 24], [34, 36]] and got["sumsq"][0, 0] == 4 * 4 + 18 * 18
    none = rr.registered([None], [(0, 0)], 2, 3, bits=16)
    assert none["count"] == 0 and not none["max"].any() and (none["min"] == 65535).all() and none["min"].shape == (3, 2)


@pytest.mark.parametrize("bits", (8, 16))
def test_every_case_meets_its_cap(bits):
    for name, spec, rw, rh, origins, mask in rc.every(bits):
        images = rg.images_of(spec)
        assert len(images) == len(origins) == spec[4], name
        rg.cap(images, spec, rw, rh, origins, mask)


@pytest.mark.parametrize("bits", (8, 16))
def test_cases_cover_what_they_claim(bits):
    seen = {(int(x) & 7, int(y) & 7) for x, y in rc.all_origins()[:64]}
    assert len(seen) == 64
    assert {(int(o[0][0]) & 7, int(o[0][1]) & 7) for _, _, _, _, o, _ in rc.residues_each(bits)} == seen
    for _, _, _, _, o, _ in rc.residues_each(bits):
        assert len({(int(x) & 7, int(y) & 7) for x, y in o}) == 1 and len({tuple(r) for r in o.tolist()}) == 3
    # the long row: the last piece's first source tile lies on both sides of tile 512, and a band spans two tile rows
    cols = 248 if bits == 8 else 120
    _, spec, rw, rh, o, _ = rc.long_row(bits)[0]
    last = (rw - 1) // cols * cols
    firsts = {(int(x) + last) >> 3 for x, _ in o}
    assert min(firsts) < 512 <= max(firsts) and any(int(y) & 7 for _, y in o) and spec[2] > 512 * 8
    # more than one piece across, and a shift that moves a column from one source tile to the next
    _, spec, rw, rh, o, _ = rc.wide(bits)[0]
    assert rw > cols and len({(int(x) + cols) >> 3 for x, _ in o}) > 1
    # the far corner: a last band of fewer than 8 rows against the frame's last (partial) tile row
    for (_, spec, rw, rh, o, _), H in zip(rc.windows(bits)[2:], (45, 48)):
        assert spec[3] == H and rh % 8 and rw % 8 and (spec[2] - rw, H - rh) in {tuple(r) for r in o.tolist()}
