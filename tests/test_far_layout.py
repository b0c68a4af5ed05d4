"""CPU: the layout that tests/test_gpu_far_offsets.py relies on (tests/far.py), for every geometry and straddle kind it
places.  A far frame's offset that loses its high half lands on that frame's decoy, inside the allocation, never on a
real frame; no two frames or decoys overlap; each straddle holds the byte it claims to."""
import numpy as np
import pytest

import crafted as cr
import far
from test_oracle_u16 import o16, pack16   # noqa: F401  (fixture + helper)

CASES = [(W, H, 8) for W, H in far.GEOMETRIES8] + [(W, H, 16) for W, H in far.GEOMETRIES16]


@pytest.fixture(scope="module")
def sets(oracle, o16):   # noqa: F811
    cache = {}

    def get(W, H, bits):
        if (W, H, bits) not in cache:
            cache[(W, H, bits)] = far.frame_set(W, H, bits, oracle, lambda img, i: pack16(o16, img, i))
        return cache[(W, H, bits)]
    return get


@pytest.mark.parametrize("W,H,bits", CASES, ids=[f"{w}x{h}-{b}" for w, h, b in CASES])
@pytest.mark.parametrize("straddle", far.STRADDLES)
def test_far_layout(sets, W, H, bits, straddle):
    good, bad, decoys = sets(W, H, bits)
    lay = far.far_layout(good, bad, decoys, straddle)
    lay.check()
    x = lay.offsets
    sizes = [len(f) for f in lay.frames]
    # the slots are what they say
    assert x[0] + sizes[0] < far.G31 and far.G31 - x[0] - sizes[0] <= 64
    assert x[1] + 20 <= far.G31 < x[1] + 24, "frame 1: header below 2^31, depth bytes above"
    assert x[2] > far.G31 and x[2] % 2 == 1 and x[2] + sizes[2] < far.G32
    assert x[3] < far.G32 < x[3] + sizes[3]
    assert x[4] > far.G32 and x[4] % 2 == 1
    assert lay.stream_bytes == x[5] + sizes[5] and x[5] + sizes[5] < far.G32 + far.G31
    st = far.straddles(lay)
    a, b = far.parts(lay.frames[3])[straddle]
    assert f"{straddle}@2^32" in st[3] and x[3] + a <= far.G32 < x[3] + b
    if b - a > 1:
        assert x[3] + a <= far.G32 - 1 and far.G32 <= x[3] + b - 1, f"{straddle}: bytes on both sides of 2^32"
    assert "T@2^31" in st[1]
    # the aliases of every far frame: its decoy, a valid frame of this geometry that is not the frame
    T, mb = cr.tiles(W, H), bits // 8
    for x_d, dec, k in lay.decoys:
        assert x_d == x[k] - far.G32
        assert not cr.broken_rules(dec[20:], W, H, bits)
        assert int(dec[24:24 + T].astype(np.int64).sum()) * 8 + 32 + T + mb * T == len(dec)
    assert {k for _, _, k in lay.decoys} == {1, 2, 3, 4, 5}
    for k in (2, 3, 4, 5):
        assert far.aliases(x[k]) == [x[k] - far.G32]
    # frames past 2^31 are more than the frame they alias: the valid ones decode, the broken ones break a rule
    assert cr.broken_rules(lay.frames[2][20:], W, H, bits) and cr.broken_rules(lay.frames[4][20:], W, H, bits)
    for k in (0, 1, 3, 5):
        assert not cr.broken_rules(lay.frames[k][20:], W, H, bits), k


def test_aliases():
    G31, G32 = far.G31, far.G32
    assert far.aliases(5) == [] and far.aliases(G31 - 1) == []
    assert far.aliases(G31) == [-G31] and far.aliases(G32 - 1) == [-1]
    assert far.aliases(G32) == [0] and far.aliases(G32 + 7) == [7]
    assert far.aliases(G32 + G31) == [-G31, G31]


def test_leads_hold_every_alias():
    # a sign-extended 32-bit byte offset reaches 2^31 in front of P, a U16 element index 2^32; both keep the margin
    assert far.LEAD8 % 256 == 0 and far.LEAD8 >= far.G31 + far.MARGIN
    assert far.LEAD16 % 256 == 0 and far.LEAD16 >= 2 * far.G31 + far.MARGIN
