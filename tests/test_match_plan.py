"""CPU: dbde_hip_match_plan / dbde16_hip_match_plan (host arithmetic) on hand-derived cases; no device.

The search patch of a tw x th template at radius S is (tw + 2S) x (th + 2S); its tiles, the tile rows a wave takes and
the index geometry are the patch decoder's for that size (patches_plan).  What the match adds: up to four decoding
waves, the row slices (the count r up to min(th, 16) with the least ceil(D * D * r / 256) * (ceil(th / r) * b + 3): a
lane's passes over the (shift, slice) items times an item's cost, its rows of b batches of four dwords each plus a fixed
part of about three batches; the smallest on a tie) and the LDS, sized per launch: the band of 8 * max_tiles_y rows at an odd pitch of (2 * pix * max_tiles_x) | 1 dwords plus
16 bytes, the template with rows padded to dwords, and the larger of the decoding waves' payload ranges and the
24 * D * D bytes of accumulators (only where a shift is split), each rounded up to 16 bytes.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@pytest.fixture(scope="module")
def dv():
    import dbde_video_cpp_amd as m
    if not os.path.exists(m.LIB_PATH):
        m.build()
    return m


def r16(v):
    return (v + 15) // 16 * 16


def slices_for(D, th, tw, pix):
    batches = -(-((tw * pix + 3) // 4) // 4)        # batches of four dwords in a template row
    cost = {r: -(-D * D * r // 256) * (-(-th // r) * batches + 3) for r in range(1, min(th, 16) + 1)}
    return min(cost, key=lambda r: (cost[r], r))


def lds_for(pix, tw, th, S, mtx, mty, G, dwaves, slices):
    D = 2 * S + 1
    band = r16(8 * mty * ((2 * mtx * pix) | 1) * 4 + 16)
    tmpl = r16(th * ((tw * pix + 3) // 4) * 4)
    pay = dwaves * r16(G * (64 * pix * mtx + 32))
    acc = 24 * D * D if slices > 1 else 0
    return band + tmpl + max(pay, acc)


# (W, H, n, tw, th, S, K, edge) -> pw, ph, D, max_tiles_x, max_tiles_y, rows_per_wave, decode_waves, steps
CASES = [
    ((4096, 3072, 10, 32, 32, 8, 64, "clamp"), (48, 48, 17, 7, 7, 9, 1, 1)),
    ((4096, 3072, 10, 64, 64, 16, 16, "clamp"), (96, 96, 33, 13, 13, 4, 4, 1)),
    ((4096, 3072, 10, 128, 128, 16, 64, "fill"), (160, 160, 33, 21, 21, 3, 4, 2)),
    ((4096, 3072, 10, 1, 1, 0, 1, "fill"), (1, 1, 1, 1, 1, 64, 1, 1)),
    ((4096, 3072, 10, 9, 1, 1, 3, "clamp"), (11, 3, 3, 3, 2, 21, 1, 1)),
    ((4096, 3072, 10, 7, 7, 1, 3, "clamp"), (9, 9, 3, 2, 2, 32, 1, 1)),
    ((72, 56, 3, 33, 31, 2, 5, "clamp"), (37, 35, 5, 6, 6, 10, 1, 1)),
    ((48, 48, 3, 32, 32, 8, 2, "clamp"), (48, 48, 17, 6, 6, 10, 1, 1)),              # the search patch is the frame
    ((10, 10, 3, 128, 128, 16, 2, "fill"), (160, 160, 33, 21, 21, 3, 4, 2)),         # larger than the frame: fill only
]


@pytest.mark.parametrize("args,want", CASES)
def test_hand_derived_plans(dv, args, want):
    W, H, n, tw, th, S, K, edge = args
    for pix, fn, pfn in ((1, dv.match_plan, dv.patches_plan), (2, dv.match16_plan, dv.patches16_plan)):
        pl = fn(W, H, n, tw, th, S, K, edge=edge)
        got = (pl["pw"], pl["ph"], pl["D"], pl["max_tiles_x"], pl["max_tiles_y"], pl["rows_per_wave"], pl["decode_waves"],
               pl["steps_per_patch"])
        assert got == want, (args, got)
        assert pl["row_slices"] == slices_for(pl["D"], th, tw, pix)
        assert pl["threads"] == 256
        assert pl["grid"] == n * K
        assert pl["surface_bytes"] == n * K * pl["D"] ** 2 * 8
        dec = pfn(W, H, n, pl["pw"], pl["ph"], K, edge)   # the patch decoder's plan of the search patch
        assert (pl["max_tiles_x"], pl["max_tiles_y"], pl["rows_per_wave"]) == \
            (dec["max_tiles_x"], dec["max_tiles_y"], dec["rows_per_workgroup"])
        assert pl["decode_waves"] == min(4, dec["groups_per_patch"])
        assert pl["steps_per_patch"] == -(-dec["groups_per_patch"] // pl["decode_waves"])
        for k in ("chunks_per_frame", "chunk_tiles", "chunk_pieces", "index_split"):
            assert pl[k] == dec[k], k
        assert pl["lds_bytes"] == lds_for(pix, tw, th, S, pl["max_tiles_x"], pl["max_tiles_y"], pl["rows_per_wave"],
                                          pl["decode_waves"], pl["row_slices"])
        assert fn(W, H, n, tw, th, S, K, 1, edge=edge) == pl   # one shared template: the same launch


# (tw, th, S, pix) -> row_slices, with the winning cost: passes * (rows * batches + 3)
SLICES = [
    ((32, 32, 8, 1), 4),      # 289 shifts, 2 batches a row: ceil(1156 / 256) = 5 passes * (8 * 2 + 3) = 95 (one slice: 134)
    ((32, 32, 8, 2), 4),      # 4 batches a row: 5 * (8 * 4 + 3) = 175
    ((64, 64, 16, 1), 2),     # 1089 shifts, 4 batches: ceil(2178 / 256) = 9 passes * (32 * 4 + 3) = 1179
    ((64, 64, 16, 2), 3),     # 8 batches: ceil(3267 / 256) = 13 * (22 * 8 + 3) = 2327
    ((128, 128, 16, 1), 3),   # 8 batches: 13 * (43 * 8 + 3) = 4511
    ((1, 1, 0, 1), 1),
    ((9, 1, 1, 2), 1),        # one row: nothing to split
    ((7, 7, 1, 1), 7),        # 9 shifts: 63 lanes, one pass of one row
    ((33, 31, 2, 1), 8),      # 25 shifts: 200 lanes, one pass of 4 rows of 3 batches
]


@pytest.mark.parametrize("args,want", SLICES)
def test_hand_derived_row_slices(dv, args, want):
    tw, th, S, pix = args
    fn = dv.match_plan if pix == 1 else dv.match16_plan
    assert fn(4096, 3072, 4, tw, th, S, 8)["row_slices"] == want == slices_for(2 * S + 1, th, tw, pix)


def test_lds_fits_a_workgroup_at_the_largest_sizes(dv):
    worst = 0
    for fn in (dv.match_plan, dv.match16_plan):
        for tw, th, S in ((128, 128, 16), (128, 1, 16), (1, 128, 16), (128, 128, 0), (121, 128, 16), (128, 128, 1)):
            for edge in ("fill", "clamp"):
                worst = max(worst, fn(4096, 3072, 4, tw, th, S, 8, edge=edge)["lds_bytes"])
    assert worst <= 163840, worst
    assert dv.match_plan(4096, 3072, 4, 32, 32, 8, 8)["lds_bytes"] < 16384   # a 48 x 48 search patch does not pay for it


REJECTED = [
    dict(tw=0), dict(th=0), dict(tw=129), dict(th=129), dict(tw=-1), dict(S=-1), dict(S=17),
    dict(K=0), dict(K=-1), dict(n=-1), dict(W=0), dict(edge=2), dict(edge=-1),
    dict(Kt=2), dict(Kt=0), dict(Kt=5), dict(stats=0), dict(stats=8), dict(stats=15), dict(fill=256),
    dict(W=40, H=200, tw=32, th=8, S=8),            # CLAMP: the search patch (48) is wider than the frame
    dict(W=200, H=40, tw=8, th=32, S=8),
    dict(n=1 << 16, K=1 << 15),                     # 2^31 workgroups
    dict(W=16, H=8 * 32768 * 512 + 8),              # more than 32768 plain 512-tile chunks
]


@pytest.mark.parametrize("kw", REJECTED, ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_rejections(dv, kw):
    a = dict(W=300, H=200, n=2, tw=8, th=8, S=2, K=4, Kt=4, edge="clamp", fill=0, stats=7)
    a.update(kw)
    for fn in (dv.match_plan, dv.match16_plan):
        if kw == dict(fill=256) and fn is dv.match16_plan:
            a["fill"] = 65536
        with pytest.raises(ValueError):
            fn(a["W"], a["H"], a["n"], a["tw"], a["th"], a["S"], a["K"], a["Kt"], a["edge"], a["fill"], a["stats"])


def test_accepted_at_the_limits(dv):
    assert dv.match_plan(300, 200, 2, 128, 128, 16, 4, edge="clamp")["pw"] == 160
    assert dv.match_plan(300, 200, 2, 1, 1, 16, 4)["D"] == 33
    assert dv.match_plan(48, 48, 2, 32, 32, 8, 4, edge="clamp")["max_tiles_x"] == 6
    assert dv.match_plan(10, 10, 2, 32, 32, 8, 4, edge="fill")["max_tiles_x"] == 7     # pw > W is legal in FILL mode
    assert dv.match_plan(300, 200, 2, 8, 8, 2, 4, fill=255)["grid"] == 8
    assert dv.match16_plan(300, 200, 2, 8, 8, 2, 4, fill=65535)["grid"] == 8
    for m in range(1, 8):
        assert dv.match_plan(300, 200, 2, 8, 8, 2, 4, stats=m)["surface_bytes"] == 8 * 25 * 8
    assert dv.match_plan(300, 200, 2, 8, 8, 2, 4, stats=("prod",)) == dv.match_plan(300, 200, 2, 8, 8, 2, 4, stats=1)
    p = dv.match_plan(300, 200, 0, 8, 8, 2, 4)
    assert p["grid"] == 0 and p["surface_bytes"] == 0
    with pytest.raises(ValueError):
        dv.match_plan(300, 200, 2, 8, 8, 2, 4, edge="wrap")
    with pytest.raises(ValueError):
        dv.match_plan(300, 200, 2, 8, 8, 2, 4, stats=("prod", "mean"))


def test_null_plan(dv):
    L = dv.lib()
    assert L.dbde_hip_match_plan(300, 200, 2, 8, 8, 2, 4, 4, 0, 0, 7, None) == dv.ERR_ARG
    assert L.dbde16_hip_match_plan(300, 200, 2, 8, 8, 2, 4, 4, 0, 0, 7, None) == dv.ERR_ARG
    assert dv.match_mask(("prod", "sq")) == 5 and dv.match_mask(6) == 6
