"""CPU: the geometry matrix of tests/geometry_cases.py, judged before any GPU run.

tests/test_gpu_geometry.py runs every stream-reading family at four frames chosen for roi_index_geometry's three regimes.
A GPU case shows something only if its frame really is in the regime, its windows really sit on the long prefix, the
piece seam or the straddled tile row, and its content tells a right tile from its neighbours.  Here, without a device:

  * every family's plan function reports the table's index geometry for every geometry (they share one planner; a
    geometry swapped for one of another regime fails here);
  * roi_index_geometry restated in Python (as tests/test_roi_plan.py does) gives, for every window, origin and patch,
    what the front half of a kernel meets there: npre >= 500, a first tile in a second or later piece with npre >= 1,
    a tile row whose window tiles lie in two chunks (a window moved off its seam or straddled row fails here);
  * the cap: the reference output of every window differs from that of the window 8 px left, right, up and down, for
    every accepted frame, and the match surfaces at every search origin differ from those 8 px away (a stream replaced by
    a constant image fails here) -- a condition on the inputs, not a measurement;
  * the verdicts are as built: frame 2 rejected, the others accepted.
"""
import numpy as np
import pytest

import geometry_cases as gc
import match_ref as mr
import patch_ref as pr

CELLS = [(name, bits) for name in gc.NAMES for bits in gc.BITS]


@pytest.fixture(scope="module")
def dv():
    import os
    import dbde_video_cpp_amd as m
    if not os.path.exists(m.LIB_PATH):
        m.build()
    return m


def split_for(n, cpf):
    """index_split_for (dbde_capi.cpp), as tests/test_roi_plan.py restates it."""
    return 1 if (n >= 256 or cpf < 8) else max(1, min(1024 // n, (cpf + 3) // 4))


def plans(dv, name, n):
    """{family: plan} of every stream-reading family, both pixel sizes, at the geometry's first window."""
    W, H = gc.GEOMETRIES[name]
    win = gc.WINDOWS[name][0]
    al = gc.aligned(win)
    (rw, rh), _ = gc.MOVING[name]
    lab = np.zeros((H, W), np.int32)
    lab[win[1]:win[1] + win[3], win[0]:win[0] + win[2]] = 1
    info = dv.trace_map_summary(lab, 1)
    tw, th, S = gc.MATCH[0]
    out = {}
    for s in ("", "16"):
        f = lambda base, alt=None: getattr(dv, (alt or base).replace("#", s))   # noqa: E731
        out["decode_roi" + s] = f("roi#_plan")(W, H, n, *win)
        out["project" + s] = f("project#_plan")(W, H, n, *win)
        out["traces" + s] = f("trace#_plan")(W, H, n, info)
        out["histogram" + s] = f("histogram#_plan")(W, H, n, *win)
        out["decode_binned" + s] = f("binned#_plan")(W, H, n, 4, *al)
        out["decode_scaled" + s] = f("scaled#_plan")(W, H, n, *win)
        out["crop_frames" + s] = f("crop#_plan")(W, H, n, *al)
        out["decode_mask" + s] = f("mask#_plan")(W, H, n, *win)
        out["decode_patches" + s] = f("patches#_plan")(W, H, n, 24, 16, 6, "fill")
        out["project_groups" + s] = f("project_groups#_plan")(W, H, n, *win, group_frames=2)
        out["project_weighted" + s] = f("wproject#_plan")(W, H, n, *win, regressors=2)
        out["patch_moments" + s] = f("patch_moments#_plan")(W, H, n, 24, 16, 6, "fill")
        out["project_counts" + s] = f("counts#_plan")(W, H, n, *win, levels=2)
        out["project_pairs" + s] = f("pairs#_plan")(W, H, n, *win)
        out["project_lag" + s] = f("lag#_plan")(W, H, n, *win, lag=1)
        out["project_registered" + s] = f("registered#_plan")(W, H, n, rw, rh)
        out["match_patches" + s] = f("match#_plan")(W, H, n, tw, th, S, 4, edge="fill")
    return out


@pytest.mark.parametrize("name", gc.NAMES)
def test_every_family_plans_the_regime(dv, name):
    W, H = gc.GEOMETRIES[name]
    g = gc.index_geometry(W, H)
    assert g["regime"] == gc.REGIME[name]
    want = dict(gc.PLAN[name])
    want.setdefault("index_split", split_for(3, want["chunks_per_frame"]))
    # the restated geometry agrees with the table (chunk_pieces: 0 = plain chunks)
    assert g["cpf"] == want["chunks_per_frame"] and g["ct"] == want["chunk_tiles"]
    assert (0 if g["regime"] == "C" else g["pieces"]) == want["chunk_pieces"]
    got = plans(dv, name, 3)
    assert len(got) == 34
    for family, pl in got.items():
        assert {k: pl[k] for k in want} == want, (family, pl)
    # few frames of row1025 and plain take the split index, the stream's N frames too; the others never
    for n in (3, gc.N):
        split = dv.roi_plan(W, H, n, 0, 0, 8, 8)["index_split"]
        assert split == split_for(n, g["cpf"])
        assert (split > 1) == (name in ("row1025", "plain")), (name, n, split)
    if name == "plain":
        # 512 is no multiple of the 3 tiles across: 128 of the 192 chunk boundaries fall inside a tile row, the first
        # at tile 512 = row 170, column 2; boundary 100 inside row DEEP
        inside = [c for c in range(1, g["cpf"]) if (512 * c) % g["w"]]
        assert len(inside) == 128 and inside[0] == 1 and divmod(512, g["w"]) == (170, 2)
        assert divmod(512 * 100, g["w"]) == (gc.DEEP, 2)
        assert H % 8 == 3 and g["h"] == 32769
    else:
        assert H % 8 == 1                                  # the last tile row is 1 px high
        assert g["w"] == {"row512": 512, "row513": 513, "row1025": 1025}[name]


def hard_spot(name, win):
    """Which of the geometry's hard spots the window's tile rows meet: (largest npre, largest npre of a row whose first
    tile lies in a second or later piece or None, tile rows whose window tiles lie in two chunks)."""
    W, H = gc.GEOMETRIES[name]
    rows = gc.window_rows(W, H, win)
    assert all(0 <= npre < 512 for _, _, _, npre, _, _ in rows)
    later = [npre for _, _, _, npre, piece, _ in rows if piece >= 1]
    return max(r[3] for r in rows), (max(later) if later else None), [r[0] for r in rows if len(r[5]) > 1]


def test_windows_sit_on_the_hard_spots():
    W = gc.WINDOWS
    # row512: the first window's prefix is at least 500 depth bytes, the full frame starts every row at its chunk
    assert hard_spot("row512", W["row512"][0])[0] >= 500
    assert hard_spot("row512", W["row512"][1])[0] == 2051 // 8
    assert hard_spot("row512", W["row512"][2])[0] == 0
    for name in ("row513", "row1025"):
        wins = W[name]
        full = wins[-1]
        assert full == (0, 0) + gc.GEOMETRIES[name]
        # a window wholly in a later piece: its first tile is in that piece, past the piece's first tile where the frame
        # has such a tile (row513's second piece holds one tile, so there npre is 0 and the seam window has the prefix)
        _, later, _ = hard_spot(name, wins[0])
        assert later is not None
        # across the seam: the first tile in piece 0 with a long prefix, tiles in two chunks
        top, _, two = hard_spot(name, (4080, 3, 24, 14))
        assert (4080, 3, 24, 14) in wins and top == 510 and two == [0, 1, 2]
        assert hard_spot(name, full)[2] == list(range((gc.GEOMETRIES[name][1] + 7) // 8))
    # npre >= 1 in a second or later piece: row513's second piece holds one tile, so no first tile there has anything in
    # front of it (npre is 0 by construction); row1025 has a window that starts 238 tiles inside its second piece
    assert hard_spot("row513", W["row513"][0])[1] == 0
    assert hard_spot("row1025", W["row1025"][0])[1] == 0 and hard_spot("row1025", W["row1025"][1])[1] == 0
    assert {r[4] for r in gc.window_rows(8200, 33, W["row1025"][0])} == {1}
    assert {r[4] for r in gc.window_rows(8200, 33, W["row1025"][1])} == {2}       # the last piece holds one tile too
    assert (6001, 2, 300, 20) in W["row1025"] and hard_spot("row1025", (6001, 2, 300, 20))[1] == 6001 // 8 - 512 >= 1
    assert hard_spot("row1025", (4090, 1, 4110, 30))[0] == 511 and (4090, 1, 4110, 30) in W["row1025"]
    assert all(len(ch) == 3 for *_, ch in gc.window_rows(8200, 33, (4090, 1, 4110, 30)))
    # plain: the straddled rows
    assert hard_spot("plain", W["plain"][0])[2] == [170]
    assert hard_spot("plain", W["plain"][1])[2] == [gc.DEEP]
    assert [r[0] for r in gc.window_rows(24, 262147, W["plain"][1])] == [gc.DEEP - 1, gc.DEEP, gc.DEEP + 1]
    assert [r[0] for r in gc.window_rows(24, 262147, W["plain"][2])] == [32768]
    assert W["plain"][2][0] + W["plain"][2][2] == 24 and W["plain"][2][1] + W["plain"][2][3] == 262147
    assert max(r[3] for n in W["plain"] for r in gc.window_rows(24, 262147, n)) >= 509   # and long prefixes there too
    for name in gc.NAMES:                # every window is inside its frame
        for x, y, rw, rh in W[name]:
            assert 0 <= x and 0 <= y and rw > 0 and rh > 0 and x + rw <= gc.GEOMETRIES[name][0] and y + rh <= gc.GEOMETRIES[name][1]


@pytest.mark.parametrize("name", gc.NAMES)
def test_origins_and_patches_sit_on_the_hard_spots(name):
    W, H = gc.GEOMETRIES[name]
    (rw, rh), org = gc.MOVING[name]
    assert len(org) == gc.N and len(set(org)) == gc.N
    assert all(0 <= ox <= W - rw and 0 <= oy <= H - rh for ox, oy in org)          # no clamp moves them
    spots = [hard_spot(name, (ox, oy, rw, rh)) for f, (ox, oy) in enumerate(org) if f != gc.BAD]
    if name == "row512":
        assert max(s[0] for s in spots) >= 500 and min(s[0] for s in spots) < 400
    elif name == "plain":
        assert any(s[2] for s in spots) and not all(s[2] for s in spots)           # on the straddled row, and off it
    else:
        assert any(s[2] for s in spots) and any(s[1] is not None and not s[2] for s in spots)   # across, and behind
        assert any(s[1] is None for s in spots)                                                 # and in front
    # the patches: clipped to the frame, one over the right edge or the seam, one over the bottom edge
    pw, ph = 24, 16
    boxes = [(max(ox, 0), max(oy, 0), min(ox + pw, W) - max(ox, 0), min(oy + ph, H) - max(oy, 0)) for ox, oy in gc.PATCHES[name]]
    assert all(b[2] > 0 and b[3] > 0 for b in boxes)
    assert any(ox + pw > W for ox, oy in gc.PATCHES[name]) and any(oy + ph > H for ox, oy in gc.PATCHES[name])
    assert any(ox < 0 or oy < 0 for ox, oy in gc.PATCHES[name])
    two = [hard_spot(name, b)[2] for b in boxes]
    if name == "row512":
        assert max(hard_spot(name, b)[0] for b in boxes) >= 500
    else:
        assert sum(bool(t) for t in two) >= 2, two
    for tw, th, S in gc.MATCH:
        pw, ph = tw + 2 * S, th + 2 * S
        so = gc.SEARCH[name][S]
        assert len(so) == 4
        mode = gc.match_mode(name, tw, th, S)
        assert mode == (pr.CLAMP if S == 2 else pr.FILL)
        boxes = []
        for ox, oy in so:
            if mode == pr.CLAMP:
                ox, oy = min(max(ox, 0), W - pw), min(max(oy, 0), H - ph)
            b = (max(ox, 0), max(oy, 0), min(ox + pw, W) - max(ox, 0), min(oy + ph, H) - max(oy, 0))
            assert b[2] > 0 and b[3] > 0
            boxes.append(b)
        if name == "row512":
            assert max(hard_spot(name, b)[0] for b in boxes) >= 500
        else:
            assert sum(bool(hard_spot(name, b)[2]) for b in boxes) >= 2


@pytest.mark.parametrize("name,bits", CELLS)
def test_streams_are_as_built(name, bits):
    W, H = gc.GEOMETRIES[name]
    frames, rows, images = gc.host_frames(name, bits)
    assert len(frames) == gc.N
    assert [im is None for im in images] == [f == gc.BAD for f in range(gc.N)]
    for f in range(gc.N):
        assert rows[f][3] == (20 if f == gc.BAD else len(frames[f])) and (f != gc.BAD or rows[f][0] == 0xFFFFFFFF)
        if f != gc.BAD:
            assert images[f].shape == (H, W) and images[f].dtype == (np.uint8 if bits == 8 else np.uint16)
    # the one broken rule: the depth of the last tile, nothing else
    import crafted as cr
    assert cr.broken_rules(frames[gc.BAD][20:], W, H, bits) == {"depth"}
    p = gc.pool(name, bits)
    assert p.ok == [f != gc.BAD for f in range(gc.N)] and p.n == gc.N and gc.pool(name, bits) is p
    for f in range(gc.N):                                             # "residues": frame f's payload at residue f mod 16
        assert (p.lead + int(p.offs[f]) + cr.payload_start(frames[f])) % 16 == f % 16
        at = p.lead + int(p.offs[f])
        assert np.array_equal(p.buf[at:at + len(frames[f])], frames[f])


@pytest.mark.parametrize("name,bits", CELLS)
def test_a_wrong_tile_changes_every_expected_window(name, bits):
    """The cap.  For every accepted frame the window's pixels differ from those of the window 8 px left, right, up and
    down (so does every per-frame output: decode_roi, crop, scaled, binned, mask, histogram rows are functions of
    them), and so do the sums over the accepted frames (the projections); the same for every moving origin, patch and
    search patch, on what their families' references give."""
    _, _, images = gc.host_frames(name, bits)
    live = [im for im in images if im is not None]
    W, H = gc.GEOMETRIES[name]

    def cut(im, win):
        x, y, rw, rh = win
        return im[y:y + rh, x:x + rw]

    (rw, rh), org = gc.MOVING[name]
    wins = list(gc.WINDOWS[name]) + [(ox, oy, rw, rh) for ox, oy in org]
    for win in wins:
        moved = gc.displaced(name, win)
        assert moved or win[2:] == (W, H), (name, win)
        for other in moved:
            for im in live:
                assert not np.array_equal(cut(im, win), cut(im, other)), (name, bits, win, other)
            total = sum(cut(im, win).astype(np.int64) for im in live)
            assert not np.array_equal(total, sum(cut(im, other).astype(np.int64) for im in live)), (name, bits, win, other)
            assert not np.array_equal(np.max([cut(im, win) for im in live], 0), np.max([cut(im, other) for im in live], 0))
    for win in gc.WINDOWS[name]:         # ... and a window's content is not the same in two frames
        for k, im in enumerate(live):
            assert all(not np.array_equal(cut(im, win), cut(o, win)) for o in live[:k])
    for mode in (pr.CLAMP, pr.FILL):
        for ox, oy in gc.PATCHES[name]:
            for im in live:
                here = pr.patch(im, W, H, 24, 16, ox, oy, mode, 0x5A)[0]
                for dx, dy in ((-8, 0), (8, 0), (0, -8), (0, 8)):
                    there, used = pr.patch(im, W, H, 24, 16, ox + dx, oy + dy, mode, 0x5A)
                    clamped_back = mode == pr.CLAMP and tuple(used) == tuple(pr.patch(im, W, H, 24, 16, ox, oy, mode, 0x5A)[1])
                    assert clamped_back or not np.array_equal(here, there), (name, bits, mode, (ox, oy), (dx, dy))
    for tw, th, S in gc.MATCH:
        T = gc.templates(name, bits, tw, th)
        mode = gc.match_mode(name, tw, th, S)
        here = mr.expected(images, W, H, T, S, gc.search_origins(name, S), None, mode, 0x5A)
        for dx, dy in ((-8, 0), (8, 0), (0, -8), (0, 8)):
            there = mr.expected(images, W, H, T, S, gc.search_origins(name, S) + (dx, dy), None, mode, 0x5A)
            for f in range(gc.N):
                for k in range(4):
                    if f == gc.BAD:
                        assert (here[0][f, k] == mr.UNTOUCHED).all()
                    elif tuple(here[3][f, k]) != tuple(there[3][f, k]):      # (the clamp may put both at the same place)
                        for i in range(3):
                            assert not np.array_equal(here[i][f, k], there[i][f, k]), (name, bits, S, f, k, (dx, dy), mr.NAMES[i])


@pytest.mark.parametrize("bits", gc.BITS)
def test_row512_outputs_depend_on_the_last_prefix_dword(bits):
    """That the matrix bites, by reasoning instead of a broken build: a prefix sum that drops its last dword (nd - 1 in
    a kernel's front half) loses the last 1..4 depth bytes in front of the row's first tile -- how many depends on the
    frame's address, the byte right in front of it always.  For the first window and for every search patch of row512,
    in every accepted frame, there is a tile row with a long prefix whose last depth byte is not 0: the payload offset
    of that row then comes out at least 8 bytes short, and the bytes there are not those of the row's first tile that
    has a payload, so its pixels (and with them every output and every match surface, by the cap above) differ."""
    import crafted as cr
    name = "row512"
    W, H = gc.GEOMETRIES[name]
    frames = gc.host_frames(name, bits)[0]
    T = cr.tiles(W, H)
    boxes = [gc.WINDOWS[name][0]]
    for tw, th, S in gc.MATCH:
        pw, ph = tw + 2 * S, th + 2 * S
        clamp = gc.match_mode(name, tw, th, S) == pr.CLAMP
        for ox, oy in gc.SEARCH[name][S]:
            if clamp:
                ox, oy = min(max(ox, 0), W - pw), min(max(oy, 0), H - ph)
            boxes.append((max(ox, 0), max(oy, 0), min(ox + pw, W) - max(ox, 0), min(oy + ph, H) - max(oy, 0)))
    long_prefix = 0
    for f, fr in enumerate(frames):
        if f == gc.BAD:
            continue
        depths = fr[24:24 + T].astype(np.int64)
        pay = fr[cr.payload_start(fr):]
        offs = 8 * np.concatenate([[0], np.cumsum(depths)])
        for box in boxes:
            bites = 0
            for ty, pos0, c, npre, _, _ in gc.window_rows(W, H, box):
                if npre < 400 or depths[pos0 - 1] == 0:
                    continue
                long_prefix += 1
                tiles_x = (box[0] + box[2] - 1) // 8 - box[0] // 8 + 1
                first = next((t for t in range(pos0, pos0 + tiles_x) if depths[t]), None)
                if first is None:
                    continue
                size = 8 * depths[first]
                right = pay[offs[first]: offs[first] + size]
                for last in range(1, 5):          # the depth bytes the dropped dword can hold
                    short = 8 * depths[pos0 - last: pos0].sum()
                    assert short >= 8 and not np.array_equal(right, pay[offs[first] - short: offs[first] - short + size])
                bites += 1
            assert bites or box[0] // 8 < 400, (bits, f, box)
    assert long_prefix >= 4 * 3
