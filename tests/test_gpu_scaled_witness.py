"""GPU: the scaled float decode on the witness set of tests/scaled_witness.py, for DBDE and DBDE16 frames.

Every image holds witness (i * s) mod K at raster position i, the dark and gain maps hold the same witnesses' operands
at the same frame coordinates, so each pixel of each window is a witness of a known category at a known arithmetic
site (A, B or C of decode_scaled_kernel's step 4) and slot of a 16-byte block; tests/test_scaled_witness.py proves on
the CPU that these calls put every witness at every site of every kernel instance.  The frames are encoded on the
device, dbde_hip_decode_frames returns the images (the codec is lossless), and the scaled decode's bit patterns are
compared over the whole window with the exact integer reference (IEEE gradual underflow: subnormal operands,
intermediates and BF16 results included) and with tests/scaled_ref.py's numpy definition.  Outputs are guarded and sit
at the address residue the placement proof assumes.  The README's torch expression is evaluated on the device over the
witness set too.
"""
import numpy as np
import pytest

import scaled_ref as sr
import scaled_witness as sw
from test_gpu_project import Batch
from test_gpu_roi16 import Batch16
from test_gpu_scaled import Out, dev
from test_oracle_u16 import o16   # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

PIX = (8, 16)
CALL = {8: "decode_scaled", 16: "decode_scaled16"}
PLAN = {8: "scaled_plan", 16: "scaled16_plan"}
CASES = [(pix, c.name) for pix in PIX for c in sw.cases(pix)]
PAIRS = [(pix, j) for pix in PIX for j in range(len(sw.scalar_witnesses(pix)))]


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


def encoded(codec, o16, pix, frame, n):   # noqa: F811
    """n copies of the (H, W) frame encoded on the device; dbde_hip_decode_frames must return them."""
    import torch
    images = np.ascontiguousarray(np.broadcast_to(frame, (n,) + frame.shape))
    H, W = frame.shape
    if pix == 8:
        b = Batch(codec, None, W, H, n, images=torch.from_numpy(images.astype(np.uint8)).cuda())
        back = b.images.cpu().numpy()
    else:
        b = Batch16(codec, o16, images.astype(np.uint16))
        back = b.gpu_full
    assert back.dtype == images.dtype and np.array_equal(back, images), "decode_frames returns the witness pixels"
    return b, images


def decode(codec, dv, pix, b, case, t, dark, gain):
    """One scaled decode of the case into a guarded output at the residue the placement proof assumes."""
    import torch
    x, y, rw, rh = case.win
    o = Out(case.n, rw, rh, t, odd=sw.RESIDUE)
    es = 4 if t == "f32" else 2
    assert o.t.data_ptr() % 16 == sw.RESIDUE * es, "the output's address residue is the one the site coverage was proven for"
    org = None if case.origins is None else torch.from_numpy(np.asarray(case.origins, np.int32).reshape(case.n, 2)).cuda()
    out, _ = getattr(codec, CALL[pix])(b.buf, b.lead, b.total, b.offs, case.W, case.H, case.n, x, y, rw, rh,
                                       dtype=sr.torch_dtype(t), dark=dark, gain=gain, origins=org, out=o.t)
    codec.sync()
    assert out is o.t
    threads = getattr(dv, PLAN[pix])(case.W, case.H, case.n, x, y, rw, rh, dtype=sr.torch_dtype(t))["threads"]
    return o.read(f"{case.name} {t}"), threads, es


def check(got, want, what, case, threads, es, idx, describe, ref):
    """got == want over the windows; a failure names the frame, position, witness, site and slot."""
    if np.array_equal(got, want):
        return
    f, j, i = (int(v) for v in np.argwhere(got != want)[0])
    site, slot = sw.sites(case, threads, es)
    x, y = sw.origins_of(case)[f].tolist()
    k = int(sw.windowed(case, idx)[f, j, i])
    raise AssertionError(f"{what}: differs from {ref} in frame {f} at window row {j} column {i} (frame row {y + j} column {x + i}): "
                         f"{int(got[f, j, i]):#x} != {int(want[f, j, i]):#x}; witness {k}: {describe(k)}; "
                         f"site {sw.SITES[site[f, j, i]]}, slot {int(slot[f, j, i])} of {16 // es}, {threads} threads; "
                         f"{int((got != want).sum())} of {got.size} elements differ")


@pytest.fixture(scope="module")
def tables():
    """Per pixel size: the witnesses' operands as arrays and their exact results in every type (computed once)."""
    out = {}
    for pix in PIX:
        ws = sw.witnesses(pix)
        p = np.array([w.p for w in ws], np.int64)
        D = np.array([w.D for w in ws], np.uint32)
        G = np.array([w.G for w in ws], np.uint32)
        out[pix] = (ws, p, D, G, {t: sw.exact_array(p, D, G, t) for t in sw.TYPES})
    return out


@pytest.mark.parametrize("pix,name", CASES)
def test_witnesses_in_both_maps_at_every_site(dv, codec, o16, tables, pix, name):   # noqa: F811
    case = next(c for c in sw.cases(pix) if c.name == name)
    ws, p, D, G, exact = tables[pix]
    idx = sw.witness_index(case, len(ws))
    frame = p[idx].astype(np.uint8 if pix == 8 else np.uint16)
    dark, gain = D[idx].view(np.float32), G[idx].view(np.float32)
    b, images = encoded(codec, o16, pix, frame, case.n)
    dd, dg = dev(dark), dev(gain)
    x, y, rw, rh = case.win
    widx = sw.windowed(case, idx)

    def describe(k):
        w = ws[k]
        return f"{w.cat} ({w.t}) p={w.p} D={w.D:#x} G={w.G:#x}"
    for t in sw.TYPES:
        what = f"{pix}-bit {name} {t}"
        got, threads, es = decode(codec, dv, pix, b, case, t, dd, dg)
        check(got, exact[t][widx], what, case, threads, es, idx, describe, "the exact reference")
        want = sr.expected(images, x, y, rw, rh, dark, gain, t, origins=case.origins)
        check(got, want, what, case, threads, es, idx, describe, "scaled_ref.expected")


@pytest.mark.parametrize("pix,j", PAIRS)
def test_scalar_witness_pairs_as_scalars_and_with_one_map(dv, codec, o16, pix, j):   # noqa: F811
    s = sw.scalar_witnesses(pix)[j]
    ps = np.array(s.ps, np.int64)
    D0, G0 = sw.f32_of(s.D0), sw.f32_of(s.G0)
    exact = {t: sw.exact_array(ps, np.full(11, s.D0, np.uint32), np.full(11, s.G0, np.uint32), t) for t in sw.TYPES}

    def describe(k):
        return f"p={s.ps[k]} {s.tags[k]} with D0={s.D0:#x} G0={s.G0:#x}"
    for case in sw.scalar_cases(pix):
        idx = sw.witness_index(case, 11, 1)
        frame = ps[idx].astype(np.uint8 if pix == 8 else np.uint16)
        b, images = encoded(codec, o16, pix, frame, case.n)
        dmap = dev(np.full((case.H, case.W), s.D0, np.uint32).view(np.float32))
        gmap = dev(np.full((case.H, case.W), s.G0, np.uint32).view(np.float32))
        widx = sw.windowed(case, idx)
        for form, dark, gain in (("scalars", D0, G0), ("dark map", dmap, G0), ("gain map", D0, gmap)):
            for t in sw.TYPES:
                what = f"{pix}-bit pair {j} {case.name} {form} {t}"
                got, threads, es = decode(codec, dv, pix, b, case, t, dark, gain)
                check(got, exact[t][widx], what, case, threads, es, idx, describe, "the exact reference")
                want = sr.expected(images, *case.win, np.float32(D0), np.float32(G0), t, origins=case.origins)
                check(got, want, what, case, threads, es, idx, describe, "scaled_ref.expected")


@pytest.mark.parametrize("pix", PIX)
def test_torch_on_the_device_on_the_witnesses(tables, pix):
    """The README's expression, ((images.float() - dark) * gain).to(dtype), on the device over the witness set: equal
    to the exact reference on every witness, the subnormal categories included (observed on gfx950: torch's kernels do
    not flush binary32 subnormals either)."""
    import torch
    ws, p, D, G, exact = tables[pix]
    x = torch.from_numpy(p.astype(np.int32)).cuda()
    dark, gain = (torch.from_numpy(a.view(np.float32).copy()).cuda() for a in (D, G))
    sub = np.array([w.cat in sw.SUBNORMAL_CATEGORIES for w in ws])
    assert sub.sum() >= 40
    for t in sw.TYPES:
        v = ((x.float() - dark) * gain).to(sr.torch_dtype(t))
        got = v.view(torch.int32 if t == "f32" else torch.int16).cpu().numpy().view(sr.BITS[t])
        same = got == exact[t]
        print(f"torch on the device, {pix}-bit {t}: {int(same[~sub].sum())} of {int((~sub).sum())} other witnesses and "
              f"{int(same[sub].sum())} of {int(sub.sum())} witnesses of the subnormal categories equal the exact reference")
        bad = np.flatnonzero(~same & ~sub)
        assert bad.size == 0, f"torch differs from the exact reference in {t} on witness {ws[bad[0]]}"
        bad = np.flatnonzero(~same & sub)
        assert bad.size == 0, f"torch differs from the exact reference in {t} on the subnormal witness {ws[bad[0]]}"
