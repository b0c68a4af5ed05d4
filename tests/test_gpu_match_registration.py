"""GPU: shift estimation by block matching (registration.estimate_shifts / estimate_file) and the chain into the
registered projection.

The scene is tests/match_cases.py's: a smooth synthetic image moved by known integer shifts within +-6, searched with
S = 8 from five 32 x 32 templates of the unmoved frame.  tests/test_match_ref.py checks on the CPU that the reference
surfaces have a unique maximum at the true shift, for the mean over the patches and for every patch on its own; here the
library must return exactly those shifts.
"""
import os

import numpy as np
import pytest

import match_cases as mc
import match_gpu as mg

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
def scene(codec):
    ref, frames = mc.scene_frames()
    return ref, frames, mg.Encoded(codec, frames)


def estimate(codec, scene, n=None, **kw):
    import torch
    from dbde_video_cpp_amd import registration
    sc = mc.SCENE
    ref, frames, e = scene
    n = sc["n"] if n is None else n
    return registration.estimate_shifts(codec, *e.stream, sc["W"], sc["H"], n, torch.from_numpy(ref).cuda(),
                                        np.array(sc["positions"]), sc["tw"], sc["th"], sc["S"], **kw)


def test_estimate_shifts_returns_the_known_shifts(codec, scene):
    import torch
    from dbde_video_cpp_amd import registration
    sc = mc.SCENE
    shifts, score, per_patch = estimate(codec, scene)
    codec.sync()
    want = np.array(sc["shifts"])
    assert shifts.dtype == torch.int32 and np.array_equal(shifts.cpu().numpy(), want)
    assert per_patch.dtype == torch.int32 and tuple(per_patch.shape) == (sc["n"], len(sc["positions"]), 2)
    assert np.array_equal(per_patch.cpu().numpy(), np.repeat(want[:, None], len(sc["positions"]), 1))
    assert (score.cpu().numpy() > 0.999999).all()      # the same pixels: zncc is 1 up to its float64 rounding
    # a rejected frame: shift (0, 0) and score NaN; its neighbours as before
    ref, frames, e = scene
    buf = e.buf.clone()
    buf[e.lead + int(e.offs[1]) + 24] = 9               # frame 1's first depth byte
    s2, sc2, pp2 = registration.estimate_shifts(codec, buf, e.lead, e.total, e.offs, sc["W"], sc["H"], sc["n"],
                                                torch.from_numpy(ref).cuda(), np.array(sc["positions"]), sc["tw"], sc["th"],
                                                sc["S"])
    want2 = want.copy()
    want2[1] = 0
    assert np.array_equal(s2.cpu().numpy(), want2) and np.isnan(sc2.cpu().numpy()[1]) and (pp2[1] == 0).all()
    assert not np.isnan(np.delete(sc2.cpu().numpy(), 1)).any()
    # helpers
    org = registration.search_origins(sc["positions"], sc["S"], 2)
    assert org.dtype == torch.int32 and org.tolist() == [[[x - 8, y - 8] for x, y in sc["positions"]]] * 2
    T = registration.templates_from_image(torch.from_numpy(ref), sc["positions"], sc["tw"], sc["th"])
    x, y = sc["positions"][2]
    assert tuple(T.shape) == (5, 32, 32) and np.array_equal(T[2].numpy(), ref[y:y + 32, x:x + 32])
    with pytest.raises(ValueError):
        registration.templates_from_image(torch.from_numpy(ref), [(sc["W"] - 31, 0)], 32, 32)


def test_chain_into_the_registered_projection(codec, scene):
    """estimate_shifts -> origins_from_shifts -> project_registered: the planes equal project's planes of the unmoved
    scene (the reference frame n times) on the common window."""
    import torch
    from dbde_video_cpp_amd import registration
    sc = mc.SCENE
    ref, frames, e = scene
    W, H, n = sc["W"], sc["H"], sc["n"]
    shifts, _, _ = estimate(codec, scene)
    origins, rw, rh, (X0, Y0) = registration.origins_from_shifts(shifts, W, H)
    assert (rw, rh, X0, Y0) == (W - 12, H - 12, 6, 6)
    pr_reg, _ = codec.project_registered(*e.stream, W, H, n, rw, rh, origins)
    still = mg.Encoded(codec, np.repeat(ref[None], n, 0))
    pr_still, _ = codec.project(*still.stream, W, H, n, X0, Y0, rw, rh)
    codec.sync()
    for s in ("max", "min", "sum", "sumsq"):
        assert torch.equal(getattr(pr_reg, s), getattr(pr_still, s)), s
    assert np.array_equal(pr_reg.max.cpu().numpy(), ref[Y0:Y0 + rh, X0:X0 + rw])
    # ... and through registered_image, which takes the shifts as they come
    pr2, at, _ = registration.registered_image(codec, *e.stream, W, H, n, shifts)
    codec.sync()
    assert at == (X0, Y0) and torch.equal(pr2.sum, pr_still.sum)


def test_estimate_file_in_three_batches_equals_one_call(codec, dv, scene, tmp_path):
    import torch
    from dbde_video_cpp_amd import registration
    sc = mc.SCENE
    ref, frames, e = scene
    W, H, n = sc["W"], sc["H"], sc["n"]
    path = os.path.join(tmp_path, "moved.dbde")
    host = e.buf.cpu().numpy()
    offs = e.offs.cpu().numpy()
    with open(path, "wb") as f:
        f.write(dv.pack_video_header(3, H, W, 30.0).tobytes())
        f.write(host[e.lead + int(offs[0]): e.lead + e.total].tobytes())     # the frames lie back to back
    one = estimate(codec, scene)
    got = registration.estimate_file(codec, path, torch.from_numpy(ref).cuda(), sc["positions"], sc["tw"], sc["th"], sc["S"],
                                     batch=4)   # 4 + 4 + 1 frames
    codec.sync()
    assert got[0].shape[0] == n
    for a, b in zip(got, one):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert np.array_equal(got[0].cpu().numpy(), np.array(sc["shifts"]))
