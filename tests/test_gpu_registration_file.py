"""GPU: dbde_video_cpp_amd.registration's drivers.

registered_file at batch sizes that do and do not divide the frame count equals registered_image bit for bit, and both
equal tests/registered_ref.py over the frames that were encoded.  The whole chain tracking.follow ->
shifts_from_centres -> origins_from_shifts -> project_registered runs on a synthetic scene: a bright disc on a fixed,
noise-free background, the scene moving under the sensor by known integer shifts.  The chain recovers the shifts, and
the registered maximum and minimum both equal the scene's unshifted window exactly.
"""
import numpy as np
import pytest

import registered_ref as rr

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


def encode(codec, imgs, W, H, n):
    buf, lead, cap = codec.alloc_stream(W, H, n)
    offs, sizes = codec.encode_frames(imgs, W, H, n, buf, lead, cap)
    codec.sync()
    return buf, lead, int((offs[-1] + sizes[-1]).item()), offs


def test_registered_file_equals_registered_image(dv, codec, tmp_path):
    import torch
    from dbde_video_cpp_amd import registration as reg
    W, H, n = 72, 40, 13
    imgs = codec.synth_frames("mixed", 78, 0, n, W, H)
    path = str(tmp_path / "r.dbde")
    with codec.open_writer(path, W, H, frame_hz=30.0, batch_frames=4) as wtr:
        wtr.put(imgs, n)
    buf, lead, total, offs = encode(codec, imgs, W, H, n)
    rng = np.random.default_rng(78)
    shifts = rng.integers(-6, 7, (n, 2))
    host = list(imgs.cpu().numpy())
    for max_shift in (None, 4):           # 4: some frames moved further and are clamped
        for stats in (("max", "min", "sum", "sumsq"), ("sum",)):
            used = torch.full((n, 2), -77, dtype=torch.int32, device="cuda")
            mem, at, res = reg.registered_image(codec, buf, lead, total, offs, W, H, n, shifts, stats=stats,
                                                max_shift=max_shift, origins_used=used)
            codec.sync()
            origins, rw, rh, at2 = reg.origins_from_shifts(shifts, W, H, max_shift)
            assert at == at2 and tuple(mem.sum.shape) == (rh, rw)
            want = rr.registered(host, origins.numpy(), rw, rh)
            for k in stats:
                t = getattr(mem, k).cpu().numpy()
                assert np.array_equal(t.view(np.uint64) if k in ("sum", "sumsq") else t, want[k]), (max_shift, k)
            assert used.tolist() == [list(want["used"][f]) for f in range(n)]
            assert (max_shift is None) == (used.cpu().numpy() == origins.numpy()).all()      # 4 clamps, None does not
            for batch in (5, 4, 1, 13, 64):
                got, at3, res_f = reg.registered_file(codec, path, shifts, stats=stats, batch=batch, max_shift=max_shift)
                codec.sync()
                assert at3 == at and int(got.count.item()) == n
                for k in stats:
                    assert torch.equal(getattr(got, k), getattr(mem, k)), (max_shift, stats, batch, k)
                assert tuple(res_f.shape) == (n, 4) and res_f[:, 1].tolist() == list(range(n))
    with pytest.raises(ValueError):
        reg.registered_file(codec, path, shifts, bits=16)
    with pytest.raises(ValueError):
        reg.registered_file(codec, path, shifts[:n - 1])          # fewer shifts than frames
    with pytest.raises(ValueError):
        reg.registered_image(codec, buf, lead, total, offs, W, H, n, shifts[:n - 1])


def test_follow_to_registered_projection_recovers_the_scene(dv, codec):
    import torch
    from dbde_video_cpp_amd import registration as reg, tracking
    W, H, n, M = 96, 64, 12, 12
    yy, xx = np.mgrid[0:H + 2 * M, 0:W + 2 * M]
    scene = (20 + (3 * xx + 5 * yy) % 97).astype(np.uint8)                  # fixed, noise-free, below the threshold
    cx, cy = M + 40, M + 30
    scene[(xx - cx) ** 2 + (yy - cy) ** 2 <= 36] = 250                      # the fiducial: a disc of radius 6
    rng = np.random.default_rng(4)
    steps = rng.integers(-2, 3, (n, 2))
    steps[0] = 0
    shifts = np.clip(np.cumsum(steps, 0), -M + 1, M - 1)                    # a walk of at most 2 pixels a frame
    # frame_f[Y + dy][X + dx] = scene window [Y][X]
    frames = np.stack([scene[M - dy:M - dy + H, M - dx:M - dx + W] for dx, dy in shifts])
    imgs = torch.from_numpy(frames.copy()).cuda()
    buf, lead, total, offs = encode(codec, imgs, W, H, n)
    centres, _ = tracking.follow(codec, buf, lead, total, offs, W, H, n, [(cx - M, cy - M)], 32, 32, 200, 255,
                                 weight="count")
    got_shifts = reg.shifts_from_centres(centres)
    origins, rw, rh, (X0, Y0) = reg.origins_from_shifts(got_shifts, W, H)
    pr, _ = codec.project_registered(buf, lead, total, offs, W, H, n, rw, rh, origins, stats=("max", "min"))
    codec.sync()
    assert np.array_equal(got_shifts.cpu().numpy(), shifts)
    window = scene[M + Y0:M + Y0 + rh, M + X0:M + X0 + rw]
    assert np.array_equal(pr.max.cpu().numpy(), window) and np.array_equal(pr.min.cpu().numpy(), window)
    assert int(pr.count.item()) == n and (window == 250).any() and len(np.unique(shifts, axis=0)) > 3
    # an unregistered projection of the same frames smears the disc: the registration is what made them equal
    flat, _ = codec.project(buf, lead, total, offs, W, H, n, X0, Y0, rw, rh, stats=("max", "min"))
    codec.sync()
    assert not torch.equal(flat.max, flat.min)
