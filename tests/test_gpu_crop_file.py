"""GPU: cropping.crop_file -- a sub-video cut out of a .dbde file in the compressed domain.

The source is written by the HIP writer (oracle_ffi.WALKER_FILE's odd geometry); the cropped file must be the video
header of the window's size followed by tests/crop_ref.py's frames, for pieces small enough to cut frames, and the
reference's own walker must read it.
"""
import numpy as np
import pytest

import crop_ref
from oracle_ffi import WALKER_FILE, Reference

pytestmark = pytest.mark.gpu
SEED = 0xDBDE2016


@pytest.fixture(scope="module")
def dv():
    import dbde_video_cpp_amd as m
    return m


@pytest.fixture(scope="module")
def codec(dv):
    c = dv.Codec(0)
    yield c
    c.close()


def write_source(codec, path, W, H, n, first, hz):
    imgs = codec.synth_frames("mixed", SEED, 0, n, W, H)
    with codec.open_writer(path, W, H, frame_hz=hz, batch_frames=5) as w:
        w.put(imgs, n, first_index=first)
    return imgs.cpu().numpy()


def source_frames(data, W, H):
    out, at = [], 28
    while at < len(data):
        n = crop_ref.frame_length(data[at:], W, H)
        out.append(data[at:at + n])
        at += n
    return out


@pytest.mark.parametrize("window", [(8, 16, 301, 50), (0, 0, 333, 77), (200, 8, 133, 69), (328, 72, 5, 5)])
@pytest.mark.parametrize("batch_bytes", [1 << 20, 5000, 777])
def test_crop_file_equals_header_and_model_frames(dv, codec, oracle, tmp_path, window, batch_bytes):
    from importlib import import_module
    cropping = import_module("dbde_video_cpp_amd.cropping")
    f = WALKER_FILE
    W, H, n, first, hz = f["W"], f["H"], f["n"], f["first_index"], f["frame_hz"]
    x, y, rw, rh = window
    src, dst = str(tmp_path / "src.dbde"), str(tmp_path / "dst.dbde")
    imgs = write_source(codec, src, W, H, n, first, hz)
    data = np.fromfile(src, np.uint8)
    frames = source_frames(data, W, H)
    assert len(frames) == n and min(len(fr) for fr in frames) > 777    # the small pieces cut every frame
    written, rejected, size = cropping.crop_file(codec, src, dst, x, y, rw, rh, batch_bytes=batch_bytes)
    got = np.fromfile(dst, np.uint8)
    want = np.concatenate([oracle.pack_video_header(3, rh, rw, hz)] +
                          [crop_ref.crop_frame(fr, W, H, x, y, rw, rh) for fr in frames])
    assert (written, rejected, size) == (n, 0, len(want))
    assert got.tobytes() == want.tobytes()
    if Reference.available():
        reference = Reference()
        for keep in f["keeps"]:
            cnt, hw, last, img = reference.walk_file(dst, f["buffered"], rw, rh, keep=keep)
            assert cnt == n and hw == (rh, rw) and last == first + n - 1
            assert np.array_equal(img, imgs[keep - 1][y:y + rh, x:x + rw])


def test_crop_file_leaves_rejected_frames_and_a_cut_tail_out(dv, codec, oracle, tmp_path):
    from importlib import import_module
    cropping = import_module("dbde_video_cpp_amd.cropping")
    W, H, n = 120, 50, 6
    rng = np.random.default_rng(2)
    imgs = [rng.integers(0, 256, (H, W), dtype=np.uint8) >> (k % 4) for k in range(n)]
    frames = [oracle.pack_frame(k, imgs[k], W, H) for k in range(n)]
    frames[2] = frames[2].copy()
    frames[2][24 + 3] = 9                                    # a depth byte > 8 with n64 unchanged: rejected, same length
    src, dst = str(tmp_path / "s.dbde"), str(tmp_path / "d.dbde")
    np.concatenate([oracle.pack_video_header(3, H, W, 25.0)] + frames + [frames[0][:100]]).tofile(src)
    written, rejected, size = cropping.crop_file(codec, src, dst, 8, 8, 100, 37, batch_bytes=4096)
    want = np.concatenate([oracle.pack_video_header(3, 37, 100, 25.0)] +
                          [crop_ref.crop_frame(fr, W, H, 8, 8, 100, 37) for k, fr in enumerate(frames) if k != 2])
    assert (written, rejected, size) == (n - 1, 1, len(want))
    assert np.fromfile(dst, np.uint8).tobytes() == want.tobytes()
