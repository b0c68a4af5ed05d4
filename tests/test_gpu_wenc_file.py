"""GPU: FileWriter.put_window -- windows of pitched source images appended to a .dbde file through the writer's
double-buffered path.  5 + 3 frames of a 33 x 31 window give the file that a video header plus the oracle's frames of
the windows make, and open_reader reads the windows back."""
import numpy as np
import pytest

import wenc_ref as wr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dv():
    import dbde_video_cpp_amd as m
    m.build()
    return m


@pytest.fixture(scope="module")
def codec(dv):
    c = dv.Codec(0)
    yield c
    c.close()


def test_put_window_writes_header_and_oracle_frames(dv, codec, oracle, tmp_path):
    import torch
    W, H, rw, rh, x, y = 61, 40, 33, 31, 5, 3
    rng = np.random.default_rng(33)
    host = (rng.integers(0, 256, (8, H, W)) >> rng.integers(0, 8, (8, 1, 1))).astype(np.uint8)
    frames = torch.from_numpy(host).cuda()
    path = str(tmp_path / "windows.dbde")
    with codec.open_writer(path, rw, rh, frame_hz=50.0, batch_frames=2) as w:   # batches of 2: 5 frames take three
        w.put_window(frames[:5], x=x, y=y, first_index=100)
        w.put_window(frames[5:, y:y + rh, x:x + rw], first_index=105)          # the same window as a sliced view
        with pytest.raises(dv.DbdeError):
            w.put_window(frames[:, :20, :20])                                   # smaller than the writer's frames
    pack = wr.packer(oracle)
    want = np.concatenate([oracle.pack_video_header(3, rh, rw, 50.0)] +
                          [pack(100 + f, host[f, y:y + rh, x:x + rw]) for f in range(8)])
    got = np.fromfile(path, np.uint8)
    assert got.tobytes() == want.tobytes()
    with codec.open_reader(path, batch_frames=3) as r:
        assert (r.W, r.H) == (rw, rh)
        batches = [(imgs.cpu().numpy(), hdrs) for imgs, hdrs in r]
    back = np.concatenate([b for b, _ in batches])
    assert np.array_equal(back, host[:, y:y + rh, x:x + rw])
    assert [h for _, hs in batches for h in hs] == [(2, 100 + f, 0) for f in range(8)]
