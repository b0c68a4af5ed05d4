"""GPU: binning.bin_file -- a .dbde file binned in time, group_frames frames to one (Codec.project_groups).

The source is written by the HIP writer; the binned file is read back by the HIP reader and compared with the numpy
binning of the decoded source, for pieces small enough that a group straddles two of them.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = 0xDBDE2016
W, H, N, G, HZ, FIRST = 72, 50, 23, 4, 1000.0, 40


@pytest.fixture(scope="module")
def dv():
    import dbde_video_cpp_amd as m
    return m


@pytest.fixture(scope="module")
def codec(dv):
    c = dv.Codec(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def source(codec, tmp_path_factory):
    """23 frames of 72x50 with their own indices and elapsed times; the decoded source, read back with the reader."""
    import torch
    path = str(tmp_path_factory.mktemp("binning") / "src.dbde")
    imgs = codec.synth_frames("mixed", SEED, 0, N, W, H)
    idx = torch.arange(FIRST, FIRST + N, dtype=torch.int64, device="cuda") * 3
    el = torch.arange(N, dtype=torch.int64, device="cuda") * 1_000_000 + 17
    with codec.open_writer(path, W, H, frame_hz=HZ, batch_frames=5) as w:
        w.put(imgs, N, indices=idx, elapsed_ns=el)
    decoded, headers = [], []
    with codec.open_reader(path, batch_frames=7) as r:
        for im, hd in r:
            decoded.append(im.cpu().numpy())
            headers += hd
    decoded = np.concatenate(decoded)
    assert decoded.shape == (N, H, W) and np.array_equal(decoded, imgs.cpu().numpy())
    assert headers == [(2, 3 * (FIRST + f), 1_000_000 * f + 17) for f in range(N)]
    return path, decoded, headers


def numpy_binning(frames, g, stat):
    out = []
    for lo in range(0, len(frames), g):
        w = frames[lo:lo + g].astype(np.int64)
        c = w.shape[0]
        out.append({"mean": (2 * w.sum(0) + c) // (2 * c), "max": w.max(0), "min": w.min(0)}[stat])
    return np.stack(out).astype(np.uint8)


@pytest.mark.parametrize("stat", ["mean", "max", "min"])
def test_bin_file_matches_the_numpy_binning(dv, codec, source, tmp_path, stat):
    from importlib import import_module
    binning = import_module("dbde_video_cpp_amd.binning")
    src, decoded, headers = source
    want = numpy_binning(decoded, G, stat)
    assert want.shape[0] == 6
    src_bytes = np.fromfile(src, np.uint8)
    frame_bytes = (len(src_bytes) - 28) // N
    files = []
    for batch_bytes in (1 << 20, 5 * frame_bytes // 2, 777):   # one piece; groups straddling pieces; pieces cutting frames
        dst = str(tmp_path / f"{stat}_{batch_bytes}.dbde")
        written, rejected, size = binning.bin_file(codec, src, dst, G, stat=stat, batch_bytes=batch_bytes)
        data = np.fromfile(dst, np.uint8)
        assert (written, rejected, size) == (6, 0, len(data))
        files.append(data.tobytes())
        with codec.open_reader(dst, batch_frames=4) as r:
            assert r.video_header == (3, H, W, HZ / G)
            got, hdrs = [], []
            for im, hd in r:
                got.append(im.cpu().numpy())
                hdrs += hd
        assert np.array_equal(np.concatenate(got), want), (stat, batch_bytes)
        assert hdrs == [headers[k * G] for k in range(6)]   # the groups' first frames, the last group of 3 included
    assert files[1] == files[0] and files[2] == files[0]


def test_bin_file_leaves_out_groups_without_an_accepted_frame(dv, codec, source, tmp_path):
    """Frames 4..7 (group 1) and frame 8 damaged: group 1 is left out, group 2 starts at its first accepted frame."""
    from importlib import import_module
    binning = import_module("dbde_video_cpp_amd.binning")
    src, decoded, headers = source
    data = np.fromfile(src, np.uint8).copy()
    T = dv.tiles(W, H)
    offs, at = [], 28
    for f in range(N):
        offs.append(at)
        at += 32 + 2 * T + 8 * int.from_bytes(data[at + 28 + 2 * T: at + 32 + 2 * T].tobytes(), "little")
    assert at == len(data)
    for f in (4, 5, 6, 7, 8):
        data[offs[f] + 24 + 3] = 9   # a depth byte > 8 with n64 unchanged: rejected, same length
    bad, dst = str(tmp_path / "bad.dbde"), str(tmp_path / "binned.dbde")
    data.tofile(bad)
    written, rejected, size = binning.bin_file(codec, bad, dst, G, stat="max", batch_bytes=3000)
    assert (written, rejected) == (5, 5)
    with codec.open_reader(dst, batch_frames=8) as r:
        got, hdrs = r.next()
    keep = [f for f in range(N) if f not in (4, 5, 6, 7, 8)]
    want = [decoded[[f for f in keep if f // G == k]].max(0) for k in (0, 2, 3, 4, 5)]
    assert np.array_equal(got.cpu().numpy(), np.stack(want))
    assert hdrs == [headers[0], headers[9], headers[12], headers[16], headers[20]]
