"""CPU: dbde_hip_project_registered_plan (host arithmetic) and the argument rules of dbde_hip_project_registered that
need no device: sizes, statistics, pieces, bands, segments against n_cu, instance, workspace; NULL and misaligned
pointers are rejected before anything touches the GPU (a NULL context)."""
import ctypes as C
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


def plans(dv):
    return ((dv.registered_plan, 248, 1), (dv.registered16_plan, 120, 2))


def test_pieces_and_bands(dv):
    for plan, cols, pix in plans(dv):
        for rw in (1, 7, cols - 1, cols, cols + 1, 2 * cols, 2 * cols + 1, 4096):
            for rh in (1, 8, 9, 27, 3072):
                p = plan(4096, 3072, 5, rw, rh)
                assert p["piece_cols"] == cols == 8 * (256 // (8 * pix) - 1)
                assert p["pieces_x"] == -(-rw // cols) and p["bands"] == -(-rh // 8) and p["band_rows"] == 8
                assert p["threads"] == 256 and p["max_frames_per_segment"] == 65536
                assert p["grid"] == p["pieces_x"] * p["bands"] * p["segments"]


def segments_of(n, base, n_cu):
    """project's segment rule: fill about 4 workgroups per CU, at least 32 frames a segment, at most 65,536."""
    target = 4 * max(n_cu, 1)
    seg = 1 if base >= target else -(-target // base)
    seg = min(seg, -(-n // 32))
    seg = max(seg, -(-n // 65536), 1)
    fps = -(-n // seg)
    return (-(-n // fps) if fps else seg), fps


def test_segments_against_n_cu(dv):
    for plan, cols, pix in plans(dv):
        for W, H, rw, rh in ((77, 45, 41, 27), (200, 123, 150, 100), (4096, 3072, 4064, 3040), (512, 512, 480, 480)):
            for n in (0, 1, 31, 33, 67, 70, 1024, 65536, 65537, 200000):
                for n_cu in (1, 64, 256, 304):
                    p = plan(W, H, n, rw, rh, n_cu=n_cu)
                    base = -(-rw // cols) * -(-rh // 8)
                    assert (p["segments"], p["frames_per_segment"]) == segments_of(n, base, n_cu), (W, n, n_cu)
                    assert p["frames_per_segment"] <= 65536
                    P = rw * rh
                    assert p["combine_grid"] == (-(-P // 256) if p["segments"] > 1 else 0)
    assert dv.registered_plan(77, 45, 67, 41, 27, n_cu=256)["segments"] == 3
    assert dv.registered_plan(4096, 3072, 1024, 4064, 3040, n_cu=256)["segments"] == 1


def test_instance_and_workspace(dv):
    r16 = lambda v: (v + 15) // 16 * 16   # noqa: E731
    for plan, cols, pix in plans(dv):
        for mask in range(1, 16):
            p = plan(77, 45, 67, 41, 27, stats=mask, n_cu=256)
            assert p["instance"] == (3 if mask & ~3 == 0 else 12 if mask & ~12 == 0 else 15)
            n = p["segments"] * 41 * 27
            want = ((r16(pix * n) if mask & 1 else 0) + (r16(pix * n) if mask & 2 else 0) + (r16(4 * n) if mask & 4 else 0) +
                    (r16(4 * pix * n) if mask & 8 else 0))
            assert p["segments"] == 3 and p["workspace_bytes"] == want
            assert plan(77, 45, 20, 41, 27, stats=mask)["workspace_bytes"] == 0       # one segment
            # the same workspace as project's for the same statistics and segments
            q = (dv.project_plan if pix == 1 else dv.project16_plan)(77, 45, 67, 0, 0, 41, 27, stats=mask, n_cu=256)
            if q["segments"] == p["segments"]:
                assert q["workspace_bytes"] == p["workspace_bytes"]
        assert plan(77, 45, 5, 41, 27)["lds_bytes"] == 2 * 4 * 8 * 68 * 4 + 2 * 4 * 2 * 32 + 16


def test_index_geometry_is_the_window_decoders(dv):
    for W, H in ((77, 45), (4107, 17), (4096, 3072)):
        p, r = dv.registered_plan(W, H, 9, 9, 9), dv.roi_plan(W, H, 9, 0, 0, 9, 9)
        for k in ("chunks_per_frame", "chunk_tiles", "chunk_pieces", "index_split"):
            assert p[k] == r[k], (W, H, k)


def test_plan_rejects_bad_sizes_and_statistics(dv):
    for plan, _, _ in plans(dv):
        for kw in (dict(rw=0), dict(rw=78), dict(rh=0), dict(rh=46), dict(rw=-1), dict(stats=0), dict(stats=16), dict(n=-1),
                   dict(W=0), dict(H=0)):
            a = dict(W=77, H=45, n=5, rw=41, rh=27, stats=15)
            a.update(kw)
            with pytest.raises(ValueError):
                plan(a["W"], a["H"], a["n"], a["rw"], a["rh"], stats=a["stats"])
        assert plan(77, 45, 5, 77, 45)["pieces_x"] >= 1 and plan(77, 45, 0, 1, 1)["segments"] == 1
    L = dv.lib()
    assert L.dbde_hip_project_registered_plan(77, 45, 5, 41, 27, 15, 256, None) == dv.ERR_ARG


def test_call_rejects_null_context(dv):
    """Without a context nothing can run; the pointer rules themselves (NULL origins, no statistic, NULL count,
    misaligned U64 planes) are exercised with a live context in tests/test_gpu_registered.py."""
    L = dv.lib()
    for fn in (L.dbde_hip_project_registered, L.dbde16_hip_project_registered):
        assert fn(None, 4096, 100, 4096, 77, 45, 1, 41, 27, 4096, 0, 4096, 4096, 4096, 4096, 4096, None, None) == dv.ERR_ARG
