"""CPU: the stand-in transport the multi-rank GPU tests run on (tests/fake_rccl/, reached through DBDE_HIP_RCCL_LIBRARY),
tested by itself before anything is built on it, and the override route of csrc/dbde_rccl.h.

  * it builds, exports exactly the eleven entry points dbde_rccl.h resolves, and needs nothing from the package;
  * transport semantics in host mode (DBDE_FAKE_RCCL_HOST=1: buffers are host memory): 2, 3 and 4 real processes call it
    through ctypes -- all-gather of 2 x U64, broadcast from root 0 and from a non-zero root, grouped sends and receives in
    the shapes dbde_hip_gather_plan and dbde_hip_scatter_plan emit for the world, messages of 0 bytes, 1 byte and several
    mailboxes, two back-to-back rounds, send / receive to self.  What a rank must hold afterwards is numpy slices of the
    senders' inputs, worked out here;
  * a rank whose peer never posts gets an error, naming the peer and the operation, within the configured bound;
  * DBDE_HIP_RCCL_LIBRARY: a fresh process reports the stand-in's version code; a missing file, or a library without the
    entry points, is an error (version 0 and a reason) -- never a quiet fall-back to the real RCCL."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FAKE_DIR = os.path.join(ROOT, "tests", "fake_rccl")
sys.path.insert(0, FAKE_DIR)
FAKE_VERSION = 990077
ENTRY_POINTS = {"ncclGetUniqueId", "ncclCommInitRank", "ncclCommDestroy", "ncclAllGather", "ncclBroadcast", "ncclSend",
                "ncclRecv", "ncclGroupStart", "ncclGroupEnd", "ncclGetErrorString", "ncclGetVersion"}
MAILBOX = 4096


def build_fake_rccl(out_dir):
    """hipcc (for the HIP and RCCL headers and libamdhip64), as test_c_client.py builds its clients."""
    so = os.path.join(str(out_dir), "libdbde_fake_rccl.so")
    if not os.path.exists(so):
        subprocess.run(["/opt/rocm/bin/hipcc", "-O1", "-fPIC", "-shared", "-Wall", os.path.join(FAKE_DIR, "fake_rccl.cpp"),
                        "-o", so + ".tmp", "-Wl,-soname,libdbde_fake_rccl.so",
                        "-Wl,--version-script=" + os.path.join(FAKE_DIR, "exports.map"), "-lrt", "-pthread"],
                       check=True, capture_output=True, text=True)
        os.rename(so + ".tmp", so)
    return so


@pytest.fixture(scope="module")
def fake(tmp_path_factory):
    return build_fake_rccl(tmp_path_factory.mktemp("fake_rccl"))


def test_it_builds_and_exports_exactly_the_eleven_entry_points(fake):
    out = subprocess.run(["nm", "-D", "--defined-only", fake], capture_output=True, text=True, check=True).stdout
    assert {line.split()[-1] for line in out.splitlines() if line.strip()} == ENTRY_POINTS
    # the names csrc/dbde_rccl.h resolves are these eleven
    with open(os.path.join(ROOT, "dbde-video-cpp_amd", "csrc", "dbde_rccl.h")) as f:
        text = f.read()
    assert set(re.findall(r"DBDE_RCCL_SYM\(\w+, (nccl\w+)\)", text)) == ENTRY_POINTS
    dyn = subprocess.run(["readelf", "-d", fake], capture_output=True, text=True, check=True).stdout
    soname = [line for line in dyn.splitlines() if "SONAME" in line]
    assert len(soname) == 1 and "libdbde_fake_rccl.so" in soname[0] and "librccl" not in soname[0]
    assert "dbde_hip" not in dyn, "the stand-in needs nothing from the package"
    und = subprocess.run(["nm", "-D", "--undefined-only", fake], capture_output=True, text=True, check=True).stdout
    assert "dbde_hip" not in und
    hip_calls = {line.split()[-1].split("@")[0] for line in und.splitlines() if line.split()[-1].startswith("hip")}
    assert hip_calls == {"hipStreamSynchronize", "hipMemcpy"}, hip_calls


def play(fake, tmp_path, world, rank_steps, env_extra=None, timeout=60):
    """Starts `world` host-mode ranks on their programs; -> (return codes, [npz per rank], [stderr per rank])."""
    program = {"world": world, "id_file": str(tmp_path / "unique_id"), "ranks": rank_steps}
    path = tmp_path / "program.json"
    path.write_text(json.dumps(program))
    env = dict(os.environ, DBDE_FAKE_RCCL_HOST="1", DBDE_FAKE_RCCL_MAILBOX=str(MAILBOX), DBDE_FAKE_RCCL_TIMEOUT_S="20")
    env.update(env_extra or {})
    procs = [subprocess.Popen([sys.executable, os.path.join(FAKE_DIR, "host_rank.py"), fake, str(path), str(r),
                               str(tmp_path / f"rank{r}.npz")], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for r in range(world)]
    codes, errs = [], []
    try:
        for p in procs:
            _, err = p.communicate(timeout=timeout)
            codes.append(p.returncode)
            errs.append(err)
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.communicate()
    outs = [dict(np.load(tmp_path / f"rank{r}.npz")) if c == 0 else None for r, c in enumerate(codes)]
    return codes, outs, errs


def gather_steps(dv, world, root, sizes, piece):
    steps = []
    for r in range(world):
        ops, total = dv.gather_plan(world, r, root, sizes, piece)
        assert total == sum(sizes)
        group = []
        for peer, kind, seg_off, win_off, nbytes in ops:
            if kind == dv.GATHER_SEND:
                group.append(["send", peer, "data", seg_off, "canvas", 0, nbytes])
            elif kind == dv.GATHER_RECV:
                group.append(["recv", peer, "data", 0, "canvas", win_off, nbytes])
        steps.append({"op": "group", "ops": group})
    return steps


def scatter_steps(dv, world, root, blocks, piece):
    steps = []
    for r in range(world):
        group = []
        for peer, kind, src_off, dst_off, nbytes in dv.scatter_plan(world, r, root, blocks, piece):
            if kind == dv.SCATTER_SEND_BYTES:
                group.append(["send", peer, "data", src_off, "canvas", 0, nbytes])
            elif kind == dv.SCATTER_SEND_OFFSETS:
                group.append(["send", peer, "aux", src_off, "canvas2", 0, nbytes])
            elif kind == dv.SCATTER_RECV_BYTES:
                group.append(["recv", peer, "data", 0, "canvas", dst_off, nbytes])
            elif kind == dv.SCATTER_RECV_OFFSETS:
                group.append(["recv", peer, "aux", 0, "canvas2", dst_off, nbytes])
        steps.append({"op": "group", "ops": group})
    return steps


def expected_canvases(world, group_per_rank):
    """What every rank must hold after a group step: the k-th receive of r from p meets the k-th send of p to r."""
    from host_rank import DATA_BYTES, inputs
    want = []
    for r in range(world):
        canv = {"canvas": np.full(DATA_BYTES, 0xEE, np.uint8), "canvas2": np.full(DATA_BYTES, 0xEE, np.uint8)}
        for p in range(world):
            sends = [o for o in group_per_rank[p]["ops"] if o[0] == "send" and o[1] == r]
            recvs = [o for o in group_per_rank[r]["ops"] if o[0] == "recv" and o[1] == p]
            assert len(sends) == len(recvs)
            src = dict(zip(("data", "aux"), inputs(p)))
            for (_, _, s, s_off, _, _, n), (_, _, _, _, d, d_off, m) in zip(sends, recvs):
                assert n == m
                canv[d][d_off:d_off + m] = src[s][s_off:s_off + n]
        want.append(canv)
    return want


@pytest.mark.parametrize("world", [2, 3, 4])
def test_transport_semantics_between_real_processes(fake, tmp_path, world):
    import dbde_video_cpp_amd as dv
    last = world - 1
    big = 3 * MAILBOX + 5
    gather_sizes = {2: [2 * MAILBOX + 1, 1], 3: [1, 0, 9000], 4: [MAILBOX, 0, 1, 3 * MAILBOX + 1]}[world]
    rng = np.random.default_rng(40 + world)
    frame_bytes = rng.integers(34, 1500, {2: 7, 3: 2, 4: 25}[world])          # world 3: fewer frames than ranks
    offs = [int(x) for x in np.concatenate([[0], np.cumsum(frame_bytes)])[:-1]]
    blocks = dv.scatter_blocks(world, offs, int(frame_bytes.sum()))
    per_step = [
        [{"op": "allgather", "words": [7 * r + 1, 1000 + r]} for r in range(world)],
        [{"op": "broadcast", "root": 0, "words": [100 + k if r == 0 else 0 for k in range(4 * world)]} for r in range(world)],
        [{"op": "broadcast", "root": last, "words": [900 + k if r == last else 0 for k in range(4 * world)]} for r in range(world)],
        # the two pipelined slots: two rounds back to back, pieces larger than the mailbox, then one whole message
        gather_steps(dv, world, 0, gather_sizes, MAILBOX + 904),
        gather_steps(dv, world, last, gather_sizes[::-1], 0),
        scatter_steps(dv, world, 0, blocks, 0),
        scatter_steps(dv, world, last, blocks, 777),
        # a ring of 0 bytes, 1 byte and several mailboxes, with a send / receive to self in the same group
        [{"op": "group", "ops": [["send", (r + 1) % world, "data", 0, "canvas", 0, 0], ["recv", (r - 1) % world, "data", 0, "canvas", 3, 0],
                                 ["send", r, "aux", 11, "canvas2", 0, 2 * MAILBOX + 3], ["send", (r + 1) % world, "data", 5, "canvas", 0, 1],
                                 ["recv", (r - 1) % world, "data", 0, "canvas", 9, 1], ["recv", r, "aux", 0, "canvas2", 100, 2 * MAILBOX + 3],
                                 ["send", (r + 1) % world, "data", 17, "canvas", 0, big], ["recv", (r - 1) % world, "data", 0, "canvas", 64, big],
                                 ["send", r, "data", 0, "canvas2", 0, 0], ["recv", r, "data", 0, "canvas2", 0, 0]]} for r in range(world)],
    ]
    rank_steps = [[step[r] for step in per_step] for r in range(world)]
    codes, outs, errs = play(fake, tmp_path, world, rank_steps)
    assert codes == [0] * world, errs
    for r in range(world):
        o = outs[r]
        assert o["s0_out"].tolist() == [x for q in range(world) for x in (7 * q + 1, 1000 + q)]
        assert o["s1_out"].tolist() == [100 + k for k in range(4 * world)]
        assert o["s2_out"].tolist() == [900 + k for k in range(4 * world)]
    moved = 0
    for k in range(3, len(per_step)):
        want = expected_canvases(world, per_step[k])
        for r in range(world):
            for name in ("canvas", "canvas2"):
                assert np.array_equal(outs[r][f"s{k}_{name}"], want[r][name]), (k, r, name)
                moved += int((want[r][name] != 0xEE).sum())
    assert moved > 10 * MAILBOX          # the expectation is not vacuous
    # the gather's root holds the ranks' segments back to back, a scatter's peer its block and its frame offsets
    from host_rank import inputs
    at = 0
    for r, n in enumerate(gather_sizes):
        if r != 0:
            assert np.array_equal(outs[0]["s3_canvas"][at:at + n], inputs(r)[0][:n])
        at += n
    for r in range(world - 1):
        f0, nf, b0, nb = blocks[r]
        assert np.array_equal(outs[r]["s6_canvas"][:nb], inputs(last)[0][b0:b0 + nb])
        assert np.array_equal(outs[r]["s6_canvas2"][:8 * nf], inputs(last)[1][8 * f0:8 * (f0 + nf)])


def test_a_peer_that_never_posts_is_an_error_within_the_bound(fake, tmp_path):
    """Bound 2 s: rank 1 joins the communicator and leaves; rank 0's receive from it must come back with ncclSystemError."""
    codes, outs, errs = play(fake, tmp_path, 2, [[{"op": "recv_alone", "peer": 1, "bytes": 100}], [{"op": "leave"}]],
                             env_extra={"DBDE_FAKE_RCCL_TIMEOUT_S": "2"}, timeout=30)
    assert codes == [0, 0], errs
    o = outs[0]
    assert int(o["s0_code"]) == 2                                  # ncclSystemError
    assert 2.0 <= float(o["s0_seconds"]) < 4.0
    text = str(o["s0_text"])
    assert "recv" in text and "from rank 1" in text and "100 bytes" in text and "rank 0 waited" in text, text
    assert (o["s0_out"] == 0xEE).all()


def test_a_size_mismatch_between_the_two_ends_is_an_error_not_a_hang(fake, tmp_path):
    steps = [[{"op": "group", "ops": [["send", 1, "data", 0, "canvas", 0, 10]]}],
             [{"op": "group", "ops": [["recv", 0, "data", 0, "canvas", 0, 11]]}]]
    codes, outs, errs = play(fake, tmp_path, 2, steps, env_extra={"DBDE_FAKE_RCCL_TIMEOUT_S": "2"}, timeout=30)
    assert codes[1] != 0 and "disagree" in errs[1], errs


OVERRIDE_CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
import dbde_video_cpp_amd as dv
L = dv.lib()
print(L.dbde_hip_gather_rccl_version())
print((L.dbde_hip_gather_error(None) or b"").decode())
"""


def test_override_route_in_a_fresh_process(fake, tmp_path):
    cases = {"fake": fake, "missing": str(tmp_path / "no_such_librccl.so"), "not_rccl": "libm.so.6"}
    procs = {k: subprocess.Popen([sys.executable, "-c", OVERRIDE_CHILD, ROOT], env=dict(os.environ, DBDE_HIP_RCCL_LIBRARY=v),
                                 stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for k, v in cases.items()}
    got = {}
    for k, p in procs.items():
        out, err = p.communicate(timeout=120)
        assert p.returncode == 0, (k, err[-1500:])
        got[k] = out.strip().splitlines()
    assert got["fake"][0] == str(FAKE_VERSION)
    assert got["missing"][0] == "0" and "DBDE_HIP_RCCL_LIBRARY" in got["missing"][1] and "cannot be opened" in got["missing"][1]
    assert got["not_rccl"][0] == "0" and "lacks ncclGetUniqueId" in got["not_rccl"][1]


def test_nothing_in_the_product_names_the_stand_in_or_sets_the_variable():
    """The repository's own sources: the files at its root and everything under its source directories."""
    paths = [os.path.join(ROOT, name) for name in os.listdir(ROOT) if os.path.isfile(os.path.join(ROOT, name))]
    for top in ("dbde-video-cpp_amd", "include", "oracle", "profiles", "tests"):
        for base, dirs, files in os.walk(os.path.join(ROOT, top)):
            dirs[:] = [d for d in dirs if d not in ("__pycache__", "_ref")]
            paths += [os.path.join(base, name) for name in files]
    hits = []
    for path in paths:
        rel = os.path.relpath(path, ROOT)
        if path.endswith((".so", ".npz", ".pyc")) or os.path.getsize(path) > (1 << 20):
            continue
        with open(path, errors="ignore") as f:
            text = f.read()
        if "DBDE_HIP_RCCL_LIBRARY" in text:
            hits.append(rel)
        if "fake_rccl" in text:
            assert not rel.startswith(("dbde-video-cpp_amd" + os.sep, "profiles" + os.sep)) and rel != "bench.py", rel
    allowed = (os.path.join("dbde-video-cpp_amd", "csrc", "dbde_rccl.h"), os.path.join("include", "dbde_hip.h"), "INTEGRATION.md")
    assert hits and all(h in allowed or h.startswith("tests" + os.sep) for h in hits), hits
