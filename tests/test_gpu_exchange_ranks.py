"""GPU, 2-4 REAL ranks on one MI355X: the multi-rank half of the native exchange (csrc/dbde_gather.cpp, csrc/dbde_scatter.cpp)
and streaming.RoundTripStream(gather="native") at world > 1.  RCCL refuses two ranks on one device, so every rank is a
fresh process (tests/exchange_rank.py) whose DBDE_HIP_RCCL_LIBRARY names a stand-in transport (tests/fake_rccl/, itself
tested on the CPU by tests/test_fake_rccl.py): the library's own SEND / RECV-at-a-displacement / OWN-at-a-displacement
branches, SEND_/RECV_BYTES and _OFFSETS, the in-place rebase of received offsets and the shared capacity verdicts run
with real peers.  This checks bytes and verdicts; it is NOT a measurement, nothing crosses xGMI, and RCCL itself still has
not carried rank-to-rank traffic (the one-rank tests keep using the real RCCL).

The ranks judge nothing: each writes one JSON line per step (SHA-256 of what it holds, sizes, tables, return codes, guard
verdicts) and this module compares them with what it works out from the oracle -- the frames of every case packed by
oracle_ffi.Oracle, whose 4096x3072 frames r * 1024 and r * 1024 + 3 are first held to the reference-made SHA-256 of
tests/golden/manifest.json.  Nothing is compared with another run of the code under test.  All comparisons are exact.

Two defects this found by reading, fixed with it: a root that never declared its window let the overflow verdict fall on
the root alone (its peers' sends stayed unmatched), and the root's frame capacity did not count in the scatter's verdict
although the rebased offsets of its block are written to its array.  Against the library before the fix, steps
"gather_undeclared_window" and "scatter_root_frames_one_short" fail (observed), and pass after it.

Caps, not measurements: the stand-in's wait bound is 60 s, a world's overall limit 300 s (the largest the subprocess tests
use, test_c_client.py); a world takes 2.6 s (2 ranks) to 2.9 s (4 ranks) on an MI355X, start-up included."""
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import exchange_rank as xr
from test_fake_rccl import FAKE_VERSION, build_fake_rccl

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAIT_BOUND_S, WORLD_LIMIT_S = 60, 300
MODES = {"noise8": 0, "mixed": 1, "flat": 2, "smooth": 3}
OK, ERR_CAPACITY = 0, -3


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.fixture(scope="module")
def fake(tmp_path_factory):
    return build_fake_rccl(tmp_path_factory.mktemp("fake_rccl"))


@pytest.fixture(scope="module")
def frames(oracle):
    """(mode, W, H, f) -> (image, packed frame) by the oracle, computed once for all worlds and left unchanged."""
    cache = {}

    def get(mode, W, H, f):
        key = (mode, W, H, f)
        if key not in cache:
            img = oracle.synth_frame(MODES[mode], xr.SEED, f, W, H)
            packed = oracle.pack_frame(f, img, W, H)
            img.setflags(write=False)
            packed.setflags(write=False)
            cache[key] = (img, packed)
        return cache[key]
    return get


def cat(parts, dtype=np.uint8):
    return np.concatenate([np.asarray(p, dtype).reshape(-1) for p in parts]) if parts else np.zeros(0, dtype)


def run_world(fake, tmp_path, world):
    """Starts the ranks (fresh processes, device 0, at most 4 + this one with the GPU open) under one overall limit; on its
    expiry or on any exit status != 0 the others are killed and the test fails.  -> ([lines per rank], seconds)."""
    env = dict(os.environ, DBDE_HIP_RCCL_LIBRARY=fake, DBDE_FAKE_RCCL_TIMEOUT_S=str(WAIT_BOUND_S))
    env.pop("DBDE_FAKE_RCCL_HOST", None)
    id_file = str(tmp_path / "unique_id")
    t0 = time.monotonic()
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "exchange_rank.py"), str(world), str(r), id_file,
                               str(tmp_path / f"rank{r}.jsonl")], env=env, stdout=subprocess.DEVNULL,
                              stderr=open(tmp_path / f"rank{r}.err", "w")) for r in range(world)]
    failure = None
    try:
        pending = list(range(world))
        while pending and failure is None:
            r = pending[0]
            try:
                status = procs[r].wait(timeout=0.25)
            except subprocess.TimeoutExpired:
                status = None
                pending.append(pending.pop(0))
            if status is not None:
                pending.remove(r)
                if status != 0:
                    failure = f"rank {r} of {world} left with status {status}"
            if failure is None and time.monotonic() - t0 > WORLD_LIMIT_S:
                failure = f"world {world} exceeded {WORLD_LIMIT_S} s"
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
            p.wait()
    seconds = time.monotonic() - t0
    if failure:
        tails = {r: open(tmp_path / f"rank{r}.err").read()[-1500:] for r in range(world)}
        steps = {r: [json.loads(x)["step"] for x in open(tmp_path / f"rank{r}.jsonl")][-3:] if os.path.exists(tmp_path / f"rank{r}.jsonl") else None
                 for r in range(world)}
        pytest.fail(f"{failure}; last steps {steps}; stderr {tails}")
    return [[json.loads(x) for x in open(tmp_path / f"rank{r}.jsonl")] for r in range(world)], seconds


# ---- what the oracle says every rank must report ------------------------------------------------------------------------

def expect_gather(frames, world, name, root, in_place):
    W, H, mode, _, _ = xr.GATHER_CASES[name]
    blocks = [xr.gather_block(name, r, world)[:2] for r in range(world)]
    segs = [cat([frames(mode, W, H, f)[1] for f in range(lo, lo + nf)]) for lo, nf in blocks]
    sizes = [len(s) for s in segs]
    want = []
    for r in range(world):
        f = dict(case=name, root=root, rc=OK, sizes=sizes)
        if r == root:
            f.update(window_sha=sha(cat(segs)), guard_before=True, guard_behind=True)
        if not (in_place and r == root):
            f.update(segment_sha=sha(segs[r]), segment_guard_before=True, segment_guard_behind=True)   # a peer's segment: untouched
        want.append(f)
    return want


def expect_scatter(frames, world, name, root, sizes_of_gather=None):
    W, H, mode, n, cut, _ = xr.SCATTER_CASES[name]
    packed = [frames(mode, W, H, f)[1] for f in range(n)]
    offs = np.concatenate([[0], np.cumsum([len(p) for p in packed])]).astype(np.int64)
    nbytes = xr.scatter_extent(int(offs[-1]), cut)
    stream = cat(packed)[:nbytes]
    count = int(sum(1 for f in range(n) if offs[f + 1] <= nbytes))           # the scanner counts whole frames
    want, table = [], []
    for r in range(world):
        lo, hi = count * r // world, count * (r + 1) // world
        b0 = int(offs[lo]) if lo < count else nbytes
        b1 = int(offs[hi]) if hi < count else nbytes
        table.append([lo, hi - lo, b0, b1 - b0])
    if sizes_of_gather is not None:
        assert [t[3] for t in table] == sizes_of_gather and [t[1] for t in table] == [xr.gather_block(name, r, world)[1] for r in range(world)]
    for r in range(world):
        lo, nf, b0, nb = table[r]
        f = dict(case=name, root=root, rc=OK, mine=table[r], table=table, offsets=[int(offs[k]) - b0 for k in range(lo, lo + nf)],
                 offsets_guard=True, block_sha=sha(stream[b0:b0 + nb]), segment_guard=True)
        if nf:
            f.update(images_sha=sha(cat([frames(mode, W, H, k)[0] for k in range(lo, lo + nf)])), headers=[[2, k, 0] for k in range(lo, lo + nf)])
        want.append(f)
    return want


def refused_gather(world, root=0):
    return [dict(case=xr.VERDICT_CASE, root=root, rc=ERR_CAPACITY, **({"window_untouched": True} if r == root else {})) for r in range(world)]


def refused_scatter(world):
    return [dict(case=xr.VERDICT_CASE, root=0, rc=ERR_CAPACITY, segment_untouched=True, offsets_untouched=True) for _ in range(world)]


def expect_stream(frames, world):
    W, H, mode, N, B, _ = xr.STREAM
    blocks = [xr.block(N, r, world) for r in range(world)]
    rounds = max(-(-(hi - lo) // B) for lo, hi in blocks)
    assert len({-(-(hi - lo) // B) for lo, hi in blocks}) > 1, "the rank blocks must differ in their number of batches"
    size = lambda f: len(frames(mode, W, H, f)[1])
    batch = lambda r, k: range(min(blocks[r][0] + k * B, blocks[r][1]), min(blocks[r][0] + (k + 1) * B, blocks[r][1]))
    want = []
    for r, (lo, hi) in enumerate(blocks):
        nb = -(-(hi - lo) // B)
        f = dict(frames=hi - lo, batches=nb, rounds=rounds, mismatches=0, packed_bytes=sum(size(k) for k in range(lo, hi)),
                 gathered_bytes=sum(size(k) for k in range(N)),
                 frame_bytes={str(k): [size(x) for x in batch(r, k)] for k in range(nb)},
                 frame_offsets={str(k): [int(x) for x in np.concatenate([[0], np.cumsum([size(x) for x in batch(r, k)])])[:-1]] for k in range(nb)},
                 snapshots=[])
        if r == 0:       # every gathered batch: that batch of every rank, in rank order
            for k in range(rounds):
                whole = cat([frames(mode, W, H, x)[1] for q in range(world) for x in batch(q, k)])
                f["snapshots"].append([len(whole), sha(whole)])
        want.append(f)
    return want


def expected_lines(frames, world):
    """[(step, [fields per rank])] in the order exchange_rank.py walks."""
    last = world - 1
    steps = []
    for name in xr.GATHER_ROOT0:
        steps.append(("gather", expect_gather(frames, world, name, 0, in_place=True)))
    for name in xr.GATHER_LAST:
        steps.append(("gather", expect_gather(frames, world, name, last, in_place=False)))
    for name in xr.SCATTER_ROOT0:
        steps.append(("scatter", expect_scatter(frames, world, name, 0)))
    for name in xr.SCATTER_LAST:
        steps.append(("scatter", expect_scatter(frames, world, name, last)))
    v = xr.VERDICT_CASE
    gathered_sizes = expect_gather(frames, world, v, 0, True)[0]["sizes"]
    steps.append(("gather_then_scatter", expect_scatter(frames, world, v, 0, sizes_of_gather=gathered_sizes)))
    steps.append(("gather_window_one_short", refused_gather(world)))
    steps.append(("gather_after_refusal", expect_gather(frames, world, v, 0, in_place=False)))
    steps.append(("scatter_segment_one_short", refused_scatter(world)))
    steps.append(("scatter_frames_one_short", refused_scatter(world)))
    steps.append(("scatter_after_refusal", expect_scatter(frames, world, v, 0)))
    steps.append(("scatter_root_frames_one_short", refused_scatter(world)))
    steps.append(("scatter_after_root_refusal", expect_scatter(frames, world, v, 0)))
    steps.append(("gather_undeclared_window", refused_gather(world)))
    steps.append(("gather_after_declaring", expect_gather(frames, world, v, 0, in_place=False)))
    steps.append(("stream", expect_stream(frames, world)))
    return steps


def test_the_oracles_rank_frames_are_the_references(frames, golden):
    """Anchor of the 4096x3072 case: the reference-made SHA-256 of every rank's frames r * 1024 and r * 1024 + 3."""
    manifest, _ = golden
    checked = 0
    for e in manifest["big"]:
        if e["mode"] != "noise8" or e["name"] not in ("cfg2_4096x3072", "cfg2_rank_frames") or e["frame"] // xr.RANK_STRIDE >= 4:
            continue
        img, packed = frames("noise8", e["W"], e["H"], e["frame"])
        assert e["frame"] % xr.RANK_STRIDE < xr.RANK_FRAMES
        assert sha(img) == e["image_sha"] and len(packed) == e["packed_bytes"] and sha(packed) == e["packed_sha"], e["frame"]
        checked += 1
    assert checked == 8          # ranks 0-3, two frames each: all inside the gathered case


@pytest.mark.parametrize("world", [2, 3, 4])
def test_real_ranks_gather_scatter_and_stream(fake, frames, tmp_path, world):
    lines, seconds = run_world(fake, tmp_path, world)
    print(f"world {world}: {seconds:.1f} s")
    assert seconds < WORLD_LIMIT_S / 3, "shrink the frame counts rather than raise the limit"
    want = expected_lines(frames, world)
    for r in range(world):
        got = lines[r]
        assert got[0]["step"] == "hello" and (got[0]["world"], got[0]["rank"]) == (world, r)
        assert got[0]["rccl_version"] == FAKE_VERSION, "the ranks must run on the stand-in, not on RCCL"
        assert got[-1]["step"] == "done"
        assert [g["step"] for g in got[1:-1]] == [step for step, _ in want], r
        for g, (step, fields) in zip(got[1:-1], want):
            g = dict(g)
            assert g.pop("step") == step
            error = g.pop("error", None)
            if fields[r].get("rc", OK) != OK:
                assert error and ("do not fit" in error or "does not fit" in error), (step, r, error)
            assert g == fields[r], (world, r, step, g.get("case"), {k: (g.get(k), v) for k, v in fields[r].items() if g.get(k) != v})
