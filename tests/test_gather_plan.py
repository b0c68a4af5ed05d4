"""CPU: the host logic of the native gather (dbde_hip_gather_plan, csrc/dbde_gather.cpp).  Both ends of every
transfer derive their send / receive lists from the same all-gathered byte counts; RCCL hangs if they disagree, so
the plan is exposed through the C-ABI and checked here by playing every rank of worlds of 1..8 against the root:
each sender's messages must meet, in order and byte for byte, the root's receives from that peer, and the pieces
must tile the gathered stream (ranks' segments in rank order, README.md:12-23) exactly once."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_every_send_meets_its_receive_and_the_window_is_tiled():
    import dbde_video_cpp_amd as dv
    rng = np.random.default_rng(11)
    for world in range(1, 9):
        for root in sorted({0, world - 1, world // 2}):
            for piece in (0, 1 << 20, 4096, 7):
                sizes = [int(x) for x in rng.integers(0, 3 * max(piece, 1000), world)]
                sizes[int(rng.integers(world))] = 0                      # a rank with nothing to send
                if piece:
                    sizes[int(rng.integers(world))] = 5 * piece           # exact multiple of the piece size
                plans = [dv.gather_plan(world, r, root, sizes, piece) for r in range(world)]
                assert all(t == sum(sizes) for _, t in plans)
                root_ops, total = plans[root]
                disp = np.concatenate([[0], np.cumsum(sizes)])
                covered = np.zeros(total, np.uint8)
                for r in range(world):
                    ops = plans[r][0]
                    if r == root:
                        own = [o for o in ops if o[1] == dv.GATHER_OWN]
                        assert len(own) == (1 if sizes[r] else 0)
                        for peer, kind, so, wo, b in own:
                            assert (peer, so, wo, b) == (root, 0, disp[r], sizes[r])
                            covered[wo:wo + b] += 1
                        continue
                    sends = ops
                    assert all(k == dv.GATHER_SEND and p == root for p, k, _, _, _ in sends)
                    recvs = [o for o in root_ops if o[1] == dv.GATHER_RECV and o[0] == r]
                    assert len(sends) == len(recvs)
                    at = 0
                    for (_, _, so, wo, b), (_, _, _, rwo, rb) in zip(sends, recvs):
                        assert b == rb and wo == rwo and so == at and wo == disp[r] + at
                        assert 0 < b <= (piece or 1 << 30)
                        covered[wo:wo + b] += 1
                        at += b
                    assert at == sizes[r]
                assert (covered == 1).all()
                # a non-root rank never sees a receive; the root never sends
                assert all(k != dv.GATHER_SEND for _, k, _, _, _ in root_ops)


def test_an_undeclared_window_with_peers_is_one_verdict_for_every_rank():
    """A root that never declared its window (dbde_hip_gather_set_window) used to send "no limit" (~0): the shared check
    passed everywhere, and the root's own window_bytes test then failed on the root ALONE, after its peers had posted
    their sends.  With peers, dbde_hip_gather_begin now sends "none" (capacity 0) for an undeclared window: the verdict
    is a function of the exchanged pairs alone, so a total that overflows is ERR_CAPACITY on every rank and nobody posts."""
    import dbde_video_cpp_amd as dv
    NO_LIMIT = (1 << 64) - 1
    for world in range(2, 9):
        for root in sorted({0, world - 1, world // 2}):
            sizes = [1000 + 7 * r for r in range(world)]
            undeclared = [0] * world                       # what travels now: the root's word is "none"
            assert dv.gather_check(world, root, sizes, undeclared) == (dv.ERR_CAPACITY, sum(sizes))
            one_byte = [0] * world
            one_byte[(root + 1) % world] = 1               # any byte at all overflows a window nobody declared
            assert dv.gather_check(world, root, one_byte, undeclared) == (dv.ERR_CAPACITY, 1)
            assert dv.gather_check(world, root, [0] * world, undeclared) == (dv.OK, 0)      # empty rounds still pass
            # the verdict has no rank argument: what the root alone knows (its window_bytes) cannot enter it, which is
            # why "no limit" must never travel -- it passes here whatever the total, and only the root could object
            old = [0] * world
            old[root] = NO_LIMIT
            assert dv.gather_check(world, root, sizes, old) == (dv.OK, sum(sizes))
            # the source holds the rule: with peers an undeclared window is sent as 0, never as the default ~0
    src = open(os.path.join(ROOT, "dbde-video-cpp_amd", "csrc", "dbde_gather.cpp")).read()
    assert "g->nranks > 1 && !g->window_declared) ? 0ull" in src


def test_plan_rejects_bad_arguments():
    import ctypes as C
    import dbde_video_cpp_amd as dv
    L = dv.lib()
    one = (C.c_uint64 * 1)(5)
    assert L.dbde_hip_gather_plan(0, 0, 0, one, 0, None, 0, None) < 0
    assert L.dbde_hip_gather_plan(1, 1, 0, one, 0, None, 0, None) < 0
    assert L.dbde_hip_gather_plan(1, 0, 2, one, 0, None, 0, None) < 0
    assert L.dbde_hip_gather_plan(1, 0, 0, None, 0, None, 0, None) < 0
    assert L.dbde_hip_gather_plan(1, 0, 0, one, 0, None, 0, None) == 1
