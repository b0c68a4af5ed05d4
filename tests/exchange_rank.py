"""One rank of the multi-rank exchange tests (tests/test_gpu_exchange_ranks.py) -- infrastructure like crafted.py, not a
test module.  RCCL refuses two ranks on one device, so the parent starts `world` of these as fresh processes on device 0
with DBDE_HIP_RCCL_LIBRARY naming the stand-in transport (tests/fake_rccl/): real peers then drive the branches of
csrc/dbde_gather.cpp and csrc/dbde_scatter.cpp that one rank never reaches (SEND, RECV at a displacement, the root's own
segment at a non-zero displacement, SEND_/RECV_BYTES and _OFFSETS, the in-place rebase of received offsets) and
streaming.RoundTripStream(gather="native") with unequal rank blocks.  It checks bytes and verdicts, never time.

    python exchange_rank.py <world> <rank> <unique-id file> <out.jsonl>

Every rank walks the same fixed list of scenarios (the calls are collective) and writes one JSON line per step: SHA-256 of
what it holds, sizes, block tables, return codes, guard-byte verdicts.  It judges nothing itself: the parent compares
the lines with what it works out from the oracle.  The cases below are the contract between the two."""
import hashlib
import json
import os
import re
import sys
import time

SEED = 0xDBDE2016
GUARD, LEAD = 64, 32

# rank_frames: as bench.py --gpus N shards the headline shape, rank r holds frames r * 1024 .. (here the first RANK_FRAMES of
# them: tests/golden/manifest.json has the reference's SHA-256 of frames r * 1024 and r * 1024 + 3 of every rank)
RANK_FRAMES, RANK_STRIDE = 4, 1024
# the gather's batches: (W, H, mode, frames in the whole world, max_message_bytes).  n not divisible by 2, 3 or 4; fewer
# frames than ranks (empty blocks); none at all.  Small odd pieces make a segment travel as several messages.
GATHER_CASES = {
    "odd_1921x1081": (1921, 1081, "mixed", 7, 333331),
    "many_64x64": (64, 64, "mixed", 203, 4099),
    "rank_frames_4096x3072": (4096, 3072, "noise8", RANK_FRAMES, 1 << 30),
    "fewer_frames_than_ranks": (64, 64, "mixed", 1, 4099),
    "no_frames": (64, 64, "mixed", 0, 4099),
}
GATHER_ROOT0 = ["odd_1921x1081", "many_64x64", "rank_frames_4096x3072", "fewer_frames_than_ranks", "no_frames"]
GATHER_LAST = ["many_64x64", "odd_1921x1081"]          # root = world - 1: its own segment lands at a non-zero displacement
# the scatter's streams: (W, H, mode, frames encoded, bytes kept back from the end (None: all but 10 bytes), max_message_bytes)
SCATTER_CASES = {
    "odd_1921x1081": (1921, 1081, "mixed", 7, 0, 333331),
    "many_64x64": (64, 64, "mixed", 203, 0, 4099),
    "truncated_tail": (200, 123, "mixed", 9, 3, 1 << 30),
    "empty_stream": (200, 123, "mixed", 9, None, 1 << 30),
    "fewer_frames_than_ranks": (64, 64, "mixed", 1, 0, 4099),
}
SCATTER_ROOT0 = ["odd_1921x1081", "truncated_tail", "empty_stream", "fewer_frames_than_ranks", "many_64x64"]
SCATTER_LAST = ["many_64x64", "truncated_tail"]
VERDICT_CASE = "many_64x64"                             # the batch / stream of the capacity scenarios
STREAM = (200, 123, "mixed", 37, 3, 10007)              # RoundTripStream: W, H, mode, frames, batch, max_message_bytes (37 frames in batches of 3: the ranks of worlds 2, 3 and 4 differ in their number of batches)


def block(n, rank, world):
    return n * rank // world, n * (rank + 1) // world


def gather_block(name, rank, world):
    """-> (first frame, frames) of `rank` in a gather case, and the frames of the whole world."""
    n = GATHER_CASES[name][3]
    if name.startswith("rank_frames"):
        return RANK_STRIDE * rank, n, n * world
    lo, hi = block(n, rank, world)
    return lo, hi - lo, n


def scatter_extent(total, cut):
    return 10 if cut is None else total - cut


def main():
    world, rank, id_file, out_path = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import numpy as np
    import torch
    import dbde_video_cpp_amd as dv
    from dbde_video_cpp_amd.streaming import RoundTripStream
    out = open(out_path, "w")
    last = world - 1

    def emit(step, **fields):
        out.write(json.dumps(dict(step=step, **fields)) + "\n")
        out.flush()

    def sha(t):
        return hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()

    def all_are(t, value):
        return bool((t == value).all().item())

    def code(fn):
        """-> (return code, result): DBDE_HIP_OK, or the code of the DbdeError the call raised."""
        try:
            return dv.OK, fn()
        except dv.DbdeError as e:
            return int(re.search(r"failed \((-?\d+)\)", str(e)).group(1)), str(e)

    def pipeline(n, begin, post):
        """Both slots in flight: the exchange of batch k + 1 is begun before the transfers of batch k are posted."""
        for k in range(n):
            begin(k, k % 2)
            if k >= 1:
                post(k - 1, (k - 1) % 2)
        if n:
            post(n - 1, (n - 1) % 2)

    # ---- rendezvous: rank 0 makes the id and publishes it (write, then rename); the others poll with a deadline -----
    version = dv.lib().dbde_hip_gather_rccl_version()
    if rank == 0:
        uid = dv.gather_unique_id()
        with open(id_file + ".tmp", "wb") as f:
            f.write(uid.tobytes())
        os.rename(id_file + ".tmp", id_file)
    else:
        t0 = time.monotonic()
        while not os.path.exists(id_file):
            if time.monotonic() - t0 > 120:
                raise SystemExit(f"rank {rank}: no unique id after 120 s")
            time.sleep(0.01)
        with open(id_file, "rb") as f:
            uid = np.frombuffer(f.read(), np.uint8).copy()
    codec = dv.Codec(0)
    dev = codec.device
    emit("hello", world=world, rank=rank, rccl_version=version, arch=codec.arch)

    def canvas(nbytes):
        return torch.full((nbytes,), 0xEE, dtype=torch.uint8, device=dev)

    class Batch:
        """This rank's block of a gather case, encoded into `seg` at LEAD -- or, in place, into the root's window."""

        def __init__(self, name, root, in_place):
            self.name, self.root = name, root
            W, H, mode, n, piece = GATHER_CASES[name]
            lo, self.nf, n = gather_block(name, rank, world)
            self.piece, self.n = piece, n
            mfb = dv.max_frame_bytes(W, H)
            self.cap = max(n, 1) * mfb                               # what the root's window holds: every rank's worst case
            self.window = canvas(GUARD + self.cap + GUARD) if rank == root else None
            if in_place and rank == root:
                self.seg, self.seg_off = self.window, GUARD
            else:
                self.seg, self.seg_off = canvas(LEAD + max(self.nf, 1) * mfb + GUARD), LEAD
            self.offs = self.sizes = None
            if self.nf:
                imgs = codec.synth_frames(mode, SEED, lo, self.nf, W, H)
                self.offs, self.sizes = codec.encode_frames(imgs, W, H, self.nf, self.seg, self.seg_off, self.nf * mfb, first_index=lo)

        def begin(self, g, slot):
            tail = slice(self.nf - 1, self.nf)
            g.begin(slot, self.offs[tail] if self.nf else None, self.sizes[tail] if self.nf else None)

        def post(self, g, slot, window_bytes=None):
            dv.lib().dbde_hip_gather_set_max_message(g.h, self.piece)
            rc, got = code(lambda: g.post(slot, self.seg, self.seg_off, self.window, GUARD,
                                          self.cap if window_bytes is None else window_bytes))
            g.sync(slot)
            return rc, got

        def report(self, step, rc, got, **more):
            f = dict(case=self.name, root=self.root, rc=rc, **more)
            if rc == dv.OK:
                f["sizes"] = self.got = got
                mine, total = got[rank], sum(got)
                if rank == self.root:
                    w = self.window
                    f.update(window_sha=sha(w[GUARD:GUARD + total]), guard_before=all_are(w[:GUARD], 0xEE),
                             guard_behind=all_are(w[GUARD + total:], 0xEE))
                if self.seg is not self.window:
                    s = self.seg
                    f.update(segment_sha=sha(s[self.seg_off:self.seg_off + mine]), segment_guard_before=all_are(s[:self.seg_off], 0xEE),
                             segment_guard_behind=all_are(s[self.seg_off + mine:], 0xEE))
            else:
                f["error"] = got
                if rank == self.root:
                    f["window_untouched"] = all_are(self.window, 0xEE)
            emit(step, **f)

    def run_gathers(step, g, names, root):
        batches = [Batch(name, root, in_place=(root == 0)) for name in names]

        def begin(k, slot):
            if rank == root:
                g.set_window(batches[k].cap)
            batches[k].begin(g, slot)

        def post(k, slot):
            rc, got = batches[k].post(g, slot)
            batches[k].report(step, rc, got)
        pipeline(len(batches), begin, post)
        return batches

    class Shard:
        """A scatter case: the root's stream behind a non-zero lead, every rank's receive buffers."""

        def __init__(self, name, root, stream=None):
            self.name, self.root = name, root
            W, H, mode, n, cut, piece = SCATTER_CASES[name]
            self.W, self.H, self.piece, self.n = W, H, piece, n
            mfb = dv.max_frame_bytes(W, H)
            self.max_frames = n // world + 2
            self.seg_cap = self.max_frames * mfb
            self.found = self.count = None
            if rank == root:
                if stream is None:
                    imgs = codec.synth_frames(mode, SEED, 0, n, W, H)
                    self.buf, self.lead = canvas(LEAD + n * mfb + GUARD), LEAD
                    offs, sizes = codec.encode_frames(imgs, W, H, n, self.buf, self.lead, n * mfb, first_index=0)
                    codec.sync()
                    self.nbytes = scatter_extent(int((offs[-1] + sizes[-1]).item()), cut)
                else:
                    self.buf, self.lead, self.nbytes = stream
                self.found = torch.empty(n + 4, dtype=torch.int64, device=dev)
                self.count = torch.zeros(1, dtype=torch.int32, device=dev)
            self.fresh()

        def fresh(self):
            self.seg = canvas(self.seg_cap + GUARD)
            self.my_offs = torch.full((self.max_frames + 4,), -1, dtype=torch.int64, device=dev)

        def begin(self, sc, slot, caps=None):
            # the root declares NO segment bytes (its block is decoded in place) but the frames its offsets array holds
            seg_cap, max_frames = caps if caps is not None else ((0 if rank == self.root else self.seg_cap), self.max_frames)
            sc.set_capacity(seg_cap, max_frames)
            if rank == self.root:
                codec.index_stream_async(self.buf, self.lead, self.nbytes, self.W, self.H, self.n + 4, self.found, self.count)
                sc.begin(slot, self.buf, self.lead, self.nbytes, self.found, self.count)
            else:
                sc.begin(slot)

        def post(self, sc, slot):
            dv.lib().dbde_hip_scatter_set_max_message(sc.h, self.piece)
            rc, got = code(lambda: sc.post(slot, self.seg, self.my_offs))
            sc.join(slot)
            sc.sync(slot)
            return rc, got

        def report(self, step, rc, got, **more):
            f = dict(case=self.name, root=self.root, rc=rc, **more)
            if rc == dv.OK:
                mine, table = got
                f0, nf, b0, nb = mine
                f.update(mine=mine, table=table, offsets=self.my_offs[:nf].cpu().tolist(),
                         offsets_guard=all_are(self.my_offs[nf:], -1))
                if rank == self.root:
                    f.update(block_sha=sha(self.buf[self.lead + b0:self.lead + b0 + nb]), segment_guard=all_are(self.seg, 0xEE))
                    src, src_off = self.buf, self.lead + b0
                else:
                    f.update(block_sha=sha(self.seg[:nb]), segment_guard=all_are(self.seg[nb:], 0xEE))
                    src, src_off = self.seg, 0
                if nf:
                    back, res = codec.decode_frames(src, src_off, nb, self.my_offs, self.W, self.H, nf)
                    codec.sync()
                    f.update(images_sha=sha(back), headers=[list(h[:3]) for h in codec.parse_results(res)])
                self.mine, self.table = mine, table
            else:
                f.update(error=got, segment_untouched=all_are(self.seg, 0xEE), offsets_untouched=all_are(self.my_offs, -1))
            emit(step, **f)

    def run_scatters(step, sc, names, root):
        shards = [Shard(name, root) for name in names]

        def post(k, slot):
            rc, got = shards[k].post(sc, slot)
            shards[k].report(step, rc, got)
        pipeline(len(shards), lambda k, slot: shards[k].begin(sc, slot), post)
        return shards

    # ---- 1. gather: root 0 (in place, both slots pipelined), then a non-zero root -----------------------------------
    g0 = dv.Gather(codec, uid, world, rank, 0)
    batches0 = run_gathers("gather", g0, GATHER_ROOT0, 0)
    g_last = dv.Gather(codec, uid, world, rank, last)
    run_gathers("gather", g_last, GATHER_LAST, last)
    g_last.close()

    # ---- 2. scatter: root 0, then a non-zero root -------------------------------------------------------------------
    s0 = dv.Scatter(codec, uid, world, rank, 0)
    shards0 = run_scatters("scatter", s0, SCATTER_ROOT0, 0)
    s_last = dv.Scatter(codec, uid, world, rank, last)
    run_scatters("scatter", s_last, SCATTER_LAST, last)
    s_last.close()

    # ---- 3. gather, then scatter: the stream gathered from G ranks goes back to the same blocks ----------------------
    gathered = batches0[GATHER_ROOT0.index(VERDICT_CASE)]
    # (the root's window of that batch still holds the gathered stream: GUARD bytes of lead, then the frames)
    back = Shard(VERDICT_CASE, 0, stream=(gathered.window, GUARD, sum(gathered.got)) if rank == 0 else None)
    back.begin(s0, 0)
    rc, got = back.post(s0, 0)
    back.report("gather_then_scatter", rc, got)

    # ---- 4. gather, symmetric verdict: the root declares a window one byte too small ---------------------------------
    b = Batch(VERDICT_CASE, 0, in_place=False)         # (a segment of its own on the root too: an untouched window means something)
    total = sum(gathered.got)
    if rank == 0:
        g0.set_window(total - 1)
    b.begin(g0, 0)
    rc, got = b.post(g0, 0)
    b.report("gather_window_one_short", rc, got)
    if rank == 0:
        g0.set_window(b.cap)
    b.begin(g0, 1)
    rc, got = b.post(g0, 1)
    b.report("gather_after_refusal", rc, got)
    g0.close()

    # ---- 5. scatter, symmetric verdict: a peer (rank 1) declares a segment, then a frame count, one too small --------
    shard = shards0[SCATTER_ROOT0.index(VERDICT_CASE)]
    _, nf1, _, nb1 = shard.table[1]
    for step, caps in (("scatter_segment_one_short", (nb1 - 1, shard.max_frames)), ("scatter_frames_one_short", (shard.seg_cap, nf1 - 1)),
                       ("scatter_after_refusal", None)):
        shard.fresh()
        shard.begin(s0, 0, caps=caps if rank == 1 else None)
        rc, got = shard.post(s0, 0)
        shard.report(step, rc, got)

    # ---- 7. the root's own frame capacity: one entry short of its block, with a larger -1 canvas behind it -----------
    # (the canvas is larger than the block, so even a library that ignores the root's declaration stays inside the allocation)
    nf0 = shard.table[0][1]
    shard.fresh()
    shard.begin(s0, 1, caps=(0, nf0 - 1) if rank == 0 else None)
    rc, got = shard.post(s0, 1)
    shard.report("scatter_root_frames_one_short", rc, got)
    if rc != dv.OK:
        shard.fresh()
        shard.begin(s0, 0)
        rc, got = shard.post(s0, 0)
        shard.report("scatter_after_root_refusal", rc, got)
    s0.close()

    # ---- 6. a root that never declared its window, and a total that overflows the window it passes -------------------
    g6 = dv.Gather(codec, uid, world, rank, 0)
    b = Batch(VERDICT_CASE, 0, in_place=False)
    b.begin(g6, 0)
    rc, got = b.post(g6, 0, window_bytes=total - 1)
    b.report("gather_undeclared_window", rc, got)
    if rc == dv.ERR_CAPACITY:                          # (any other outcome has left sends unmatched: nothing more on this handle)
        if rank == 0:
            g6.set_window(b.cap)
        b.begin(g6, 1)
        rc, got = b.post(g6, 1)
        b.report("gather_after_declaring", rc, got)
    g6.close()

    # ---- 8. RoundTripStream(gather="native"): unequal rank blocks, so the short ranks post empty rounds ---------------
    W, H, mode, N, B, piece = STREAM
    lo, hi = block(N, rank, world)
    rounds = max(-(-(block(N, r, world)[1] - block(N, r, world)[0]) // B) for r in range(world))
    side = torch.cuda.Stream()
    src = dv.Codec(0, stream=side)
    g8 = dv.Gather(codec, uid, world, rank, 0, max_message_bytes=piece)
    kept, snaps = {}, []

    def source(first, k, frames):
        src.synth_frames(mode, SEED, first, k, W, H, out=frames)

    def tap(k, slot, n):          # on the codec stream, behind batch k's encode
        kept[k] = (rts.offs[slot][:n].clone(), rts.sizes[slot][:n].clone())

    class Snapshots(RoundTripStream):
        def op_post(self, slot, n):
            before = self._acc[1]
            super().op_post(slot, n)
            if rank == 0:             # the gathered batch, before its window is encoded into again
                self.native.sync(slot)
                nbytes, lead = self._acc[1] - before, self.out[slot][1]
                snaps.append([nbytes, sha(self.window[slot][lead:lead + nbytes])])

    rts = Snapshots(codec, W, H, B, source=source, source_stream=side, gather="native", check=True, native=g8, world=world,
                    rank=rank, tap=tap)
    r = rts.run(lo, hi - lo, world=world, rank=rank, rounds=rounds)
    codec.sync()
    emit("stream", frames=r["frames"], batches=r["batches"], rounds=rounds, packed_bytes=r["packed_bytes"],
         gathered_bytes=r["gathered_bytes"], mismatches=rts.mismatches, snapshots=snaps,
         frame_bytes={str(k): kept[k][1].cpu().tolist() for k in sorted(kept)},
         frame_offsets={str(k): kept[k][0].cpu().tolist() for k in sorted(kept)})
    g8.close()
    src.close()
    codec.close()
    emit("done")
    out.close()


if __name__ == "__main__":
    main()
