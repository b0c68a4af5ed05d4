"""Sequences of calls of different families on ONE context: pools, ops, references and the runner (test infrastructure,
imported like crafted.py; not a test module).

A dbde_hip_ctx keeps workspaces that no call re-initialises (chunk_off / frame_ok / idx_ctr of the decode index, the
encoders' look-back block with its epoch and parity, the fused decoder's records, the partials of projections and
traces, the crop and scan workspaces: DESIGN.md, section 2).  Every family's own tests run that family's calls on a context of
their own; here any entry point follows any other.  tests/test_context_sequences.py holds the chains (CHAINS) and
proves from the plan functions what state each step meets; tests/test_gpu_context_sequences.py runs them.

Pools are small fixed streams built on the host (Pool): crafted ones through test_gpu_crafted_decode.Stream /
test_gpu_crafted_decode16.Stream16 with rejected frames mixed in, "encoder-written" ones packed by the oracles (the
encoders' byte-for-byte parity with them is established elsewhere), each with the oracle's result row and image of
every frame.  An Op is (name, bits, run, expect, plan) plus the shapes of its outputs: run() makes the call into
guarded canvases, expect() gives every output element for element -- the family references of binned_ref, crop_ref,
scaled_ref, wenc_ref, gproject_ref, mask_ref, patch_ref, moments_ref, wproject_ref, family_refs and the oracles -- with the canvas fill where a rejected frame must leave its
output alone, plan() what the planner reports (and the index launch the call makes).  Everything is integer or
bit-exact by specification: every comparison is equality.

run_chain(dv, codec, chain, steps, mode): "stepwise" synchronises and checks after every step; "queued" enqueues the
whole chain without a host synchronisation of its own between steps (every step has its own outputs, allocated and
every input uploaded before the first call), then synchronises once and checks everything.  On a mismatch -- and only
then -- the step is repeated once on a fresh Codec(0) and the assertion says whether that also mismatches (a kernel or
reference bug) or not (carried state).
"""
import os
import struct

import numpy as np

import binned_ref as br
import crafted as cr
import crop_ref
import scaled_ref as sr
import wenc_ref
from family_refs import hist_expect, hist_expect16, map_discs, reduce16, reduce_labels, reduce_numpy

GUARD = 256                      # canvas elements of fill in front of and behind every output
FILLS = {"uint8": 0xEE, "int16": 0xEEEE - 65536, "int32": 0x5A5A5A5A, "int64": 0x5A5A5A5A5A5A5A5A}
ALL4 = ("max", "min", "sum", "sumsq")
TABLE, SELF, FUSED = 0, 1, 2
MID = 3
RESIDENT = 513                   # workgroups the persistent encoders hold (encode_plan's default, test_encode_forms)

OLD_CONSUMERS8 = ("decode_frames", "decode_roi", "project", "traces", "histogram", "decode_binned", "decode_scaled",
                  "crop_frames")
NEW_CONSUMERS8 = ("project_groups", "decode_mask", "decode_patches", "project_weighted", "patch_moments")
CONSUMERS8 = OLD_CONSUMERS8 + NEW_CONSUMERS8
CONSUMERS = CONSUMERS8 + tuple(c + "16" for c in CONSUMERS8)
# (the sixteen the first chains were written for, in their order then, and the ten of the five newer families)
OLD_CONSUMERS = OLD_CONSUMERS8 + tuple(c + "16" for c in OLD_CONSUMERS8)
NEW_CONSUMERS = NEW_CONSUMERS8 + tuple(c + "16" for c in NEW_CONSUMERS8)
# the windows of each pool geometry: the whole frame, and an odd-sized one at a multiple of 8 (crop, binned)
WINDOWS = {(200, 123): ((0, 0, 200, 123), (48, 16, 101, 60)), (72, 72): ((0, 0, 72, 72), (8, 8, 40, 33)),
           (200, 40): ((0, 0, 200, 40), (16, 8, 77, 27))}


def dvm():
    import dbde_video_cpp_amd as dv
    return dv


def split_for(n, cpf):
    """index_split_for (dbde_capi.cpp), as test_decode_forms.split_for restates it and pins it to dv.roi_plan."""
    if n < 1 or n >= 256 or cpf < 8:
        return 1
    return max(1, min(1024 // n, (cpf + 3) // 4))


def grown(cap, want):
    """grow() of dbde_host.h: the capacity after a request for `want` elements."""
    return cap if want <= cap else want + want // 4 + 64


# ---- pools ------------------------------------------------------------------------------------------------------------

class Pool:
    """n frames of one geometry in one stream buffer (host arrays; dev() uploads them once): frames (bytes), rows (the
    oracle's result rows), images (the oracle's images, None for a rejected frame), ok."""

    def __init__(self, name, bits, W, H, frames, rows, images, buf, lead, offs, total):
        self.name, self.bits, self.W, self.H, self.n = name, bits, W, H, len(frames)
        self.frames, self.rows, self.images = frames, rows, images
        self.ok = [im is not None for im in images]
        self.buf, self.lead, self.offs, self.total = buf, lead, offs, total
        self._dev = None
        self.T = cr.tiles(W, H)

    @classmethod
    def of_stream(cls, name, bits, s):
        return cls(name, bits, s.W, s.H, s.frames, s.rows, s.images, s.buf.numpy(), s.lead, s.offs.numpy(), s.total)

    @classmethod
    def of_frames(cls, name, bits, W, H, frames, rows, images, how):
        buf, lead, offs, total = cr.layout(frames, how, lead=32)
        return cls(name, bits, W, H, frames, rows, images, buf, lead, offs, total)

    def reversed(self, name):
        return Pool.of_frames(name, self.bits, self.W, self.H, self.frames[::-1], self.rows[::-1], self.images[::-1],
                              "offsets")

    def dev(self):
        import torch
        if self._dev is None:
            self._dev = (torch.from_numpy(self.buf).cuda(), torch.from_numpy(self.offs).cuda())
        return self._dev

    def images_dev(self, fill):
        """(n, H, W) device tensor of the expected images (each distinct one uploaded once), `fill` where rejected."""
        import torch
        dt = torch.uint8 if self.bits == 8 else torch.int16
        uniq, index = {}, []
        for im in self.images:
            if im is not None and id(im) not in uniq:
                uniq[id(im)] = (len(uniq), im)
            index.append(uniq[id(im)][0] if im is not None else len(self.images) + 1)
        stack = [im for _, im in sorted(uniq.values(), key=lambda p: p[0])]
        npd = np.uint8 if self.bits == 8 else np.int16
        bodies = torch.from_numpy(np.stack([np.ascontiguousarray(im).view(npd) for im in stack])).cuda()
        bodies = torch.cat([bodies, torch.full((1, self.H, self.W), fill, dtype=dt, device="cuda")])
        idx = torch.tensor([min(i, len(stack)) for i in index], device="cuda")
        return bodies[idx]


def _rows_of(oracle, o16, bits, W, H, fr):
    """(result row, image or None) of one frame, from the oracles."""
    _, fh = oracle.unpack_frame_header(fr)
    if bits == 8:
        adv, _, img = oracle.unpack_frame(fr, W, H)
        used = adv - 20
    else:
        from test_oracle_u16 import unpack16
        used, img = unpack16(o16, fr, W, H)
    return (fh[0] if used else 0xFFFFFFFF, fh[1], fh[2], 20 + used), (img if used else None)


def mixed_images(rng, n, H, W, bits):
    """Images whose 8 x 8 tiles take every depth: full-range noise shifted down per tile, on a per-frame base."""
    w, h = (W + 7) // 8, (H + 7) // 8
    px = rng.integers(0, 1 << bits, (n, 8 * h, 8 * w))
    sh = rng.integers(0, bits + 2, (n, h, 1, w, 1))
    px = (px.reshape(n, h, 8, w, 8) >> sh).reshape(n, 8 * h, 8 * w)[:, :H, :W]
    base = rng.integers(0, 1 << bits, (n, 1, 1))
    return np.ascontiguousarray(((px + base) & ((1 << bits) - 1)).astype(np.uint8 if bits == 8 else np.uint16))


def packed_pool(name, oracle, o16, bits, W, H, n, seed, how="concat", breaks=()):
    """An "encoder-written" pool: n images of every depth packed by the oracle; breaks: (frame, rule) pairs replaced by
    crafted.break_rule of the packed frame (rejected frames spliced in)."""
    rng = np.random.default_rng(seed)
    pack = wenc_ref.packer(oracle, bits)
    imgs = mixed_images(rng, n, H, W, bits)
    frames = [pack(1000 + f, imgs[f]) for f in range(n)]
    for f, rule in breaks:
        frames[f] = cr.break_rule(frames[f], rule, bits)
    rows, images = [], []
    for f, fr in enumerate(frames):
        if any(f == b for b, _ in breaks):
            row, img = _rows_of(oracle, o16, bits, W, H, fr)
            assert img is None, (name, f)
        else:
            row, img = (2, 1000 + f, 0, len(fr)), imgs[f]
        rows.append(row)
        images.append(img)
    return Pool.of_frames(name, bits, W, H, frames, rows, images, how)


# which entries of the whole crafted pool (test_gpu_crafted_decode.POOL: 0..9 valid bodies, 10..16 a broken rule each,
# 17 a DBDE16 frame) the 8-bit crafted pools hold, in stream order: rejected frames at 1, 2, 5 and 9 of 13, so that
# reversing the order flips the verdict of indices 1, 2, 3, 5, 7, 9, 10 and 11
SELECT13 = (0, 10, 11, 4, 1, 17, 2, 3, 5, 12, 6, 7, 8)
SELECT_TABLE = (0, 4, 13, 1, 2, 14, 15, 3, 5, 6, 16, 7, 17, 8, 9, 10, 11)   # 17 entries: no period of 2, 3 or 4
SEED16 = {"A": 5, "D": 5}
_pools = {}


def pools(oracle, o16):
    """name -> Pool, built once per process (a few seconds of host work)."""
    if _pools:
        return _pools
    from test_gpu_crafted_decode import Stream
    from test_gpu_crafted_decode16 import Stream16
    import test_decode_forms as tdf
    dv = dvm()
    P = {}

    def crafted8(name, W, H, n, how, select, chunk_tiles=0, seed=0):
        rng = np.random.default_rng(seed or (W * 65537 + H * 257 + n))
        P[name] = Pool.of_stream(name, 8, Stream(oracle, rng, W, H, n, how, chunk_tiles=chunk_tiles, select=list(select),
                                                 device="cpu"))

    def crafted16(name, W, H, n, how, seed):
        P[name] = Pool.of_stream(name, 16, Stream16(o16, oracle, np.random.default_rng(seed), W, H, n, how, device="cpu"))

    # A / A' / B: 200 x 123 x 13 (16 tile rows: the split index); D: 200 x 40 x 13 (5 chunks: never split)
    crafted8("A8", 200, 123, 13, "residues", SELECT13)
    crafted8("D8", 200, 40, 13, "offsets", SELECT13)
    for g, (W, H) in (("A", (200, 123)), ("D", (200, 40))):
        for seed in range(1, 200):   # Stream16 shuffles its pool: the first seed that leaves a rejected frame at 9..11
            crafted16(g + "16", W, H, 13, "offsets", seed)
            if not all(P[g + "16"].ok[9:12]):
                break
    for b in (8, 16):
        P[f"Ar{b}"] = P[f"A{b}"].reversed(f"Ar{b}")
        P[f"B{b}"] = packed_pool(f"B{b}", oracle, o16, b, 200, 123, 13, seed=200 + b, how="residues")
        # C: 72 x 72 x 300 (one index workgroup per frame from 256 frames on), five rejected frames spliced in
        P[f"C{b}"] = packed_pool(f"C{b}", oracle, o16, b, 72, 72, 300, seed=72 + b, how="concat",
                                 breaks=((3, "depth"), (77, "n64+1"), (150, "nm-1"), (256, "T+1"), (298, "n64-1")))
    # E: decode_frames' own forms, the smallest row of DECODE_CASES for each
    rows = {}
    for c in tdf.DECODE_CASES:
        k = tdf.row_index(c) or "mid"
        if k not in rows or c[0] * c[1] * c[2] < rows[k][0] * rows[k][1] * rows[k][2]:
            rows[k] = c
    # (the split row holds 4 frames more than its batch, so that two batches of the row's size differ in their verdicts;
    # the fused row six frames: launches of one, two, three and six frames are all fused)
    for k, nn in (("split", rows["split"][2] + 4), ("table", None), ("self", None), ("fused", 6), ("mid", None)):
        W, H, n, how, residue, _ = rows[k]
        ct = dv.decode_plan(W, H, n, residue)["chunk_tiles"]
        crafted8("E" + k, W, H, nn or n, how, SELECT_TABLE if n >= 17 else SELECT13[:nn or n] if (nn or n) > 3 else (0, 10, 4), ct)
        P["E" + k].residue = residue
        P["E" + k].n_default = n if k == "split" else (nn or n)
    _pools.update(P)
    return _pools


def assert_pool_properties(P):
    """The plan property each pool exists for (a planner change then fails here, not as lost coverage)."""
    dv = dvm()
    import test_decode_forms as tdf
    for b, roi in ((8, dv.roi_plan), (16, dv.roi16_plan)):
        A, Ar, B, C, D = (P[f"{k}{b}"] for k in ("A", "Ar", "B", "C", "D"))
        pl = roi(A.W, A.H, A.n, 0, 0, A.W, A.H)
        assert pl["index_split"] > 1 and pl["tiles_y"] == 16 and A.n == 13, pl
        assert not all(A.ok) and A.ok[0] and A.ok[-1], A.ok
        assert Ar.ok == A.ok[::-1]
        assert any(a and not r for a, r in zip(A.ok, Ar.ok)) and any(r and not a for a, r in zip(A.ok, Ar.ok)), A.ok
        assert (B.W, B.H, B.n) == (A.W, A.H, A.n) and all(B.ok)
        pl = roi(C.W, C.H, C.n, 0, 0, C.W, C.H)
        assert C.n >= 256 and pl["index_split"] == 1 and 0 < C.ok.count(False) <= 8, (pl, C.ok.count(False))
        assert split_for(13, pl["chunks_per_frame"]) > 1, pl       # ... and split for a batch of 13 of them
        pl = roi(D.W, D.H, D.n, 0, 0, D.W, D.H)
        assert pl["chunks_per_frame"] < 8 and pl["index_split"] == 1 and not all(D.ok), pl
        assert pl["chunks_per_frame"] != roi(A.W, A.H, A.n, 0, 0, A.W, A.H)["chunks_per_frame"]
        # the patch families index the whole frame whatever the patch: PATCH splits on A, not on D, not on C's 300 frames
        for fn in ("patches", "patch_moments"):
            plan = getattr(dv, fn + suffix(b) + "_plan")
            for edge in ("clamp", "fill"):
                split = {p.name[0]: plan(p.W, p.H, p.n, *PATCH, PATCHES_PER_FRAME, edge)["index_split"] for p in (A, C, D)}
                assert split["A"] > 1 and split["C"] == 1 and split["D"] == 1, (fn, b, edge, split)
    assert dv.decode_plan(72, 72, 300)["kernel"] == MID
    for k, want in (("split", "split"), ("table", "table"), ("self", "self"), ("fused", "fused"), ("mid", None)):
        E = P["E" + k]
        pl = dv.decode_plan(E.W, E.H, E.n_default, E.residue)
        assert tdf.index_of(E.n_default, pl) == want, (k, pl)
        assert not all(E.ok) and E.ok[0], (k, E.ok)
    pl = dv.decode_plan(P["Efused"].W, P["Efused"].H, 1, P["Efused"].residue)
    assert pl["index_mode"] == FUSED, pl     # one frame alone is still too large to index itself


# ---- canvases ----------------------------------------------------------------------------------------------------------

class Canvas:
    """A device output of `shape` with GUARD (+ residue) elements of the fill in front of it and GUARD behind."""

    def __init__(self, shape, dtype, residue=0):
        import torch
        size = int(np.prod(shape))
        self.fill, self.lo, self.hi = FILLS[dtype], GUARD + residue, GUARD + residue + size
        self.flat = torch.full((self.hi + GUARD,), self.fill, dtype=getattr(torch, dtype), device="cuda")
        self.t = self.flat[self.lo: self.hi].view(*shape)

    def guards_hold(self):
        return bool(((self.flat[:self.lo] == self.fill).all() & (self.flat[self.hi:] == self.fill).all()).item())


def make_outputs(spec):
    return {k: Canvas(*v) for k, v in spec.items()}


def filled(shape, dtype):
    return np.full(shape, FILLS[dtype], getattr(np, dtype))


def rows_array(rows):
    return np.array([[r[0], r[1], r[2], r[3]] for r in rows], np.uint64).reshape(-1, 4).view(np.int64)


# ---- ops ---------------------------------------------------------------------------------------------------------------

class Op:
    """(name, bits, run, expect, plan) and outputs(pool, params) -> {name: (shape, dtype[, residue])}.  kind:
    "consumer" (runs the decode index as a launch of its own), else the intervener's kind.  expect may return None for
    an output that is not compared (none does so far); raises: the call must raise DbdeError and write nothing."""

    def __init__(self, name, bits, kind, run, expect, plan, outputs, prepare=None, raises=False):
        self.name, self.bits, self.kind = name, bits, kind
        self.run, self.expect, self.plan, self.outputs, self.prepare, self.raises = run, expect, plan, outputs, prepare, raises


OPS = {}
_const = {}


def const(key, make):
    """A device constant (origins, maps, sources), uploaded once per process."""
    if key not in _const:
        _const[key] = make()
    return _const[key]


def frames_of(pool, prm):
    f0, n = prm.get("f0", 0), prm.get("n", getattr(pool, "n_default", pool.n))
    assert 0 <= f0 and n >= 0 and f0 + n <= pool.n, (pool.name, prm)
    return f0, n


def window_of(pool, prm):
    """The step's window: prm["win"] = (x, y, rw, rh) where the step brings its own (tests/geometry_cases.py), else
    entry prm["w"] of the pool geometry's WINDOWS."""
    if prm.get("win") is not None:
        return tuple(prm["win"])
    return WINDOWS[(pool.W, pool.H)][prm.get("w", 0)]


def stream_args(pool, prm):
    buf, offs = pool.dev()
    f0, n = frames_of(pool, prm)
    return buf, pool.lead, pool.total, offs[f0:f0 + n] if n else offs, pool.W, pool.H, n   # (an empty slice has no address)


def origins_of(pool, prm):
    """Per-frame origins (host, (n, 2) int32) of a step that asks for them, else None: prm["origins"] (one (x, y) per
    pool frame) where the step brings its own, else (prm["org"]) random ones."""
    f0, n = frames_of(pool, prm)
    if prm.get("origins") is not None:
        return np.array(prm["origins"], np.int32).reshape(-1, 2)[f0:f0 + n]
    if not prm.get("org"):
        return None
    rng = np.random.default_rng(pool.W * 131 + pool.H * 7 + n + f0)
    return np.stack([rng.integers(-3, pool.W + 3, n), rng.integers(-3, pool.H + 3, n)], 1).astype(np.int32)


def origins_dev(pool, prm):
    import torch
    org = origins_of(pool, prm)
    if org is None:
        return None
    return const(("org", pool.name, prm.get("origins")) + frames_of(pool, prm), lambda: torch.from_numpy(org).cuda())


def pix_dtype(bits):
    return "uint8" if bits == 8 else "int16"


def as_pix(a, bits):
    """Values as the canvas holds them: uint8, or int16 holding the U16 bits."""
    a = np.asarray(a)
    return a.astype(np.uint8) if bits == 8 else a.astype(np.uint16).view(np.int16)


def images_or_zero(pool, f0, n):
    z = np.zeros((pool.H, pool.W), np.uint8 if pool.bits == 8 else np.uint16)
    return np.stack([pool.images[f] if pool.ok[f] else z for f in range(f0, f0 + n)]) if n else z[None][:0]


def index_of_roi_plan(bits, n, pl):
    return dict(bits=bits, n=n, cpf=pl["chunks_per_frame"], split=pl["index_split"])


def roi_family_plan(fn8, fn16, extra=lambda pool, prm: ()):
    """plan(pool, prm) of a window-family consumer: the family's own plan function, plus the index launch it makes."""
    def plan(pool, prm):
        dv = dvm()
        f0, n = frames_of(pool, prm)
        x, y, rw, rh = window_of(pool, prm)
        pl = getattr(dv, fn8 if pool.bits == 8 else fn16)(pool.W, pool.H, n, *extra(pool, prm), x, y, rw, rh)
        pl["index"] = index_of_roi_plan(pool.bits, n, pl)
        return pl
    return plan


def results_spec(n):
    return {"results": ((n, 4), "int64")}


# decode_frames in its table form (pools Esplit / Etable) and decode_frames16 ------------------------------------------
def _dec_outputs(pool, prm):
    f0, n = frames_of(pool, prm)
    return dict(images=((n, pool.H, pool.W), pix_dtype(pool.bits), getattr(pool, "residue", 0)), **results_spec(n))


def _dec_run(codec, pool, prm, out):
    buf, lead, total, offs, W, H, n = stream_args(pool, prm)
    if pool.bits == 8:
        codec.decode_frames(buf, lead, total, offs, W, H, n, images=out["images"].t, results=out["results"].t)
    else:
        # (decode_frames16 allocates its results itself: they are copied into the step's canvas on the stream)
        _, res = codec.decode_frames16(buf, lead, total, offs, W, H, n, images=out["images"].t)
        out["results"].t[:n].copy_(res)


def _dec_expect(pool, prm):
    f0, n = frames_of(pool, prm)
    key = ("images", pool.name)
    imgs = const(key, lambda: pool.images_dev(FILLS[pix_dtype(pool.bits)]))
    return dict(images=imgs[f0:f0 + n], results=rows_array(pool.rows[f0:f0 + n]))


def _dec_plan(want_index):
    def plan(pool, prm):
        dv = dvm()
        f0, n = frames_of(pool, prm)
        if pool.bits == 16:   # dbde16_hip_decode_frames: plain runs of 256 tiles, one index workgroup per frame
            return dict(index=dict(bits=16, n=n, cpf=(pool.T + 255) // 256, split=1))
        if n == 0:
            return {}
        pl = dv.decode_plan(pool.W, pool.H, n, getattr(pool, "residue", 0))
        mode = "mid" if pl["kernel"] == MID else ("table", "self", "fused")[pl["index_mode"]]
        assert mode == want_index, f"decode_frames of {pool.name} x {n} runs the {mode} form, not the {want_index} form"
        if mode == "table":
            pl["index"] = dict(bits=8, n=n, cpf=pl["chunks_per_frame"], split=split_for(n, pl["chunks_per_frame"]))
        return pl
    return plan


OPS["decode_frames"] = Op("decode_frames", 8, "consumer", _dec_run, _dec_expect, _dec_plan("table"), _dec_outputs)
OPS["decode_frames16"] = Op("decode_frames16", 16, "consumer", _dec_run, _dec_expect, _dec_plan("table"), _dec_outputs)
for _form in ("self", "fused", "mid"):
    OPS["decode_" + _form] = Op("decode_" + _form, 8, "decode_" + _form, _dec_run, _dec_expect, _dec_plan(_form), _dec_outputs)


# decode_roi ---------------------------------------------------------------------------------------------------------
def _roi_outputs(pool, prm):
    f0, n = frames_of(pool, prm)
    x, y, rw, rh = window_of(pool, prm)
    return dict(out=((n, rh, rw), pix_dtype(pool.bits)), **results_spec(n))


def _roi_run(codec, pool, prm, out):
    fn = codec.decode_roi if pool.bits == 8 else codec.decode_roi16
    fn(*stream_args(pool, prm), *window_of(pool, prm), origins=origins_dev(pool, prm), out=out["out"].t,
       results=out["results"].t)


def _roi_expect(pool, prm):
    f0, n = frames_of(pool, prm)
    x, y, rw, rh = window_of(pool, prm)
    org = origins_of(pool, prm)
    want = filled((n, rh, rw), pix_dtype(pool.bits))
    for k in range(n):
        if pool.ok[f0 + k]:
            ox, oy = (x, y) if org is None else wenc_ref.clamp_origin(org[k, 0], org[k, 1], pool.W, pool.H, rw, rh)
            want[k] = as_pix(pool.images[f0 + k][oy:oy + rh, ox:ox + rw], pool.bits)
    return dict(out=want, results=rows_array(pool.rows[f0:f0 + n]))


for _b in (8, 16):
    _s = "" if _b == 8 else "16"
    OPS["decode_roi" + _s] = Op("decode_roi" + _s, _b, "consumer", _roi_run, _roi_expect,
                                roi_family_plan("roi_plan", "roi16_plan"), _roi_outputs,
                                prepare=lambda codec, pool, prm: origins_dev(pool, prm))


# project ------------------------------------------------------------------------------------------------------------
def _proj_outputs(pool, prm):
    f0, n = frames_of(pool, prm)
    x, y, rw, rh = window_of(pool, prm)
    spec = {s: ((rh, rw), pix_dtype(pool.bits) if s in ("max", "min") else "int64") for s in prm.get("stats", ALL4)}
    return dict(spec, count=((1,), "int64"), **results_spec(n))


def _proj_run(codec, pool, prm, out):
    dv = dvm()
    pr = dv.Projection(count=out["count"].t, **{s: out[s].t for s in prm.get("stats", ALL4)})
    fn = codec.project if pool.bits == 8 else codec.project16
    fn(*stream_args(pool, prm), *window_of(pool, prm), out=pr, accumulate=bool(prm.get("acc_from") is not None
                                                                                and prm["acc_from"] < prm.get("f0", 0)),
       results=out["results"].t)


def _proj_expect(pool, prm):
    f0, n = frames_of(pool, prm)
    x, y, rw, rh = window_of(pool, prm)
    start = prm["acc_from"] if prm.get("acc_from") is not None else f0    # a continuation: everything since its start
    ims = [pool.images[f] for f in range(start, f0 + n) if pool.ok[f]]
    red = (reduce_numpy if pool.bits == 8 else reduce16)(ims, x, y, rw, rh)
    want = {s: as_pix(red[s], pool.bits) if s in ("max", "min") else red[s].astype(np.int64) for s in prm.get("stats", ALL4)}
    return dict(want, count=np.array([red["count"]], np.int64), results=rows_array(pool.rows[f0:f0 + n]))


def _proj_plan(pool, prm):
    dv = dvm()
    f0, n = frames_of(pool, prm)
    x, y, rw, rh = window_of(pool, prm)
    fn = dv.project_plan if pool.bits == 8 else dv.project16_plan
    pl = fn(pool.W, pool.H, n, x, y, rw, rh, stats=prm.get("stats", ALL4))
    pl["index"] = index_of_roi_plan(pool.bits, n, pl)
    return pl


for _b in (8, 16):
    _s = "" if _b == 8 else "16"
    OPS["project" + _s] = Op("project" + _s, _b, "consumer", _proj_run, _proj_expect, _proj_plan, _proj_outputs)


# traces -------------------------------------------------------------------------------------------------------------
LABEL_COUNTS = {"few": 7, "many": 40}


def labels_of(pool, prm):
    if prm.get("label_windows") is not None:     # label k + 1 = the k-th window (x, y, rw, rh); later ones over earlier ones
        lab = np.zeros((pool.H, pool.W), np.int32)
        for k, (x, y, rw, rh) in enumerate(prm["label_windows"]):
            lab[y:y + rh, x:x + rw] = k + 1
        return lab, len(prm["label_windows"])
    lab, L = map_discs(pool.W, pool.H, seed=5, count=LABEL_COUNTS[prm.get("labels", "few")])
    lab[:, : pool.W // 4] = 0          # untouched tiles too
    return lab, L


def _trace_map(codec, pool, prm):
    maps = codec.__dict__.setdefault("_sequence_maps", {})
    key = (pool.W, pool.H, prm.get("labels", "few"), prm.get("label_windows"))
    if key not in maps:
        maps[key] = codec.trace_map(*labels_of(pool, prm))
    return maps[key]


def _trace_outputs(pool, prm):
    f0, n = frames_of(pool, prm)
    L = len(prm["label_windows"]) if prm.get("label_windows") is not None else LABEL_COUNTS[prm.get("labels", "few")]
    spec = {s: ((n, L), pix_dtype(pool.bits) if s in ("max", "min") else "int64") for s in prm.get("stats", ALL4)}
    return dict(spec, **results_spec(n))


def _trace_run(codec, pool, prm, out):
    dv = dvm()
    tm = _trace_map(codec, pool, prm)
    tr = dv.Traces(pixels=tm.pixels, **{s: out[s].t for s in prm.get("stats", ALL4)})
    fn = codec.traces if pool.bits == 8 else codec.traces16
    fn(*stream_args(pool, prm), tm, out=tr, results=out["results"].t)


def _trace_expect(pool, prm):
    import torch
    f0, n = frames_of(pool, prm)
    lab, L = labels_of(pool, prm)
    imgs = torch.from_numpy(images_or_zero(pool, f0, n).astype(np.int32))
    red = reduce_labels(imgs, lab, L, pix_max=255 if pool.bits == 8 else 65535)
    want = {}
    for s in prm.get("stats", ALL4):
        dt = pix_dtype(pool.bits) if s in ("max", "min") else "int64"
        a = red[s].numpy()
        a = as_pix(a, pool.bits) if s in ("max", "min") else a.astype(np.int64)
        for k in range(n):
            if not pool.ok[f0 + k]:
                a[k] = FILLS[dt]      # a rejected frame's rows are left as they were
        want[s] = a
    return dict(want, results=rows_array(pool.rows[f0:f0 + n]))


def _trace_plan(pool, prm):
    dv = dvm()
    f0, n = frames_of(pool, prm)
    lab, L = labels_of(pool, prm)
    info = dv.trace_map_summary(lab, L)
    pl = (dv.trace_plan if pool.bits == 8 else dv.trace16_plan)(pool.W, pool.H, n, info, stats=prm.get("stats", ALL4))
    pl["index"] = index_of_roi_plan(pool.bits, n, pl)
    pl["n_labels"] = L
    return pl


for _b in (8, 16):
    _s = "" if _b == 8 else "16"
    OPS["traces" + _s] = Op("traces" + _s, _b, "consumer", _trace_run, _trace_expect, _trace_plan, _trace_outputs,
                            prepare=lambda codec, pool, prm: _trace_map(codec, pool, prm))


# histogram ----------------------------------------------------------------------------------------------------------
def _hist_binning(pool, prm):
    return prm.get("shift", 0), prm.get("bins", 256 if pool.bits == 8 else 4096)


def _hist_outputs(pool, prm):
    f0, n = frames_of(pool, prm)
    shift, bins = _hist_binning(pool, prm)
    return dict(counts=((n, bins), "int32"), total=((bins,), "int64"), count=((1,), "int64"), **results_spec(n))


def _hist_run(codec, pool, prm, out):
    dv = dvm()
    shift, bins = _hist_binning(pool, prm)
    h = dv.Histograms(out["counts"].t, out["total"].t, out["count"].t)
    fn = codec.histogram if pool.bits == 8 else codec.histogram16
    fn(*stream_args(pool, prm), *window_of(pool, prm), shift=shift, bins=bins, out=h,
       accumulate=bool(prm.get("acc_from") is not None and prm["acc_from"] < prm.get("f0", 0)), results=out["results"].t)


def _hist_rows(pool, f0, n, win, shift, bins):
    x, y, rw, rh = win
    if n == 0:
        return np.zeros((0, bins), np.int64)
    if pool.bits == 8:
        return hist_expect([im for im in images_or_zero(pool, f0, n)], x, y, rw, rh, shift, bins).numpy()
    return hist_expect16(images_or_zero(pool, f0, n), x, y, rw, rh, shift, bins).numpy()


def _hist_expect(pool, prm):
    f0, n = frames_of(pool, prm)
    shift, bins = _hist_binning(pool, prm)
    rows = _hist_rows(pool, f0, n, window_of(pool, prm), shift, bins)
    counts = rows.astype(np.int32)
    for k in range(n):
        if not pool.ok[f0 + k]:
            counts[k] = FILLS["int32"]
    start = prm["acc_from"] if prm.get("acc_from") is not None else f0
    since = _hist_rows(pool, start, f0 + n - start, window_of(pool, prm), shift, bins)
    keep = np.array(pool.ok[start:f0 + n], bool)
    return dict(counts=counts, total=since[keep].sum(0).astype(np.int64).reshape(bins),
                count=np.array([int(keep.sum())], np.int64), results=rows_array(pool.rows[f0:f0 + n]))


def _hist_plan(pool, prm):
    dv = dvm()
    f0, n = frames_of(pool, prm)
    x, y, rw, rh = window_of(pool, prm)
    shift, bins = _hist_binning(pool, prm)
    fn = dv.histogram_plan if pool.bits == 8 else dv.histogram16_plan
    pl = fn(pool.W, pool.H, n, x, y, rw, rh, shift=shift, bins=bins, per_frame=True, total=True)
    pl["index"] = index_of_roi_plan(pool.bits, n, pl)
    return pl


for _b in (8, 16):
    _s = "" if _b == 8 else "16"
    OPS["histogram" + _s] = Op("histogram" + _s, _b, "consumer", _hist_run, _hist_expect, _hist_plan, _hist_outputs)


# decode_binned ------------------------------------------------------------------------------------------------------
def _bin_dtypes(bits):
    return dict(sum="int16", max="uint8", min="uint8") if bits == 8 else dict(sum="int32", max="int16", min="int16")


def _bin_outputs(pool, prm):
    f0, n = frames_of(pool, prm)
    x, y, rw, rh = window_of(pool, prm)
    oh, ow = br.out_shape(rw, rh, prm.get("bin", 4))
    return dict({s: ((n, oh, ow), dt) for s, dt in _bin_dtypes(pool.bits).items()}, **results_spec(n))


def _bin_run(codec, pool, prm, out):
    dv = dvm()
    x, y, rw, rh = window_of(pool, prm)
    planes = dv.Binned(sum=out["sum"].t, max=out["max"].t, min=out["min"].t)
    fn = codec.decode_binned if pool.bits == 8 else codec.decode_binned16
    fn(*stream_args(pool, prm), prm.get("bin", 4), x, y, rw, rh, out=planes, results=out["results"].t)


def _bin_expect(pool, prm):
    f0, n = frames_of(pool, prm)
    x, y, rw, rh = window_of(pool, prm)
    red = br.binned_reduceat(images_or_zero(pool, f0, n), x, y, rw, rh, prm.get("bin", 4))
    want = {}
    for s, dt in _bin_dtypes(pool.bits).items():
        a = red[s].astype({"uint8": np.uint8, "int16": np.uint16, "int32": np.uint32}[dt]).view(getattr(np, dt))
        for k in range(n):
            if not pool.ok[f0 + k]:
                a[k] = FILLS[dt]
        want[s] = a
    return dict(want, results=rows_array(pool.rows[f0:f0 + n]))


for _b in (8, 16):
    _s = "" if _b == 8 else "16"
    OPS["decode_binned" + _s] = Op("decode_binned" + _s, _b, "consumer", _bin_run, _bin_expect,
                                   roi_family_plan("binned_plan", "binned16_plan", lambda pool, prm: (prm.get("bin", 4),)),
                                   _bin_outputs)


# decode_scaled ------------------------------------------------------------------------------------------------------
def _scaled_maps(pool):
    return sr.maps(pool.W + pool.H, pool.W, pool.H)


def _scaled_maps_dev(pool):
    import torch
    return const(("maps", pool.W, pool.H), lambda: tuple(torch.from_numpy(m).cuda() for m in _scaled_maps(pool)))


def _scaled_outputs(pool, prm):
    f0, n = frames_of(pool, prm)
    x, y, rw, rh = window_of(pool, prm)
    return dict(out=((n, rh, rw), "int32" if prm.get("type", "f32") == "f32" else "int16"), **results_spec(n))


def _scaled_run(codec, pool, prm, out):
    x, y, rw, rh = window_of(pool, prm)
    dark, gain = _scaled_maps_dev(pool)
    dt = sr.torch_dtype(prm.get("type", "f32"))
    fn = codec.decode_scaled if pool.bits == 8 else codec.decode_scaled16
    fn(*stream_args(pool, prm), x, y, rw, rh, dtype=dt, dark=dark, gain=gain, origins=origins_dev(pool, prm),
       out=out["out"].t.view(dt), results=out["results"].t)


def _scaled_expect(pool, prm):
    f0, n = frames_of(pool, prm)
    x, y, rw, rh = window_of(pool, prm)
    t = prm.get("type", "f32")
    dark, gain = _scaled_maps(pool)
    dt = "int32" if t == "f32" else "int16"
    want = sr.expected(images_or_zero(pool, f0, n), x, y, rw, rh, dark, gain, t, origins_of(pool, prm)).view(getattr(np, dt))
    for k in range(n):
        if not pool.ok[f0 + k]:
            want[k] = FILLS[dt]
    return dict(out=want, results=rows_array(pool.rows[f0:f0 + n]))


def _scaled_plan(pool, prm):
    dv = dvm()
    f0, n = frames_of(pool, prm)
    x, y, rw, rh = window_of(pool, prm)
    fn = dv.scaled_plan if pool.bits == 8 else dv.scaled16_plan
    pl = fn(pool.W, pool.H, n, x, y, rw, rh, dtype=sr.OUT[prm.get("type", "f32")])
    pl["index"] = index_of_roi_plan(pool.bits, n, pl)
    return pl


for _b in (8, 16):
    _s = "" if _b == 8 else "16"
    OPS["decode_scaled" + _s] = Op("decode_scaled" + _s, _b, "consumer", _scaled_run, _scaled_expect, _scaled_plan,
                                   _scaled_outputs,
                                   prepare=lambda codec, pool, prm: (_scaled_maps_dev(pool), origins_dev(pool, prm)))


# crop_frames --------------------------------------------------------------------------------------------------------
def _crop_cap(pool, prm):
    f0, n = frames_of(pool, prm)
    x, y, rw, rh = window_of(pool, prm)
    maxf = crop_ref.max_frame_bytes(rw, rh, pool.bits)
    slot = (maxf + 255) // 256 * 256 if prm.get("slots") else 0
    return slot, ((n - 1) * slot + maxf if slot else n * maxf)


def _crop_outputs(pool, prm):
    f0, n = frames_of(pool, prm)
    slot, cap = _crop_cap(pool, prm)
    return dict(out=((cap,), "uint8"), offsets=((n,), "int64"), nbytes=((n,), "int64"), used=((n, 2), "int32"),
                **results_spec(n))


def _crop_run(codec, pool, prm, out):
    slot, cap = _crop_cap(pool, prm)
    fn = codec.crop_frames if pool.bits == 8 else codec.crop_frames16
    c = out["out"]
    fn(*stream_args(pool, prm), *window_of(pool, prm), c.flat, c.lo, cap, origins=origins_dev(pool, prm),
       slot_stride=slot, out_offsets=out["offsets"].t, out_bytes=out["nbytes"].t, origins_used=out["used"].t,
       results=out["results"].t)


def _crop_expect(pool, prm):
    f0, n = frames_of(pool, prm)
    x, y, rw, rh = window_of(pool, prm)
    slot, cap = _crop_cap(pool, prm)
    outs, offs, nbytes, used = crop_ref.crop_batch(pool.frames[f0:f0 + n], pool.W, pool.H, x, y, rw, rh, pool.bits,
                                                   origins_of(pool, prm), slot)
    assert [o is not None for o in outs] == pool.ok[f0:f0 + n], "crop_ref and the oracle disagree on a verdict"
    want = filled((cap,), "uint8")
    for o, fr in zip(offs, outs):
        if fr is not None:
            want[int(o): int(o) + len(fr)] = fr
    return dict(out=want, offsets=offs, nbytes=nbytes, used=used, results=rows_array(pool.rows[f0:f0 + n]))


def _crop_plan(pool, prm):
    dv = dvm()
    f0, n = frames_of(pool, prm)
    x, y, rw, rh = window_of(pool, prm)
    slot, cap = _crop_cap(pool, prm)
    pl = (dv.crop_plan if pool.bits == 8 else dv.crop16_plan)(pool.W, pool.H, n, x, y, rw, rh, slot_stride=slot)
    assert pl["out_capacity"] <= cap, pl
    pl["index"] = index_of_roi_plan(pool.bits, n, pl)
    return pl


for _b in (8, 16):
    _s = "" if _b == 8 else "16"
    OPS["crop_frames" + _s] = Op("crop_frames" + _s, _b, "consumer", _crop_run, _crop_expect, _crop_plan, _crop_outputs,
                                 prepare=lambda codec, pool, prm: origins_dev(pool, prm))


# ---- the five newer families: what they share ------------------------------------------------------------------------
PATCH = (24, 16)                 # pw x ph of the patch families: inside every pool geometry, more than one tile row
PATCHES_PER_FRAME = 6


def suffix(bits):
    return "" if bits == 8 else "16"


def images_or_none(pool, f0, n):
    return [pool.images[f] if pool.ok[f] else None for f in range(f0, f0 + n)]


def parts_of(prm, f0, n):
    """The (f0, n) of every call whose frames the step's shared outputs hold: of a continuation (prm["cuts"]: the frame
    numbers its parts begin and end at) the parts up to this one, else the step itself."""
    if prm.get("acc") is None:
        return [(f0, n)]
    cuts = prm["cuts"]
    assert f0 in cuts[:-1] and f0 + n == cuts[cuts.index(f0) + 1] and cuts[0] == prm["acc_from"], prm
    return [(a, b - a) for a, b in zip(cuts, cuts[1:]) if a <= f0]


def continues(prm):
    return bool(prm.get("acc") is not None and prm["acc_from"] < prm.get("f0", 0))


def device_cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def band_of(pool, prm):
    """(lo, hi) of a step: "mid" the middle half of the range, "empty" lo > hi, "tile" the minimum and maximum of one
    8 x 8 tile of the pool's first accepted image (the sites of a decision taken from the tile's header alone)."""
    top = (1 << pool.bits) - 1
    kind = prm.get("band", "mid")
    if kind == "mid":
        return top // 4, top - top // 4
    if kind == "empty":
        return top // 2, top // 2 - 1
    assert kind == "tile"
    im = next(im for im in pool.images if im is not None)
    ty, tx = (pool.H // 16) * 8, (pool.W // 16) * 8
    return int(im[ty:ty + 8, tx:tx + 8].min()), int(im[ty:ty + 8, tx:tx + 8].max())


def patch_origins_of(pool, prm):
    """(n, K, 2) int64 origins: prm["porg"] (K per pool frame) where the step brings its own, else random ones inside
    the frame, across its edges and wholly outside it."""
    f0, n = frames_of(pool, prm)
    if prm.get("porg") is not None:
        return np.array(prm["porg"], np.int64).reshape(-1, PATCHES_PER_FRAME, 2)[f0:f0 + n]
    pw, ph = PATCH
    rng = np.random.default_rng(pool.W * 137 + pool.H * 11 + n + f0)
    org = np.stack([rng.integers(-pw - 2, pool.W + 3, (n, PATCHES_PER_FRAME)),
                    rng.integers(-ph - 2, pool.H + 3, (n, PATCHES_PER_FRAME))], -1).astype(np.int64)
    if n:
        org[0, 0] = (-pw, -ph)                                    # wholly outside
        org[-1, -1] = (pool.W - pw // 2, pool.H - ph // 2)        # across the far corner
    return org


def patch_counts_of(pool, prm):
    """None, or the live patches per frame: a 0, a value above K, everything between."""
    if not prm.get("counts"):
        return None
    f0, n = frames_of(pool, prm)
    K = PATCHES_PER_FRAME
    return np.resize(np.array([K + 3, 0, 1, K, 2, K - 1], np.int64), n)


def _patch_inputs(pool, prm):
    """The device origins (for a call without frames: those of one frame, which is never read) and counts."""
    import torch
    f0, n = frames_of(pool, prm)
    key = (pool.name, f0, n, bool(prm.get("counts")), prm.get("porg"))
    src = prm if n else dict(prm, n=1)
    org = const(("patch_org",) + key, lambda: torch.from_numpy(patch_origins_of(pool, src).astype(np.int32)).cuda())
    cnt = patch_counts_of(pool, src)
    if cnt is not None:
        cnt = const(("patch_cnt",) + key, lambda: torch.from_numpy(cnt.astype(np.int32)).cuda())
    return org, cnt


# project_groups -------------------------------------------------------------------------------------------------------
GROUP_STARTS = (0, 5, 5, 2, 9, 4000)      # pool frame numbers: [0, 5), two empty groups, [2, 9) overlapping, the rest


def _grp_starts(pool, prm):
    """None (the uniform form), or the call's group_starts: the step's, which count the pool's frames, from the call's
    first frame on (a group that ends before it is empty, one that begins before it begins with it)."""
    if prm.get("starts") is None:
        return None
    f0, n = frames_of(pool, prm)
    return [max(int(s) - f0, 0) for s in prm["starts"]]


def _grp_groups(pool, prm):
    f0, n = frames_of(pool, prm)
    return len(prm["starts"]) - 1 if prm.get("starts") is not None else -(-n // prm["g"])


def _grp_outputs(pool, prm):
    f0, n = frames_of(pool, prm)
    x, y, rw, rh = window_of(pool, prm)
    G = _grp_groups(pool, prm)
    dts = dict(max=pix_dtype(pool.bits), min=pix_dtype(pool.bits), sum="int16" if prm.get("sum16") else "int32", sumsq="int64")
    return dict({s: ((G, rh, rw), dts[s]) for s in prm.get("stats", ALL4)}, group_counts=((G,), "int32"), **results_spec(n))


def _grp_starts_dev(pool, prm):
    import torch
    st = _grp_starts(pool, prm)
    if st is None:
        return None
    return const(("starts", tuple(st)), lambda: torch.tensor(st, dtype=torch.int32, device="cuda"))


def _grp_run(codec, pool, prm, out):
    import torch
    dv = dvm()
    pr = dv.GroupProjection(counts=out["group_counts"].t, **{s: out[s].t for s in prm.get("stats", ALL4)})
    fn = codec.project_groups if pool.bits == 8 else codec.project_groups16
    fn(*stream_args(pool, prm), *window_of(pool, prm), group_frames=prm.get("g"), group_starts=_grp_starts_dev(pool, prm),
       stats=prm.get("stats", ALL4), sum_dtype=torch.int16 if prm.get("sum16") else torch.int32, accumulate=continues(prm),
       out=pr, results=out["results"].t)


def _grp_reduce(pool, prm, parts):
    """gproject_ref over the frames of every group, the calls `parts` taken together (every value is an exact integer:
    the order does not matter)."""
    import gproject_ref as gr
    x, y, rw, rh = window_of(pool, prm)
    G = _grp_groups(pool, prm)
    frames = [[] for _ in range(G)]
    for f0, n in parts:
        step = dict(prm, f0=f0, n=n)
        for k, (b, e) in enumerate(gr.group_ranges(n, prm.get("g"), _grp_starts(pool, step))):
            frames[k] += list(range(f0 + b, f0 + e))
    images = [pool.images[f] if pool.ok[f] else None for fs in frames for f in fs]
    ends = np.cumsum([0] + [len(fs) for fs in frames])
    return gr.reduce_groups(images, list(zip(ends[:-1], ends[1:])), x, y, rw, rh, pix=pool.bits // 8)


def _grp_expect(pool, prm):
    """Every group from gproject_ref (a group without frames holds the empty projection, which a call that does not
    accumulate writes and one that does leaves as it is).  The last part of a continuation over the whole pool is the
    one-call reference."""
    import gproject_ref as gr
    f0, n = frames_of(pool, prm)
    x, y, rw, rh = window_of(pool, prm)
    red = _grp_reduce(pool, prm, parts_of(prm, f0, n))
    if prm.get("acc") is not None and prm["acc_from"] == 0 and f0 + n == pool.n:
        whole = gr.reduce_groups(images_or_none(pool, 0, pool.n), gr.group_ranges(pool.n, prm.get("g"), prm.get("starts")),
                                 x, y, rw, rh, pix=pool.bits // 8)
        assert all(np.array_equal(whole[k], red[k]) for k in whole), "the parts do not add up to the one-call reference"
        red = whole
    want = {}
    for s in prm.get("stats", ALL4):
        if s in ("max", "min"):
            want[s] = as_pix(red[s], pool.bits)
        elif s == "sum":
            want[s] = red[s].astype(np.uint16).view(np.int16) if prm.get("sum16") else red[s].astype(np.uint32).view(np.int32)
        else:
            want[s] = red[s].astype(np.int64)
    return dict(want, group_counts=red["counts"].astype(np.int32), results=rows_array(pool.rows[f0:f0 + n]))


def _grp_plan(pool, prm):
    dv = dvm()
    f0, n = frames_of(pool, prm)
    x, y, rw, rh = window_of(pool, prm)
    fn = dv.project_groups_plan if pool.bits == 8 else dv.project_groups16_plan
    pl = fn(pool.W, pool.H, n, x, y, rw, rh, group_frames=prm.get("g"), has_group_starts=prm.get("starts") is not None,
            n_groups=_grp_groups(pool, prm), stats=prm.get("stats", ALL4),
            sum_dtype=dv.SUM_U16 if prm.get("sum16") else dv.SUM_U32, accumulate=continues(prm))
    pl["index"] = index_of_roi_plan(pool.bits, n, pl)
    return pl


# decode_mask ----------------------------------------------------------------------------------------------------------
def _mask_maps(pool):
    """Per-pixel lo / hi maps in frame coordinates (unsigned host arrays): bands of every width, lo > hi among them."""
    top = (1 << pool.bits) - 1
    rng = np.random.default_rng(pool.W * 29 + pool.H * 3 + pool.bits)
    lo = rng.integers(0, top // 2 + 1, (pool.H, pool.W))
    hi = np.clip(lo + rng.integers(-(top // 8) - 1, top // 2 + 1, (pool.H, pool.W)), 0, top)
    dt = np.uint8 if pool.bits == 8 else np.uint16
    return lo.astype(dt), hi.astype(dt)


def _mask_maps_dev(pool):
    import torch
    npd = np.uint8 if pool.bits == 8 else np.int16
    return const(("mask_maps", pool.W, pool.H, pool.bits),
                 lambda: tuple(torch.from_numpy(np.ascontiguousarray(m).view(npd)).cuda() for m in _mask_maps(pool)))


def _mask_outputs(pool, prm):
    f0, n = frames_of(pool, prm)
    x, y, rw, rh = window_of(pool, prm)
    spec = dict(words=((n, rh, (rw + 63) // 64), "int64"), counts=((n,), "int32"))
    if prm.get("boxes"):
        spec["boxes"] = ((n, 4), "int32")
    return dict(spec, **results_spec(n))


def _mask_run(codec, pool, prm, out):
    dv = dvm()
    x, y, rw, rh = window_of(pool, prm)
    lo, hi = _mask_maps_dev(pool) if prm.get("maps") else band_of(pool, prm)
    fn = codec.decode_mask if pool.bits == 8 else codec.decode_mask16
    fn(*stream_args(pool, prm), x, y, rw, rh, lo=lo, hi=hi, outside=bool(prm.get("outside")), origins=origins_dev(pool, prm),
       mask=dv.Mask(out["words"].t, out["counts"].t, out["boxes"].t if prm.get("boxes") else None, rw=rw),
       results=out["results"].t)


def _mask_expect(pool, prm):
    """mask_ref's words, counts and boxes; a rejected frame leaves its words alone, counts 0 and has the empty box."""
    import mask_ref
    f0, n = frames_of(pool, prm)
    x, y, rw, rh = window_of(pool, prm)
    lo, hi = _mask_maps(pool) if prm.get("maps") else band_of(pool, prm)
    mode = mask_ref.OUTSIDE if prm.get("outside") else mask_ref.INSIDE
    words, counts, boxes = mask_ref.expected(images_or_zero(pool, f0, n), x, y, rw, rh, lo, hi, mode, origins_of(pool, prm))
    words, counts = words.view(np.int64), counts.view(np.int32).copy()
    for k in range(n):
        if not pool.ok[f0 + k]:
            words[k], counts[k], boxes[k] = FILLS["int64"], 0, (rw, rh, -1, -1)
    want = dict(words=words, counts=counts, results=rows_array(pool.rows[f0:f0 + n]))
    if prm.get("boxes"):
        want["boxes"] = boxes
    return want


# decode_patches -------------------------------------------------------------------------------------------------------
def _patch_fill(pool, prm):
    return prm.get("fill", 0) & ((1 << pool.bits) - 1)


def _patch_outputs(pool, prm):
    f0, n = frames_of(pool, prm)
    pw, ph = PATCH
    K = PATCHES_PER_FRAME
    return dict(out=((n, K, ph, pw), pix_dtype(pool.bits)), used=((n, K, 2), "int32"), **results_spec(n))


def _patch_run(codec, pool, prm, out):
    dv = dvm()
    buf, lead, total, offs, W, H, n = stream_args(pool, prm)
    pw, ph = PATCH
    org, cnt = _patch_inputs(pool, prm)
    fn = "decode_patches" if pool.bits == 8 else "decode_patches16"
    if n == 0:     # (the wrapper would hand the call the address of an empty origins tensor: none)
        rc = getattr(codec.L, ("dbde_hip_" if pool.bits == 8 else "dbde16_hip_") + "decode_patches")(
            codec.h, buf.data_ptr() + lead, total, offs.data_ptr(), W, H, 0, pw, ph, PATCHES_PER_FRAME, org.data_ptr(),
            cnt.data_ptr() if cnt is not None else None, dv.patch_edge_mode(prm.get("edge", "clamp")), _patch_fill(pool, prm),
            out["out"].t.data_ptr(), out["used"].t.data_ptr(), None)
        return codec._check(rc, fn)
    getattr(codec, fn)(buf, lead, total, offs, W, H, n, pw, ph, org, counts=cnt, edge=prm.get("edge", "clamp"),
                       fill=_patch_fill(pool, prm), out=out["out"].t, used=out["used"].t, results=out["results"].t)


def _patch_expect(pool, prm):
    import patch_ref
    f0, n = frames_of(pool, prm)
    pw, ph = PATCH
    px = pix_dtype(pool.bits)
    mode = patch_ref.CLAMP if prm.get("edge", "clamp") == "clamp" else patch_ref.FILL
    got, used, live = patch_ref.expected(images_or_none(pool, f0, n), pool.W, pool.H, pw, ph, patch_origins_of(pool, prm),
                                         patch_counts_of(pool, prm), mode, _patch_fill(pool, prm),
                                         untouched=FILLS[px] & ((1 << pool.bits) - 1),
                                         dtype=np.uint8 if pool.bits == 8 else np.uint16)
    used[~live] = FILLS["int32"]
    return dict(out=as_pix(got, pool.bits), used=used, results=rows_array(pool.rows[f0:f0 + n]))


def _patch_plan(fn8, fn16):
    def plan(pool, prm):
        dv = dvm()
        f0, n = frames_of(pool, prm)
        pl = getattr(dv, fn8 if pool.bits == 8 else fn16)(pool.W, pool.H, n, *PATCH, PATCHES_PER_FRAME, prm.get("edge", "clamp"))
        pl["index"] = index_of_roi_plan(pool.bits, n, pl)
        return pl
    return plan


# patch_moments --------------------------------------------------------------------------------------------------------
def _mom_outputs(pool, prm):
    f0, n = frames_of(pool, prm)
    K = PATCHES_PER_FRAME
    spec = dict(moments=((n, K, 8), "int64"), used=((n, K, 2), "int32"))
    if prm.get("bbox"):
        spec["boxes"] = ((n, K, 4), "int32")
    return dict(spec, **results_spec(n))


def _mom_run(codec, pool, prm, out):
    buf, lead, total, offs, W, H, n = stream_args(pool, prm)
    org, cnt = _patch_inputs(pool, prm)
    lo, hi = band_of(pool, prm)
    fn = codec.patch_moments if pool.bits == 8 else codec.patch_moments16
    fn(buf, lead, total, offs, W, H, n, *PATCH, org if n else org[:0], lo, hi, weight=prm.get("weight", "above"), counts=cnt,
       edge=prm.get("edge", "clamp"), out=out["moments"].t, bbox=out["boxes"].t if prm.get("bbox") else None,
       used=out["used"].t, results=out["results"].t)


def _mom_expect(pool, prm):
    import moments_ref
    import patch_ref
    f0, n = frames_of(pool, prm)
    lo, hi = band_of(pool, prm)
    mode = patch_ref.CLAMP if prm.get("edge", "clamp") == "clamp" else patch_ref.FILL
    mom, box, used, live = moments_ref.expected(images_or_none(pool, f0, n), pool.W, pool.H, *PATCH, patch_origins_of(pool, prm),
                                                patch_counts_of(pool, prm), mode, lo, hi,
                                                moments_ref.WEIGHTS.index(prm.get("weight", "above")))
    mom[~live] = FILLS["int64"]
    box[~live] = FILLS["int32"]
    used[~live] = FILLS["int32"]
    want = dict(moments=np.array(mom.tolist(), np.int64).reshape(n, PATCHES_PER_FRAME, 8), used=used.astype(np.int32),
                results=rows_array(pool.rows[f0:f0 + n]))
    if prm.get("bbox"):
        want["boxes"] = box.astype(np.int32)
    return want


# project_weighted -----------------------------------------------------------------------------------------------------
def _wp_weights(pool, prm):
    """(R, pool.n) float32: the weights of the pool's frames (a step takes the columns of its own)."""
    import wproject_gpu as wg
    R = prm.get("R", 1)
    return wg.family(np.random.default_rng(pool.n * 31 + R), "normal", R, pool.n)


def _wp_weights_dev(pool, prm):
    """The step's columns of the device weights: a view whose rows lie pool.n (strided: pool.n + 7, NaN between them)
    apart; for a call without frames the column of one frame, which is never read."""
    import torch
    import wproject_gpu as wg
    w = _wp_weights(pool, prm)
    make = (lambda: wg.strided(w)) if prm.get("strided") else (lambda: torch.from_numpy(w).cuda())
    dev = const(("weights", pool.n, prm.get("R", 1), bool(prm.get("strided"))), make)
    f0, n = frames_of(pool, prm)
    return dev[:, f0:f0 + max(n, 1)]


def _wp_outputs(pool, prm):
    f0, n = frames_of(pool, prm)
    x, y, rw, rh = window_of(pool, prm)
    return dict(out=((prm.get("R", 1), rh, rw), "int32"), count=((1,), "int64"), **results_spec(n))


def _wp_run(codec, pool, prm, out):
    import torch
    dv = dvm()
    fn = codec.project_weighted if pool.bits == 8 else codec.project_weighted16
    fn(*stream_args(pool, prm), _wp_weights_dev(pool, prm), *window_of(pool, prm),
       out=dv.WeightedProjection(out["out"].t.view(torch.float32), out["count"].t), accumulate=continues(prm),
       one_segment=bool(prm.get("one")), results=out["results"].t)


def _wp_plan_for(pool, prm, n, n_cu):
    dv = dvm()
    x, y, rw, rh = window_of(pool, prm)
    fn = dv.wproject_plan if pool.bits == 8 else dv.wproject16_plan
    stride = (pool.n + 7 if prm.get("strided") else pool.n) if prm.get("R", 1) > 1 else max(n, 1)
    return fn(pool.W, pool.H, n, x, y, rw, rh, regressors=prm.get("R", 1), n_cu=n_cu, one_segment=bool(prm.get("one")),
              weight_stride=stride)


def _wp_expect(pool, prm):
    """The defined value (include/dbde_hip.h) as wproject_ref computes it, bit for bit: per call the chain of fused
    multiply-adds of every segment the plan reports for this device, the partials added in order -- and, in a
    continuation, added to what the parts before left, each part by its own plan."""
    import wproject_ref as wr
    f0, n = frames_of(pool, prm)
    x, y, rw, rh = window_of(pool, prm)
    w = _wp_weights(pool, prm)
    value, count = None, 0
    for a, m in parts_of(prm, f0, n):
        pl = _wp_plan_for(pool, prm, m, device_cus()) if m else dict(segments=1, frames_per_segment=0)
        value, c = wr.wproject(images_or_none(pool, a, m), w[:, a:a + m], x, y, rw, rh, segments=pl["segments"],
                               fps=pl["frames_per_segment"], accumulate=value is not None, prior=value)
        count += c
    return dict(out=wr.bits(value), count=np.array([count], np.int64), results=rows_array(pool.rows[f0:f0 + n]))


def _wp_plan(pool, prm):
    f0, n = frames_of(pool, prm)
    pl = _wp_plan_for(pool, prm, n, 256)
    pl["index"] = index_of_roi_plan(pool.bits, n, pl)
    return pl


for _b in (8, 16):
    _s = suffix(_b)
    OPS["project_groups" + _s] = Op("project_groups" + _s, _b, "consumer", _grp_run, _grp_expect, _grp_plan, _grp_outputs,
                                    prepare=lambda codec, pool, prm: _grp_starts_dev(pool, prm))
    OPS["decode_mask" + _s] = Op("decode_mask" + _s, _b, "consumer", _mask_run, _mask_expect,
                                 roi_family_plan("mask_plan", "mask16_plan"), _mask_outputs,
                                 prepare=lambda codec, pool, prm: (origins_dev(pool, prm),
                                                                   _mask_maps_dev(pool) if prm.get("maps") else None))
    OPS["decode_patches" + _s] = Op("decode_patches" + _s, _b, "consumer", _patch_run, _patch_expect,
                                    _patch_plan("patches_plan", "patches16_plan"), _patch_outputs,
                                    prepare=lambda codec, pool, prm: _patch_inputs(pool, prm))
    OPS["project_weighted" + _s] = Op("project_weighted" + _s, _b, "consumer", _wp_run, _wp_expect, _wp_plan, _wp_outputs,
                                      prepare=lambda codec, pool, prm: _wp_weights_dev(pool, prm))
    OPS["patch_moments" + _s] = Op("patch_moments" + _s, _b, "consumer", _mom_run, _mom_expect,
                                   _patch_plan("patch_moments_plan", "patch_moments16_plan"), _mom_outputs,
                                   prepare=lambda codec, pool, prm: _patch_inputs(pool, prm))


# ---- interveners: a call with no frames, for every consumer --------------------------------------------------------
def _zero_op(base):
    """The consumer `base` with n_frames = 0 (an empty tensor has no address, so the call is handed the buffers of one
    frame): it returns at once and writes nothing -- but for project, project_weighted and histogram, which, not
    accumulating, write their empty result: max 0, min the top value, sums, planes, totals and counts 0."""
    zero = lambda prm: dict(prm, n=0, f0=0)    # noqa: E731
    one = lambda prm: dict(prm, n=1, f0=0)     # noqa: E731
    written = {"project": ALL4 + ("count",), "histogram": ("total", "count"),
               "project_weighted": ("out", "count")}.get(base.name.replace("16", ""), ())

    def expect(pool, prm):
        want = {k: filled(v[0], v[1]) for k, v in base.outputs(pool, one(prm)).items()}
        empty = base.expect(pool, zero(prm)) if written else {}
        return dict(want, **{k: empty[k] for k in written if k in want})

    return Op("zero:" + base.name, base.bits, "zero:" + base.name,
              lambda codec, pool, prm, out: base.run(codec, pool, zero(prm), out), expect,
              lambda pool, prm: {k: v for k, v in base.plan(pool, zero(prm)).items() if k != "index"},
              lambda pool, prm: base.outputs(pool, one(prm)), prepare=base.prepare)


# ---- interveners: calls that must return an error and change nothing -----------------------------------------------
def _err_window_run(codec, pool, prm, out):
    x, y, rw, rh = window_of(pool, prm)
    codec.decode_roi(*stream_args(pool, prm), pool.W - rw + 1, y, rw, rh, out=out["out"].t, results=out["results"].t)


def _err_crop_run(codec, pool, prm, out):
    slot, cap = _crop_cap(pool, prm)
    c = out["out"]
    codec.crop_frames(*stream_args(pool, prm), *window_of(pool, prm), c.flat, c.lo, cap - 1, slot_stride=slot,
                      out_offsets=out["offsets"].t, out_bytes=out["nbytes"].t, origins_used=out["used"].t,
                      results=out["results"].t)


def _err_project_run(codec, pool, prm, out):
    dv = dvm()
    codec.project(*stream_args(pool, prm), *window_of(pool, prm), out=dv.Projection(count=out["count"].t),
                  results=out["results"].t)


def _untouched(outputs):
    return lambda pool, prm: {k: filled(v[0], v[1]) for k, v in outputs(pool, prm).items()}


def _no_plan(pool, prm):
    return {}


for _name in CONSUMERS:
    OPS["zero:" + _name] = _zero_op(OPS[_name])

OPS["err:window"] = Op("err:window", 8, "err:window", _err_window_run, _untouched(_roi_outputs), _no_plan, _roi_outputs,
                       raises=True)
OPS["err:crop_capacity"] = Op("err:crop_capacity", 8, "err:crop_capacity", _err_crop_run, _untouched(_crop_outputs),
                              _no_plan, _crop_outputs, raises=True)
_err_proj_outputs = lambda pool, prm: dict(count=((1,), "int64"), **results_spec(frames_of(pool, prm)[1]))   # noqa: E731
OPS["err:project_no_statistic"] = Op("err:project_no_statistic", 8, "err:project_no_statistic", _err_project_run,
                                     _untouched(_err_proj_outputs), _no_plan, _err_proj_outputs, raises=True)


# one per newer family: what the family's own argument-error test establishes as DBDE_HIP_ERR_ARG of the C call itself
def _err_groups_run(codec, pool, prm, out):
    """U16 sums cannot be continued."""
    dv = dvm()
    codec.project_groups(*stream_args(pool, prm), *window_of(pool, prm), group_frames=prm["g"], accumulate=True,
                         out=dv.GroupProjection(sum=out["sum"].t, counts=out["group_counts"].t), results=out["results"].t)


def _err_mask_run(codec, pool, prm, out):
    """No output requested (the wrapper refuses that by itself: the C call is made directly)."""
    buf, lead, total, offs, W, H, n = stream_args(pool, prm)
    lo, hi = band_of(pool, prm)
    rc = codec.L.dbde_hip_decode_mask(codec.h, buf.data_ptr() + lead, total, offs.data_ptr(), W, H, n, *window_of(pool, prm),
                                      None, 0, None, lo, None, hi, None, None, None, out["results"].t.data_ptr())
    codec._check(rc, "dbde_hip_decode_mask")


def _err_patches_run(codec, pool, prm, out):
    """An unknown edge mode."""
    _patch_run(codec, pool, dict(prm, edge=2), out)


def _err_weighted_run(codec, pool, prm, out):
    """Nine regressors (the wrapper would make two calls of them: the C call is made directly)."""
    buf, lead, total, offs, W, H, n = stream_args(pool, prm)
    w = _wp_weights_dev(pool, prm)
    rc = codec.L.dbde_hip_project_weighted(codec.h, buf.data_ptr() + lead, total, offs.data_ptr(), W, H, n,
                                           *window_of(pool, prm), w.data_ptr(), 9, w.stride(0), 0, 0,
                                           out["out"].t.data_ptr(), out["count"].t.data_ptr(), out["results"].t.data_ptr())
    codec._check(rc, "dbde_hip_project_weighted")


def _err_moments_run(codec, pool, prm, out):
    """A patch of 513 rows in fill mode."""
    buf, lead, total, offs, W, H, n = stream_args(pool, prm)
    org, cnt = _patch_inputs(pool, prm)
    codec.patch_moments(buf, lead, total, offs, W, H, n, PATCH[0], 513, org, *band_of(pool, prm), edge="fill",
                        out=out["moments"].t, bbox=out["boxes"].t, used=out["used"].t, results=out["results"].t)


for _name, _run, _outs, _prep in (
        ("err:groups_u16_accumulate", _err_groups_run, _grp_outputs, None),
        ("err:mask_no_output", _err_mask_run, _mask_outputs, None),
        ("err:patches_edge_mode", _err_patches_run, _patch_outputs, lambda codec, pool, prm: _patch_inputs(pool, prm)),
        ("err:weighted_nine_regressors", _err_weighted_run, _wp_outputs, lambda codec, pool, prm: _wp_weights_dev(pool, prm)),
        ("err:moments_513_rows", _err_moments_run, _mom_outputs, lambda codec, pool, prm: _patch_inputs(pool, prm))):
    OPS[_name] = Op(_name, 8, _name, _run, _untouched(_outs), _no_plan, _outs, prepare=_prep, raises=True)


# ---- interveners: the encoders -------------------------------------------------------------------------------------
class Images:
    """An image set of an encoder form: (n, H, W) host images, the layout, and the oracle's frames of them."""

    def __init__(self, name, bits, W, H, n, slots, residue=0, seed=0):
        self.name, self.bits, self.W, self.H, self.n, self.slots, self.residue = name, bits, W, H, n, slots, residue
        self.images = mixed_images(np.random.default_rng(seed or W * 977 + H * 31 + n), n, H, W, bits)
        self.first = 77
        self.maxf = crop_ref.max_frame_bytes(W, H, bits)
        self.slot = (self.maxf + 255) // 256 * 256 if slots else 0
        self.cap = (n - 1) * self.slot + self.maxf if slots else n * self.maxf
        self._frames = None
        self.T = cr.tiles(W, H)

    def frames(self, oracle):
        if self._frames is None:
            pack = wenc_ref.packer(oracle, self.bits)
            self._frames = [pack(self.first + f, self.images[f]) for f in range(self.n)]
        return self._frames

    def dev(self):
        """The images at their address residue (a view into a larger device buffer)."""
        import torch

        def make():
            px = self.bits // 8
            flat = torch.zeros(self.images.size * px + 64, dtype=torch.uint8, device="cuda")
            v = flat[self.residue: self.residue + self.images.size * px]
            v.copy_(torch.from_numpy(self.images.view(np.uint8).reshape(-1)).cuda())
            return v if px == 1 else v.view(torch.int16)
        return const(("imgs", self.name), make)


ENCODER_FORMS = ("persistent", "small", "tiny", "mid", "frames", "group", "persistent16", "legacy16", "window",
                 "window16")
FORM_KERNEL = {"persistent": 0, "small": 1, "tiny": 2, "mid": 3, "frames": 4, "group": 5}
_images = {}
_oracle = []          # the session's oracle (and DBDE16 oracle), set by pools(): expect() of the encoders packs with it


def image_sets():
    """name -> Images: the smallest ENCODE_CASES row of each 8-bit kernel form, a persistent launch of many more chunks
    (the look-back block grows), the two DBDE16 paths, and the window encoders' pitched sources."""
    if _images:
        return _images
    import test_encode_forms as tef
    best = {}
    for c in tef.ENCODE_CASES:
        k = c[5][0]
        if k not in best or c[0] * c[1] * c[2] < best[k][0] * best[k][1] * best[k][2]:
            best[k] = c
    for form, k in FORM_KERNEL.items():
        W, H, n, layout, residue, _ = best[k]
        _images[form] = Images(form, 8, W, H, n, layout == tef.S, residue)
    W, H, n, layout, residue, _ = best[0]
    _images["persistent_big"] = Images("persistent_big", 8, W, H, 9 * n, layout == tef.S, residue)
    _images["persistent16"] = Images("persistent16", 16, 16, 16, 560, False)
    _images["legacy16"] = Images("legacy16", 16, 16, 16, 12, False)
    _images["window"] = Images("window", 8, 61, 37, 5, False)
    _images["window16"] = Images("window16", 16, 61, 37, 5, False)
    return _images


def encode16_path(W, H, n, resident=RESIDENT, residue=0):
    """Which path dbde16_hip_encode_frames takes (its own condition, restated): "persistent16" -- the 8-bit path's
    persistent encoder with PIX = 2 -- for launches of at least as many 512-tile chunks as the device holds workgroups,
    else "legacy16" (enc16_kernel)."""
    T = cr.tiles(W, H)
    n_chunks = n * ((T + 511) // 512)
    fast_in = W % 8 == 0 and residue % 16 == 0
    raw_in = not fast_in and W >= 8 and residue % 2 == 0
    return "persistent16" if (fast_in or raw_in) and n_chunks >= resident else "legacy16"


def _enc_outputs(pool, prm):
    return dict(out=((pool.cap,), "uint8"), offsets=((pool.n,), "int64"), nbytes=((pool.n,), "int64"))


def _enc_run(codec, pool, prm, out):
    c = out["out"]
    if pool.bits == 8:
        codec.encode_frames(pool.dev(), pool.W, pool.H, pool.n, c.flat, c.lo, pool.cap, first_index=pool.first,
                            slot_stride=pool.slot, offsets=out["offsets"].t, nbytes=out["nbytes"].t)
    else:
        offs, sizes = codec.encode_frames16(pool.dev(), pool.W, pool.H, pool.n, c.flat, c.lo, pool.cap,
                                            first_index=pool.first, slot_stride=pool.slot)
        out["offsets"].t.copy_(offs)
        out["nbytes"].t.copy_(sizes)


def _stream_of(frames, slot, cap):
    want = filled((cap,), "uint8")
    offs, at = [], 0
    for f, fr in enumerate(frames):
        o = f * slot if slot else at
        want[o: o + len(fr)] = fr
        offs.append(o)
        at += len(fr)
    return want, np.array(offs, np.int64), np.array([len(fr) for fr in frames], np.int64)


def _enc_expect(pool, prm):
    want, offs, sizes = _stream_of(pool.frames(_oracle[0]), pool.slot, pool.cap)
    return dict(out=want, offsets=offs, nbytes=sizes)


def _enc_plan(form):
    def plan(pool, prm):
        dv = dvm()
        if pool.bits == 16:
            path = encode16_path(pool.W, pool.H, pool.n)
            assert path == form, f"encode_frames16 of {pool.name} takes the {path} path"
            return dict(lb_chunks=pool.n * ((pool.T + 511) // 512) if path == "persistent16" else None)
        pl = dv.encode_plan(pool.W, pool.H, pool.n, pool.residue, 0, pool.slot)
        assert pl["kernel"] == FORM_KERNEL[form], f"encode_frames of {pool.name} runs kernel {pl['kernel']}"
        pl["lb_chunks"] = pl["n_chunks"] if pl["kernel"] in (0, 1) else None   # the forms that attach the look-back block
        return pl
    return plan


for _form in ("persistent", "small", "tiny", "mid", "frames", "group", "persistent16", "legacy16"):
    OPS["encode:" + _form] = Op("encode:" + _form, 16 if _form.endswith("16") else 8, "encode:" + _form, _enc_run,
                                _enc_expect, _enc_plan(_form), _enc_outputs, prepare=lambda codec, pool, prm: pool.dev())


# window encode: a pitched source (80 x 41 images, rows 96 pixels apart, 64 bytes between frames), a window inside it
WENC = dict(SW=80, SH=41, x=11, y=3, row=96, gap=64)


def _wenc_layout(pool):
    pitch = WENC["row"] * (pool.bits // 8)
    return pitch, WENC["SH"] * pitch + WENC["gap"]


def _wenc_host(pool):
    pitch, stride = _wenc_layout(pool)
    return wenc_ref.embed(list(pool.images), WENC["SW"], WENC["SH"], WENC["x"], WENC["y"], pool.bits, pitch=pitch,
                          frame_stride=stride, fill=0x11)


def _wenc_source(pool):
    def make():
        pitch, stride = _wenc_layout(pool)
        host = _wenc_host(pool)
        return host, wenc_ref.Source(host, 0, WENC["SW"], WENC["SH"], pool.n, pool.bits, pitch=pitch, frame_stride=stride)
    return const(("wenc", pool.name), make)


def _wenc_run(codec, pool, prm, out):
    host, src = _wenc_source(pool)
    c = out["out"]
    fn = codec.encode_window if pool.bits == 8 else codec.encode_window16
    fn(src.view(), c.flat, c.lo, pool.cap, x=WENC["x"], y=WENC["y"], rw=pool.W, rh=pool.H, first_index=pool.first,
       offsets=out["offsets"].t, nbytes=out["nbytes"].t)


def _wenc_expect(pool, prm):
    pack = wenc_ref.packer(_oracle[0], pool.bits)
    pitch, stride = _wenc_layout(pool)
    frames, offs, sizes = wenc_ref.encode_window(pack, _wenc_host(pool), 0, WENC["SW"], WENC["SH"], pitch, stride, pool.n,
                                                 WENC["x"], WENC["y"], pool.W, pool.H, pool.bits, first_index=pool.first)
    want, offs, sizes = _stream_of(frames, 0, pool.cap)
    return dict(out=want, offsets=offs, nbytes=sizes)


def _wenc_plan(pool, prm):
    dv = dvm()
    pitch, stride = _wenc_layout(pool)
    fn = dv.window_encode_plan if pool.bits == 8 else dv.window_encode16_plan
    pl = fn(WENC["SW"], WENC["SH"], pool.n, WENC["x"], WENC["y"], pool.W, pool.H, pitch=pitch, frame_stride=stride)
    assert not pl["forwards"] and pl["pitch"] > WENC["SW"] * (pool.bits // 8), pl
    return pl


for _form, _b in (("window", 8), ("window16", 16)):
    OPS["encode:" + _form] = Op("encode:" + _form, _b, "encode:" + _form, _wenc_run, _wenc_expect, _wenc_plan, _enc_outputs,
                                prepare=lambda codec, pool, prm: _wenc_source(pool))


def _err_encode_run(codec, pool, prm, out):
    c = out["out"]
    codec.encode_frames(pool.dev(), pool.W, pool.H, pool.n, c.flat, c.lo, pool.cap - 1, first_index=pool.first,
                        slot_stride=pool.slot, offsets=out["offsets"].t, nbytes=out["nbytes"].t)


OPS["err:encode_capacity"] = Op("err:encode_capacity", 8, "err:encode_capacity", _err_encode_run, _untouched(_enc_outputs),
                                _no_plan, _enc_outputs, prepare=lambda codec, pool, prm: pool.dev(), raises=True)


# ---- interveners: the stream walks ---------------------------------------------------------------------------------
class Walk:
    """A stream for the walks: back-to-back oracle-packed frames of one geometry, `tail`: "plain", "garbage" (bytes
    that start no frame behind the last one) or "truncated" (the last frame's payload cut short)."""

    def __init__(self, name, W, H, n, tail, seed):
        self.name, self.bits, self.W, self.H, self.n, self.tail = name, 8, W, H, n, tail
        self.images = mixed_images(np.random.default_rng(seed), n, H, W, 8)
        self._built = None
        self.T = cr.tiles(W, H)

    def build(self, oracle):
        if self._built is None:
            frames = [oracle.pack_frame(5 + f, self.images[f], self.W, self.H) for f in range(self.n)]
            T = self.T
            for fr in frames:   # the length the depths give, as test_index_stream_finds_crafted_frames states it
                assert len(fr) == 32 + 2 * T + 8 * int(fr[24:24 + T].sum(dtype=np.int64))
            body = np.concatenate(frames)
            ends = np.cumsum([len(fr) for fr in frames]).astype(np.int64)
            starts = np.concatenate([[0], ends[:-1]]).astype(np.int64)
            self.ends = ends
            found = self.n
            if self.tail == "garbage":
                body = np.concatenate([body, np.full(3 * (32 + 2 * T) + 5, 0xA5, np.uint8)])
            elif self.tail == "truncated":
                body = body[:len(body) - 9]
                found = self.n - 1
            self._built = (np.concatenate([np.zeros(32, np.uint8), body, np.zeros(64, np.uint8)]), len(body), starts, found)
        return self._built

    def dev(self):
        import torch
        return const(("walk", self.name), lambda: torch.from_numpy(self.build(_oracle[0])[0]).cuda())


_walks = {}


def walks():
    if not _walks:
        for tail in ("plain", "garbage", "truncated"):
            _walks["F" + tail] = Walk("F" + tail, 72, 72, 40, tail, seed=72)      # >= 4 worst-case frames: speculative
        _walks["Fshort"] = Walk("Fshort", 72, 72, 3, "plain", seed=73)              # hop by hop
    return _walks


def _walk_outputs(pool, prm):
    m = prm.get("max_frames", pool.n + 4)
    return dict(offsets=((max(m, 1),), "int64"), count=((1,), "int32"))


def _walk_expect(pool, prm):
    buf, nbytes, starts, found = pool.build(_oracle[0])
    m = prm.get("max_frames", pool.n + 4)
    k = min(found, m)
    want = filled((max(m, 1),), "int64")
    want[:k] = starts[:k]
    return {"offsets": want, "offsets:n": k, "count": np.array([k], np.int32)}   # entries from `count` on: unspecified


def _walk_run(codec, pool, prm, out):
    buf, nbytes, starts, found = pool.build(_oracle[0])
    m = prm.get("max_frames", pool.n + 4)
    if prm.get("call", "async") == "sync":      # dbde_hip_index_stream: synchronises by itself
        offs, n = codec.index_stream(pool.dev(), 32, nbytes, pool.W, pool.H, m)
        out["offsets"].t[:n].copy_(offs)
        out["count"].t.fill_(n)
    else:
        codec.index_stream_async(pool.dev(), 32, nbytes, pool.W, pool.H, m, out["offsets"].t, out["count"].t)


def _walk_plan(pool, prm):
    """n_seg of dbde_hip_index_stream_async (restated): the speculative walk from two segments on."""
    buf, nbytes, starts, found = pool.build(_oracle[0])
    n_seg = min(16, nbytes // (2 * (32 + 66 * pool.T)))
    m = prm.get("max_frames", pool.n + 4)
    return dict(n_seg=n_seg, speculative=n_seg >= 2 and m > 0, max_frames=m, present=found, tail=pool.tail,
                stream_bytes=nbytes, max_frame_bytes=32 + 66 * pool.T)


OPS["index_stream"] = Op("index_stream", 8, "index_stream", _walk_run, _walk_expect, _walk_plan, _walk_outputs,
                         prepare=lambda codec, pool, prm: pool.dev())


def _scan_outputs(pool, prm):
    return dict(offsets=((pool.n + 4,), "int64"), count=((1,), "int32"), cursor=((1,), "int64"))


def _scan_run(codec, pool, prm, out):
    buf, nbytes, starts, found = pool.build(_oracle[0])
    out["cursor"].t.zero_()
    codec.scan_ahead(pool.dev(), 32, nbytes, pool.W, pool.H, pool.n + 4, out["cursor"].t, out["offsets"].t, out["count"].t)
    codec.scan_join()


def _scan_expect(pool, prm):
    buf, nbytes, starts, found = pool.build(_oracle[0])
    return dict(_walk_expect(pool, {}), cursor=np.array([int(pool.ends[found - 1])], np.int64))


OPS["scan_ahead"] = Op("scan_ahead", 8, "scan_ahead", _scan_run, _scan_expect, _walk_plan, _scan_outputs,
                       prepare=lambda codec, pool, prm: pool.dev())


# ---- interveners: host-pointer calls, files, timing (they synchronise by themselves and check themselves) -----------
class Host:
    """The frame the host-pointer calls work on: a 61 x 37 image of every depth."""
    name, bits, W, H, n = "host", 8, 61, 37, 1
    image = mixed_images(np.random.default_rng(61), 1, 37, 61, 8)[0]


def _host_run(call):
    def run(codec, pool, prm, out):
        ora = _oracle[0]
        W, H, img = pool.W, pool.H, pool.image
        fr = ora.pack_frame(9, img, W, H)
        if call == "pack_frame":
            assert codec.pack_frame(9, img, W, H).tobytes() == fr.tobytes(), "pack_frame differs from the oracle"
        elif call == "unpack_frame":
            adv, fh, got = codec.unpack_frame(fr, W, H)
            assert (adv, fh) == (len(fr), (2, 9, 0)) and np.array_equal(got, img), "unpack_frame differs"
            bad = cr.break_rule(fr, "n64+1")
            adv, fh, got = codec.unpack_frame(bad, W, H)
            assert adv == 20 and fh[0] == 0xFFFFFFFF and (got == 0xEE).all(), "a rejected frame was unpacked"
        elif call == "unpack_image":
            n, got = codec.unpack_image(fr[20:], W, H)
            assert n == len(fr) - 20 and np.array_equal(got, img), "unpack_image differs"
        elif call == "unpack_image_roi":
            n, got = codec.unpack_image_roi(fr[20:], W, H, 5, 3, 40, 30)
            assert n == len(fr) - 20 and np.array_equal(got, img[3:33, 5:45]), "unpack_image_roi differs"
        elif call == "unpack_8x8":
            rng = np.random.default_rng(8)
            for d in (0, 3, 8):
                packed = cr.payload_bytes(rng, "random", 8 * d)
                got = codec.unpack_8x8(d, 201, packed, 13, np.full(8 * 13 + 16, 0xEE, np.uint8), 2)
                want = ora.unpack_8x8(d, 201, packed, 13, np.full(8 * 13 + 16, 0xEE, np.uint8), 2)
                assert np.array_equal(got, want), ("unpack_8x8 differs", d)
    return run


for _call in ("pack_frame", "unpack_frame", "unpack_image", "unpack_image_roi", "unpack_8x8"):
    OPS["host:" + _call] = Op("host:" + _call, 8, "host:" + _call, _host_run(_call), lambda pool, prm: {}, _no_plan,
                              lambda pool, prm: {})

TMP = [None]     # the directory the file steps write into (run_chain's tmp=)
_serial = [0]


def _file_run(codec, pool, prm, out):
    """FileWriter.put and put_window, then FileReader.next, on the context under test."""
    import torch
    _serial[0] += 1
    path = os.path.join(str(TMP[0]), f"sequence{_serial[0]}.dbde")
    imgs = pool.dev().view(pool.n, pool.H, pool.W)
    host, src = _wenc_source(pool)
    with codec.open_writer(path, pool.W, pool.H, frame_hz=25.0, batch_frames=4) as w:
        w.put(imgs, pool.n, first_index=pool.first)
        w.put_window(src.view(), x=WENC["x"], y=WENC["y"], first_index=pool.first + pool.n)
    got, heads = [], []
    with codec.open_reader(path, batch_frames=3) as r:
        for im, hd in r:
            got.append(im.clone())
            heads.extend(hd)
    assert heads == [(2, pool.first + f, 0) for f in range(2 * pool.n)], heads
    both = torch.cat(got)
    assert torch.equal(both[:pool.n], imgs) and torch.equal(both[pool.n:], imgs), "the file's images differ"
    pack = wenc_ref.packer(_oracle[0], 8)
    want = np.concatenate([_oracle[0].pack_video_header(3, pool.H, pool.W, 25.0)] + pool.frames(_oracle[0])
                          + [pack(pool.first + pool.n + f, pool.images[f]) for f in range(pool.n)])
    assert np.fromfile(path, np.uint8).tobytes() == want.tobytes(), "the file's bytes differ from the oracle's frames"


OPS["file"] = Op("file", 8, "file", _file_run, lambda pool, prm: {}, _no_plan, lambda pool, prm: {},
                 prepare=lambda codec, pool, prm: (pool.dev(), _wenc_source(pool)))


def _timing_run(what):
    def run(codec, pool, prm, out):
        if what == "read":
            t = codec.timing_read()
            assert all(ms >= 0.0 and ms == ms and n >= 0 for ms, n in t.values()), t
            assert sum(n for _, n in t.values()) >= prm.get("launches", 0), t
        else:
            codec.timing(what == "on")
    return run


for _what in ("on", "read", "off"):
    OPS["timing:" + _what] = Op("timing:" + _what, 8, "timing:" + _what, _timing_run(_what), lambda pool, prm: {},
                                _no_plan, lambda pool, prm: {})

INTERVENER_KINDS = tuple(k for k, op in OPS.items() if op.kind != "consumer")


def everything(oracle, o16):
    """name -> pool, image set or walk: whatever a step's pool name can mean."""
    if not _oracle:
        _oracle.extend([oracle, o16])
    return dict(pools(oracle, o16), **image_sets(), **walks(), host=Host)


# ---- the runner ------------------------------------------------------------------------------------------------------

_expected = {}


def key_of(step):
    op, pool, prm = step
    return op, pool, tuple(sorted((k, v if not isinstance(v, (list, dict)) else repr(v)) for k, v in prm.items()))


def expected_dev(things, step):
    """The step's expectations as device tensors: computed and uploaded once per process, never changed."""
    import torch
    k = key_of(step)
    if k not in _expected:
        op, pool, prm = step
        want = OPS[op].expect(things[pool], prm)
        _expected[k] = {name: (a if isinstance(a, (torch.Tensor, int)) else torch.from_numpy(np.ascontiguousarray(a)).cuda())
                        for name, a in want.items()}
    return _expected[k]


def describe(step):
    return f"{step[0]}({step[1]}, {step[2]})" if step else "nothing"


COMPARED = [0, 0]     # outputs and elements compared since the process began (the GPU test requires them to be counted)


def differences(out, want, shared_skip=()):
    """[(output, message)] of everything that differs: values, and the guards."""
    import torch
    bad = []
    for name, c in out.items():
        if name in shared_skip:
            continue
        COMPARED[0] += 1
        COMPARED[1] += c.t.numel()
        if not c.guards_hold():
            bad.append((name, "the guard band around it was written"))
        w = want[name]
        got = c.t
        if name == "results":        # (u64s is a U32 in a U64 slot: only its low half is specified)
            got, w = got.clone(), w.clone()
            got[:, 0] &= 0xFFFFFFFF
            w[:, 0] &= 0xFFFFFFFF
        if name + ":n" in want:              # only the first n elements are specified
            got, w = got[:want[name + ":n"]], w[:want[name + ":n"]]
        if tuple(got.shape) != tuple(w.shape) or got.dtype != w.dtype:
            bad.append((name, f"shape / type {tuple(got.shape)} {got.dtype} != {tuple(w.shape)} {w.dtype}"))
        elif not torch.equal(got, w):
            at = tuple((got != w).nonzero()[0].tolist())
            bad.append((name, f"first differing element {at}: {got[at].item()} != {w[at].item()}"))
    return bad


def run_step(codec, things, step, out):
    """The call itself; an op that must raise is required to."""
    dv = dvm()
    op, pool, prm = step
    if OPS[op].raises:
        try:
            OPS[op].run(codec, things[pool], prm, out)
        except dv.DbdeError:
            return
        raise AssertionError(f"{describe(step)} did not return an error")
    OPS[op].run(codec, things[pool], prm, out)


def outputs_for(things, step, shared):
    """Fresh canvases of a step; the parts of a continuation (prm["acc"]) share all but their results."""
    op, pool, prm = step
    spec = OPS[op].outputs(things[pool], prm)
    if prm.get("acc") is None:
        return make_outputs(spec)
    if prm["acc"] not in shared:
        shared[prm["acc"]] = make_outputs({k: v for k, v in spec.items() if k not in ("results", "counts")})
    return dict(shared[prm["acc"]], **make_outputs({k: v for k, v in spec.items() if k in ("results", "counts")}))


def run_chain(codec, things, name, steps, mode, tmp=None):
    """Runs the chain on `codec` ("stepwise" or "queued") and checks every step; raises AssertionError naming the
    chain, the step, the step before it and the first differing element, after trying the step on a fresh context.
    -> (outputs compared, elements compared)."""
    import torch
    assert mode in ("stepwise", "queued")
    TMP[0] = tmp
    before = list(COMPARED)
    for step in steps:                                    # every input and expectation is on the device beforehand
        op, pool, prm = step
        if OPS[op].prepare:
            OPS[op].prepare(codec, things[pool], prm)
        if hasattr(things[pool], "dev") and op != "file" and not op.startswith("host:"):
            things[pool].dev()
        expected_dev(things, step)
    shared, outs = {}, []
    last_part = {prm["acc"]: i for i, (_, _, prm) in enumerate(steps) if prm.get("acc") is not None}
    if mode == "queued":
        outs = [outputs_for(things, step, shared) for step in steps]
    torch.cuda.synchronize()

    def check(i):
        step = steps[i]
        prm = step[2]
        skip = ()
        if mode == "queued" and prm.get("acc") is not None and last_part[prm["acc"]] != i:
            skip = tuple(shared[prm["acc"]])              # a later part has added to them since
        bad = differences(outs[i], expected_dev(things, step), skip)
        if bad:
            verdict = fresh_verdict(things, steps, i)
            raise AssertionError(
                f"chain {name} ({mode}), step {i} {describe(step)} after {describe(steps[i - 1] if i else None)}: "
                + "; ".join(f"{n}: {m}" for n, m in bad) + f" -- {verdict}")

    for i, step in enumerate(steps):
        if mode == "stepwise":
            outs.append(outputs_for(things, step, shared))
        run_step(codec, things, step, outs[i])
        if mode == "stepwise":
            codec.sync()
            check(i)
    if mode == "queued":
        codec.sync()
        for i in range(len(steps)):
            check(i)
    return COMPARED[0] - before[0], COMPARED[1] - before[1]


def fresh_verdict(things, steps, i):
    """Repeats step i (a continuation: its parts so far) alone on a fresh context; says whether it mismatches there."""
    dv = dvm()
    fresh = dv.Codec(0)
    try:
        prm = steps[i][2]
        todo = [i] if prm.get("acc") is None else [j for j in range(i + 1) if steps[j][2].get("acc") == prm["acc"]]
        shared, out = {}, None
        for j in todo:
            if OPS[steps[j][0]].prepare:
                OPS[steps[j][0]].prepare(fresh, things[steps[j][1]], steps[j][2])
            out = outputs_for(things, steps[j], shared)
            run_step(fresh, things, steps[j], out)
        fresh.sync()
        bad = differences(out, expected_dev(things, steps[i]))
        return ("a fresh context ALSO mismatches (a kernel or reference bug at this shape): " + "; ".join(m for _, m in bad)
                if bad else "a fresh context does NOT mismatch (state carried over from the calls before)")
    finally:
        fresh.close()
