"""GPU: every decoder form of tests/test_decode_forms.DECODE_CASES on the crafted streams of tests/crafted.py.

tests/test_gpu_crafted_decode.py feeds the decoders frames no encoder writes, at a handful of geometries.  Here every
row of the coverage table -- each (kernel, copy-out, workgroup size, right margin) the planner offers, each bottom
margin, index mode and unaligned image base per copy-out -- decodes streams that hold the whole pool of that file:
wrapping minima, every (depth, minimum) pair, payloads of all ones, one frame per broken rule (the bad depth in the
last tile of the first chunk) and a DBDE16 frame, mixed, in the row's placement, with arbitrary headers.  A batch
smaller than the pool decodes as many streams as it takes, each with bodies that decode and frames that do not.

Checked per stream: the form at the real image address; every results row and every pixel against the oracle; rejected
frames leave their image's 0xEE untouched; so do the guards in front of and behind the images.  Integer work: no
tolerance.  Rows of the 16-byte staged form also check, on the host, that their streams hold an all-depth-8 chunk and
another one in accepted frames: the kernel chooses between its two copy-outs per chunk, from the chunk's word count.
Mid rows check likewise that some of their groups of frames (the frames one workgroup decodes together) decode whole
and some hold a rejected frame: the staged instance has a copy-out for each.
Fused rows decode once more with the fused index's fallback forced, mid rows with three workgroups walking the batch
(seven groups and more per row: test_decode_forms.test_mid_rows_walk_the_pipelined_loop).
"""
import numpy as np
import pytest

from test_decode_forms import DECODE_CASES, FORM_KEYS, FUSED, MID, case_id, cell_of, mid_groups
from test_gpu_crafted_decode import POOL, Stream, assert_form, check_decode, codecs, decode_into, dv   # noqa: F401

pytestmark = pytest.mark.gpu


def streams_of(oracle, rng, W, H, n, how, chunk_tiles):
    """The streams of a row, until every pool entry has been in one.  Batches of the pool's size and more: the stream
    as test_gpu_crafted_decode builds it (the all-depth-8 frame at eight places in a row), then whatever its shuffle
    left out.  Smaller batches: entries k, k + s, k + 2s, .. of the pool per stream, so that each has valid bodies
    (the pool's first ten) next to frames that do not decode (the rest)."""
    todo = set(range(POOL))
    if n >= POOL:
        s = Stream(oracle, rng, W, H, n, how, chunk_tiles=chunk_tiles)
        todo -= s.used
        yield s
        if todo:
            s = Stream(oracle, rng, W, H, n, how, chunk_tiles=chunk_tiles, select=[0] + sorted(todo))
            todo -= s.used
            yield s
    else:
        step = -(-POOL // n)
        for first in range(step):
            s = Stream(oracle, rng, W, H, n, how, chunk_tiles=chunk_tiles,
                       select=[(first + k * step) % POOL for k in range(n)])
            todo -= s.used
            yield s
    assert not todo, f"pool entries {sorted(todo)} were in no stream"


def chunk_kinds(s, chunk_tiles):
    """(all-depth-8 chunks, other chunks) among the accepted frames of a stream."""
    full = other = 0
    for f, d in enumerate(s.depths):
        if s.images[f] is None:
            continue
        for at in range(0, len(d), chunk_tiles):
            if (d[at: at + chunk_tiles] == 8).all():
                full += 1
            else:
                other += 1
    return full, other


def group_kinds(s, fpw):
    """(groups of fpw frames that all decode, groups with a rejected frame) of a stream."""
    bad = [any(img is None for img in s.images[at: at + fpw]) for at in range(0, s.n, fpw)]
    return len(bad) - sum(bad), sum(bad)


@pytest.mark.parametrize("case", DECODE_CASES, ids=case_id)
def test_decoder_forms_on_crafted_streams(dv, codecs, oracle, case):   # noqa: F811  (the imported fixtures)
    W, H, n, how, residue, form = case
    form = dict(zip(FORM_KEYS, form))
    plan = dv.decode_plan(W, H, n, residue)
    cell = cell_of(W, H, n, residue, plan)
    contexts = ["default"]
    if form["kernel"] == MID:
        contexts.append("three")
    elif form["index_mode"] == FUSED:
        contexts.append("fused")
    rng = np.random.default_rng(W * 65537 + H * 257 + n * 17 + residue)
    full = other = whole = broken = rejected = 0
    for k, s in enumerate(streams_of(oracle, rng, W, H, n, how, plan["chunk_tiles"])):
        rejected += sum(img is None for img in s.images)
        if cell[:2] == ("chunk", "staged16"):
            a, b = chunk_kinds(s, plan["chunk_tiles"])
            full, other = full + a, other + b
        if cell[0] == "mid":
            a, b = group_kinds(s, mid_groups(case)[0])
            whole, broken = whole + a, broken + b
        for name in contexts:
            what = f"{case_id(case)} {cell} (dm {H % 8 or 8}) stream {k} {name}"
            got, rows, addr = decode_into(codecs[name], s, residue)
            assert addr % 256 == residue, f"{what}: images at {addr:#x}"
            assert_form(dv, W, H, n, addr, form)
            assert cell_of(W, H, n, addr, dv.decode_plan(W, H, n, addr)) == cell, what
            check_decode(got, rows, s, what)
    assert rejected >= POOL - 10, f"{case_id(case)}: {rejected} rejected frames"
    if cell[0] == "mid":
        assert whole >= 2 and broken >= 2, f"{case_id(case)}: {whole} groups decode whole, {broken} hold a bad frame"
    if cell[:2] == ("chunk", "staged16"):
        assert full and other, f"{case_id(case)}: {full} all-depth-8 chunks, {other} others: one copy-out never ran"
