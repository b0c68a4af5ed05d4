"""CPU: the chains of calls that tests/test_gpu_context_sequences.py runs on one context, and the proof of what they cover.

CHAINS maps a name to a list of steps (op, pool, params) over the ops and pools of tests/sequences.py.  Nothing here
touches a GPU: from the plan functions (the ones the entry points themselves call) and the pools alone, the tests below
work out the state every step leaves in the context and the state every step meets, and require:

  1. index state: each of the 26 index consumers (sq.CONSUMERS: thirteen families, both pixel sizes) runs directly after
     a call that left chunk_off / frame_ok / idx_ctr (a) written by the other pixel size, (b) by the split index where it
     runs unsplit, (c) the reverse, (d) for more frames, (e) for fewer frames with both calls' 2n words inside one
     idx_ctr allocation (the earlier call's flag words are this call's counters), (f) for another chunks_per_frame, (g)
     with a frame index rejected that is now accepted, (h) the reverse; and every ordered pair of consumers, 676 of
     them, is adjacent somewhere: the 256 pairs of the first sixteen in the de Bruijn walk, the 420 with one of the ten
     newer consumers in them in an Euler circuit cut into two chains.  decode_frames16 never splits its index
     (dbde16_hip_decode_frames passes 1), so (c) and (e) do not exist for it; all eight exist for every other consumer;
  2. the same stale state with calls of other kinds in between, for every consumer, every intervener kind used (a call
     without frames of every consumer and a call that fails after validation of every family that has one among them);
  3. every ordered pair of encoder forms adjacent; persistent -> an odd number of small launches -> persistent; a launch
     that makes the look-back block grow, and one with fewer chunks than the one before it;
  4. the fused decoder's records: growth, a smaller launch after it, another form in between, three of one shape;
  5. projection partials: segments > 1 -> 1 -> > 1, a change of the statistics between two segmented calls, traces and
     projections after each other, traces at two label counts and two batch sizes; and for project_weighted, whose F32
     partials lie in the same workspace, per pixel size: segments > 1 -> 1 -> > 1, two adjacent segmented calls with
     another number of regressors and other workspace_bytes, a segmented project of all four statistics directly
     before and directly after a segmented project_weighted of other workspace_bytes, traces directly before and after
     it (project_groups has no workspace);
  6. continuations: project, project16, histogram, histogram16, project_groups, project_groups16, project_weighted and
     project_weighted16 over a whole pool in three accumulate=True parts each with at least three other families
     between the parts (the weighted expectation is the header's defined value applied part by part, which may differ
     from the one-call value in the last bits: chain_continuations_new);
  7. the stream walks in the order speculative, hop by hop, speculative cut by max_frames, garbage tail, truncated
     tail, speculative again;
  8. every step is accepted by its plan function, the pools have the plan properties they exist for, no chain is
     longer than 300 steps.

Each test fails with the list of what is not covered.
"""
import numpy as np
import pytest

import dbde_video_cpp_amd as dv
import sequences as sq
from test_oracle_u16 import o16   # noqa: F401  (fixture)

ROI_FAMILY = tuple(c for c in sq.CONSUMERS if not c.startswith("decode_frames"))
RELATIONS = "abcdefgh"
# the look-back block's header (attach_lookback in dbde_capi.cpp, restated): two sets of control words, the mode flags
# and the arrival flags of up to 4096 workgroups, rounded up to 4096 bytes
LB_HEADER = (2 * 4 * (16 * 64 + 1024) + 2 * 4 * 4096 + 4095) & ~4095


@pytest.fixture(scope="module", autouse=True)
def built():
    dv.build()


@pytest.fixture(scope="module")
def things(oracle, o16):   # noqa: F811
    return sq.everything(oracle, o16)


def family(op):
    return op[:-2] if op.endswith("16") else op


def bits_of(op):
    return sq.OPS[op].bits


def variant(op, v):
    """The v-th parameter set of a consumer (few distinct ones, so that expectations are shared between chains)."""
    f, b = family(op), bits_of(op)
    table = {
        "decode_frames": [{}],
        "decode_roi": [{}, dict(w=1, org=True)],
        "project": [{}, dict(w=1, stats=("max", "sum"))],
        "traces": [dict(labels="few"), dict(labels="many", stats=("min", "sumsq"))],
        "histogram": [{}, dict(w=1, shift=3, bins=20) if b == 8 else dict(w=1, shift=8, bins=256)],
        "decode_binned": [dict(bin=4), dict(w=1, bin=8), dict(w=1, bin=2)],
        "decode_scaled": [dict(type="f32"), dict(w=1, type="bf16", org=True), dict(type="f16")],
        "crop_frames": [dict(w=1), dict(w=1, org=True, slots=True)],
        "project_groups": [dict(g=4), dict(w=1, g=5, stats=("max", "sum"), sum16=b == 8),
                           dict(w=1, starts=sq.GROUP_STARTS, stats=("min", "sum", "sumsq"))],
        "decode_mask": [dict(band="mid"), dict(w=1, maps=True, outside=True, org=True, boxes=True),
                        dict(w=1, band="tile", org=True, boxes=True)],
        "decode_patches": [dict(edge="clamp"), dict(edge="fill", fill=0x1A5, counts=True)],
        "project_weighted": [dict(R=1), dict(w=1, R=3, strided=True), dict(w=1, R=8, one=True)],
        "patch_moments": [dict(edge="clamp", weight="above", band="tile", bbox=True),
                          dict(edge="fill", weight="value", band="empty", counts=True, bbox=True),
                          dict(edge="fill", weight="count", band="mid", counts=True)],
    }[f]
    return dict(table[v % len(table)])


def consumer_step(op, pool, v=0, **more):
    return (op, pool, dict(variant(op, v), **more))


def de_bruijn(k):
    """A cyclic sequence over range(k) of length k * k in which every ordered pair (i, j) is adjacent exactly once."""
    a, seq = [0] * (2 * k), []

    def db(t, p):
        if t > 2:
            if 2 % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)
    db(1, 1)
    return seq


def intervener_pool(op):
    if op.startswith("zero:"):
        base = op[5:]
        return ("Esplit" if base == "decode_frames" else "A" + str(bits_of(op)))
    return {"decode_self": "Eself", "decode_fused": "Efused", "decode_mid": "Emid", "err:window": "A8",
            "err:crop_capacity": "A8", "err:project_no_statistic": "A8", "err:encode_capacity": "small",
            "err:groups_u16_accumulate": "A8", "err:mask_no_output": "A8", "err:patches_edge_mode": "A8",
            "err:weighted_nine_regressors": "A8", "err:moments_513_rows": "A8",
            "index_stream": "Fplain", "scan_ahead": "Fplain", "file": "window"}.get(
        op, op[7:] if op.startswith("encode:") else "host")


def intervener_step(op, **prm):
    if op.startswith("zero:"):
        prm = dict(variant(op[5:], 0), **prm)
    if op == "err:crop_capacity":
        prm = dict(w=1, **prm)
    prm = dict({"err:groups_u16_accumulate": dict(g=4, stats=("sum",), sum16=True), "err:weighted_nine_regressors": dict(R=9),
                "err:moments_513_rows": dict(bbox=True)}.get(op, {}), **prm)
    return (op, intervener_pool(op), prm)


# ---- the chains --------------------------------------------------------------------------------------------------------

def chain_relations(consumers=sq.OLD_CONSUMERS):
    """For every consumer B, the pairs (stale-making call, B) that give each relation of condition 1."""
    steps = []
    for k, B in enumerate(consumers):
        b = bits_of(B)
        o = 24 - b
        roi, roi_o = ("decode_roi", "decode_roi16") if b == 8 else ("decode_roi16", "decode_roi")
        if B == "decode_frames":
            pairs = [((roi_o, "A16", {}), (B, "Esplit", {})),                              # a
                     ((roi, "A8", {}), (B, "Etable", {})),                                 # b, f
                     ((roi, "D8", {}), (B, "Esplit", {})),                                 # c, f
                     ((roi, "C8", {}), (B, "Esplit", {})),                                 # d
                     ((roi, "A8", {}), (B, "Esplit", {})),                                 # e: 13 frames split, then 36
                     ((B, "Esplit", {}), (B, "Esplit", dict(f0=4)))]                        # g, h
        elif B == "decode_frames16":
            pairs = [((roi_o, "A8", {}), (B, "A16", {})),                                  # a
                     ((roi, "A16", {}), (B, "A16", {})),                                   # b, f
                     ((roi, "C16", {}), (B, "A16", {})),                                   # d
                     ((roi, "A16", {}), (B, "Ar16", {}))]                                  # g, h
        else:
            pairs = [((roi_o, f"A{o}", {}), (B, f"A{b}", {})),                             # a
                     ((roi, f"A{b}", {}), (B, f"D{b}", {})),                               # b, f
                     ((roi, f"D{b}", {}), (B, f"A{b}", {})),                               # c, f
                     ((roi, f"C{b}", {}), (B, f"A{b}", {})),                               # d
                     ((roi, f"A{b}", dict(n=5)), (B, f"A{b}", {})),                        # e
                     ((roi, f"A{b}", {}), (B, f"Ar{b}", {}))]                              # g, h
        for j, ((op0, pool0, prm0), (op1, pool1, prm1)) in enumerate(pairs):
            steps.append(consumer_step(op0, pool0, 0, **prm0))
            steps.append(consumer_step(op1, pool1, (j + k) % 2, **prm1))
    return steps


def chain_walk():
    """A de Bruijn walk over the sixteen consumers (every ordered pair adjacent once: 257 steps), pools and parameter
    sets drawn with a seeded generator."""
    seq = de_bruijn(len(sq.OLD_CONSUMERS))
    return drawn_steps([sq.OLD_CONSUMERS[c] for c in seq + seq[:1]], seed=257)


def drawn_steps(ops, seed):
    """The consumers `ops` in order, pools and parameter sets drawn with a seeded generator."""
    rng = np.random.default_rng(seed)
    steps = []
    for op in ops:
        b = bits_of(op)
        if op == "decode_frames":
            pool, more = [("Esplit", {}), ("Etable", {}), ("Esplit", dict(f0=4))][int(rng.integers(0, 3))]
        elif op == "decode_frames16":
            pool, more = [(f"{g}16", {}) for g in ("A", "Ar", "B", "C", "D")][int(rng.integers(0, 5))]
        else:
            pool, more = [(f"A{b}", {}), (f"Ar{b}", {}), (f"B{b}", {}), (f"C{b}", {}), (f"D{b}", {}), (f"A{b}", dict(n=5)),
                          (f"C{b}", dict(n=13))][int(rng.integers(0, 7))]
        steps.append(consumer_step(op, pool, int(rng.integers(0, 3)), **more))
    return steps


def new_pairs_circuit():
    """A closed walk over the 26 consumers in which every ordered pair with one of the ten newer consumers in it -- the
    420 pairs the de Bruijn walk over the first sixteen does not have -- is adjacent exactly once: an Euler circuit of
    the graph of those pairs (every newer consumer has 26 edges in and 26 out, every older one 10 and 10), by
    Hierholzer's algorithm in a fixed order.  421 entries."""
    new = set(sq.NEW_CONSUMERS)
    todo = {a: [b for b in reversed(sq.CONSUMERS) if a in new or b in new] for a in sq.CONSUMERS}
    stack, circuit = [sq.NEW_CONSUMERS[0]], []
    while stack:
        if todo[stack[-1]]:
            stack.append(todo[stack[-1]].pop())
        else:
            circuit.append(stack.pop())
    circuit.reverse()
    assert len(circuit) == 421 and len(set(zip(circuit, circuit[1:]))) == 420
    return circuit


def chain_walk_new(half):
    """One half of new_pairs_circuit (the halves share the step between them: 211 steps each), pools and parameter sets
    drawn as the walk draws its own."""
    ops = new_pairs_circuit()
    return drawn_steps(ops[:211] if half == 0 else ops[210:], seed=421 + half)


def intervener_kinds_in_order():
    """Every intervener: timing switched on first, read and switched off last; the walks in both forms."""
    kinds = [k for k in sq.INTERVENER_KINDS if not k.startswith("timing:")]
    steps = [intervener_step("timing:on")] + [intervener_step(k) for k in kinds]
    steps.insert(steps.index(intervener_step("index_stream")) + 1, ("index_stream", "Fshort", {}))
    return steps + [intervener_step("timing:read", launches=40), intervener_step("timing:off")]


def chain_interveners():
    """For every consumer: a call that leaves index state of another geometry, calls of other kinds, the consumer."""
    iv = intervener_kinds_in_order()
    per = -(-len(iv) // len(sq.CONSUMERS))
    steps = []
    for k, B in enumerate(sq.CONSUMERS):
        b = bits_of(B)
        stale = "decode_roi" if b == 8 else "decode_roi16"
        steps.append(consumer_step(stale, f"D{b}", 0))
        steps += iv[k * per:(k + 1) * per] or [intervener_step("host:pack_frame")]
        pool = "Esplit" if B == "decode_frames" else f"A{b}"
        steps.append(consumer_step(B, pool, k % 2))
    return steps


def encoder_step(form):
    if form == "persistent_big":
        return ("encode:persistent", "persistent_big", {})
    return ("encode:" + form, form, {})


def chain_encoders():
    """A de Bruijn walk over the ten encoder forms, then the look-back block's cases: persistent launches with one and
    with three small ones between them, a persistent launch of nine times the chunks (the block grows), fewer after."""
    seq = de_bruijn(len(sq.ENCODER_FORMS))
    forms = [sq.ENCODER_FORMS[c] for c in seq + seq[:1]]
    forms += ["persistent", "small", "persistent", "small", "small", "small", "persistent", "persistent_big", "small",
              "persistent", "persistent16", "small", "persistent16"]
    return [encoder_step(f) for f in forms]


def chain_fused():
    f = lambda n: ("decode_fused", "Efused", dict(n=n))   # noqa: E731
    return [f(1), f(6), f(2), ("decode_self", "Eself", {}), f(2), ("decode_mid", "Emid", {}), f(3), f(3), f(3),
            consumer_step("decode_frames", "Esplit"), f(6)]


def chain_partials():
    steps = []
    for b in (8, 16):
        s = "" if b == 8 else "16"
        P, T, C, A = "project" + s, "traces" + s, f"C{b}", f"A{b}"
        steps += [(P, C, {}), (P, C, dict(n=13)), (P, C, {}), (P, C, dict(stats=("max", "sum"))),
                  (P, C, dict(w=1, stats=("min", "sumsq"))), (T, C, dict(labels="few")), (P, C, {}),
                  (T, C, dict(labels="many", n=13)), (T, A, dict(labels="few")), (P, C, dict(stats=("sum",))),
                  (T, C, dict(labels="many"))]
    steps += [("project", "C8", {}), ("project16", "C16", {}), ("project", "C8", dict(stats=("sumsq",))),
              ("traces16", "C16", dict(labels="few")), ("traces", "C8", dict(labels="few"))]
    # the weighted projections' F32 partials lie in the same workspace
    for b in (8, 16):
        s = "" if b == 8 else "16"
        P, T, V, C = "project" + s, "traces" + s, "project_weighted" + s, f"C{b}"
        steps += [(V, C, dict(R=3, strided=True)), (V, C, dict(R=8, one=True)), (V, C, dict(R=8)), (V, C, dict(R=1)),
                  (V, C, dict(n=13, R=3)), (V, C, dict(w=1, R=3)), (P, C, {}), (V, C, dict(R=3, strided=True)), (P, C, {}),
                  (T, C, dict(labels="few")), (V, C, dict(w=1, R=8)), (T, C, dict(labels="many"))]
    return steps


def chain_continuations():
    """Four accumulations in three parts each, calls of other families between the parts."""
    cuts = {"C": (0, 100, 200, 300), "A": (0, 4, 9, 13)}
    conts = [("project", "C8", "C", {}), ("histogram", "A8", "A", {}), ("project16", "C16", "C", dict(w=1)),
             ("histogram16", "A16", "A", dict(shift=4, bins=4096))]
    between = [[consumer_step("decode_roi", "D8", 1), consumer_step("traces", "A8", 0), consumer_step("decode_binned16", "B16", 1),
                consumer_step("crop_frames16", "A16", 0)],
               [consumer_step("decode_scaled16", "D16", 1), consumer_step("decode_roi16", "Ar16", 0),
                consumer_step("traces16", "C16", 1, n=13), encoder_step("small"), consumer_step("crop_frames", "Ar8", 1)],
               []]
    steps = []
    for part in range(3):
        for op, pool, cut, prm in conts:
            c = cuts[cut]
            steps.append((op, pool, dict(prm, acc=op, acc_from=0, f0=c[part], n=c[part + 1] - c[part])))
        steps += between[part]
    return steps


def chain_continuations_new():
    """The grouped and the weighted projections over a whole pool in three accumulate=True parts each, calls of other
    families between the parts.  The grouped planes are exact integers: the third part's value is the one-call
    reference (sq._grp_expect asserts that the parts add up to it).  The weighted planes are F32 sums whose defined
    value (include/dbde_hip.h) is ((prior + P_0) + P_1) + ... per call, each call cut into the segments of its own
    plan: three parts round at other places than one call does, so their value may differ from the one-call value in
    the last bits, and the expectation is the definition applied part by part (sq._wp_expect), not the one-call value."""
    cuts = {"C": (0, 100, 200, 300), "A": (0, 4, 9, 13)}
    conts = [("project_groups", "A8", "A", dict(starts=sq.GROUP_STARTS)), ("project_weighted", "C8", "C", dict(w=1, R=3)),
             ("project_groups16", "A16", "A", dict(w=1, starts=sq.GROUP_STARTS, stats=("max", "sum"))),
             ("project_weighted16", "C16", "C", dict(w=1, R=8, strided=True))]
    between = [[consumer_step("decode_mask", "D8", 1), consumer_step("patch_moments16", "A16", 0),
                consumer_step("decode_roi16", "B16", 1), consumer_step("decode_patches", "Ar8", 1)],
               [consumer_step("patch_moments", "C8", 1, n=13), consumer_step("traces16", "A16", 0),
                consumer_step("decode_patches16", "D16", 0), consumer_step("histogram", "A8", 0),
                consumer_step("decode_mask16", "Ar16", 2)],
               []]
    steps = []
    for part in range(3):
        for op, pool, cut, prm in conts:
            c = cuts[cut]
            steps.append((op, pool, dict(prm, acc=op, acc_from=0, cuts=c, f0=c[part], n=c[part + 1] - c[part])))
        steps += between[part]
    return steps


def chain_scan():
    w = lambda pool, **prm: ("index_stream", pool, prm)   # noqa: E731
    return [w("Fplain"), w("Fshort"), w("Fplain", max_frames=17), w("Fgarbage"), w("Ftruncated"), w("Fplain"),
            ("scan_ahead", "Fplain", {}), w("Fplain", call="sync"), ("scan_ahead", "Ftruncated", {}), w("Fgarbage", max_frames=40)]


CHAINS = {"relations": chain_relations(), "walk": chain_walk(), "interveners": chain_interveners(),
          "encoders": chain_encoders(), "fused": chain_fused(), "partials": chain_partials(),
          "continuations": chain_continuations(), "scan": chain_scan(),
          "relations_new": chain_relations(sq.NEW_CONSUMERS[4:5] + sq.NEW_CONSUMERS[:4] + sq.NEW_CONSUMERS[5:]),
          "walk_new1": chain_walk_new(0), "walk_new2": chain_walk_new(1), "continuations_new": chain_continuations_new()}
# the chains that make an encoder, fused or small-encode call: the ones the experiment contexts differ on
EXPERIMENT_CHAINS = tuple(name for name, steps in CHAINS.items()
                          if any(op.startswith(("encode:", "decode_fused", "file", "host:pack_frame")) for op, _, _ in steps))


# ---- what the steps leave and meet ---------------------------------------------------------------------------------

_plans = {}


def plan_of(things, step):
    """The step's plan (worked out once per distinct step: the tests below ask for it many times over)."""
    k = sq.key_of(step)
    if k not in _plans:
        op, pool, prm = step
        _plans[k] = sq.OPS[op].plan(things[pool], prm)
    return _plans[k]


def plans(things, steps):
    return [plan_of(things, step) for step in steps]


def index_launches(things, steps):
    """Per step: None, or the index launch it makes: dict(bits, n, cpf, split, ok), ok the verdict of each frame."""
    out = []
    for (op, pool, prm), pl in zip(steps, plans(things, steps)):
        ix = pl.get("index")
        if ix is not None:
            f0, n = sq.frames_of(things[pool], prm)
            ix = dict(ix, ok=things[pool].ok[f0:f0 + n])
            assert ix["n"] == n and n > 0
        out.append(ix)
    return out


def relations(prev, now, ctr_cap):
    """Which of (a)..(h) hold between the index launch `prev` and the launch `now` that follows it; ctr_cap: idx_ctr's
    capacity after prev."""
    both = min(prev["n"], now["n"])
    return {r for r, holds in (
        ("a", prev["bits"] != now["bits"]),
        ("b", prev["split"] > 1 and now["split"] == 1),
        ("c", prev["split"] == 1 and now["split"] > 1),
        ("d", prev["n"] > now["n"]),
        ("e", prev["n"] < now["n"] and prev["split"] > 1 and now["split"] > 1 and 2 * now["n"] <= ctr_cap),
        ("f", prev["cpf"] != now["cpf"]),
        ("g", any(not prev["ok"][i] and now["ok"][i] for i in range(both))),
        ("h", any(prev["ok"][i] and not now["ok"][i] for i in range(both)))) if holds}


def walk_index_state(things, steps):
    """Yields (i, index launch of step i, the last index launch before it, steps between the two, idx_ctr's capacity
    before step i) for every step that launches the index, from a fresh context on."""
    last, last_at, cap = None, None, 0
    for i, ix in enumerate(index_launches(things, steps)):
        if ix is None:
            continue
        yield i, ix, last, (i - last_at - 1 if last is not None else None), cap
        if ix["split"] > 1:
            cap = sq.grown(cap, 2 * ix["n"])
        last, last_at = ix, i


def applicable(consumer):
    return "abdfgh" if consumer == "decode_frames16" else RELATIONS


def test_index_state_relations(things):
    covered, pairs = set(), set()
    for name, steps in CHAINS.items():
        for i, ix, prev, gap, cap in walk_index_state(things, steps):
            if prev is None or gap != 0:
                continue
            pairs.add((steps[i - 1][0], steps[i][0]))
            for r in relations(prev, ix, cap):
                covered.add((steps[i][0], r))
    missing = [f"{c} never runs directly after index state in relation ({r})" for c in sq.CONSUMERS for r in applicable(c)
               if (c, r) not in covered]
    missing += [f"{a} -> {b} never adjacent" for a in sq.CONSUMERS for b in sq.CONSUMERS if (a, b) not in pairs]
    assert not missing, "\n".join(missing)
    assert len(CHAINS["walk"]) == 257


def kind_of(things, step):
    op, pool, prm = step
    if op == "index_stream":
        return "index_stream:" + ("speculative" if sq.OPS[op].plan(things[pool], prm)["speculative"] else "hop")
    return sq.OPS[op].kind


def all_intervener_kinds():
    return {k for k in sq.INTERVENER_KINDS if k != "index_stream"} | {"index_stream:speculative", "index_stream:hop"}


def test_index_state_survives_interveners(things):
    used, served = set(), set()
    for name, steps in CHAINS.items():
        for i, ix, prev, gap, cap in walk_index_state(things, steps):
            if prev is None or not gap or not relations(prev, ix, cap):
                continue   # nothing between, or the state left is what this call would write anyway
            served.add(steps[i][0])
            used |= {kind_of(things, s) for s in steps[i - gap:i]}
    missing = [f"{c}: no call of another kind between stale index state and it" for c in sq.CONSUMERS if c not in served]
    missing += [f"intervener {k} never sits between a stale-making call and a consumer"
                for k in sorted(all_intervener_kinds() - used)]
    assert not missing, "\n".join(missing)
    assert any(k.startswith("err:") for k in used) and any(k.startswith("zero:") for k in used)


def test_encoder_workspace(things):
    missing = []
    pairs, parity_gaps, grew, fewer = set(), set(), False, False
    for name, steps in CHAINS.items():
        cap, last_chunks, since_persistent = 0, None, None
        pls = plans(things, steps)
        for i, ((op, pool, prm), pl) in enumerate(zip(steps, pls)):
            if not op.startswith("encode:"):
                since_persistent = None
                continue
            form = op[7:]
            if i and steps[i - 1][0].startswith("encode:"):
                pairs.add((steps[i - 1][0][7:], form))
            if pl.get("lb_chunks") is not None:                  # a form that attaches the look-back block
                need = (LB_HEADER + 8 * pl["lb_chunks"] + 15) & ~15
                if cap and need > cap:
                    grew = True
                cap = sq.grown(cap, need)
                if last_chunks is not None and pl["lb_chunks"] < last_chunks:
                    fewer = True
                last_chunks = pl["lb_chunks"]
            if form in ("persistent", "persistent16"):
                if since_persistent is not None:
                    parity_gaps.add(since_persistent)
                since_persistent = 0
            elif form == "small" and since_persistent is not None:
                since_persistent += 1
            else:
                since_persistent = None
    missing += [f"encoder forms {a} -> {b} never adjacent" for a in sq.ENCODER_FORMS for b in sq.ENCODER_FORMS
                if (a, b) not in pairs]
    if not any(g % 2 == 1 for g in parity_gaps):
        missing.append("no persistent -> odd number of small launches -> persistent")
    if not any(g and g % 2 == 0 for g in parity_gaps) and 3 not in parity_gaps:
        missing.append("persistent launches with only one small launch between them: no second spacing")
    if not grew:
        missing.append("no launch makes an allocated look-back block grow")
    if not fewer:
        missing.append("no look-back launch with fewer chunks than the one before it")
    assert not missing, "\n".join(missing)


def test_fused_records(things):
    seen = set()
    for name, steps in CHAINS.items():
        cap, prev_chunks, run, other_since = 0, None, 0, False
        for (op, pool, prm), pl in zip(steps, plans(things, steps)):
            if op != "decode_fused":
                other_since = prev_chunks is not None
                run = 0
                continue
            assert pl["index_mode"] == sq.FUSED
            n = pl["n_chunks"]
            if prev_chunks is not None:
                if n > prev_chunks and n > cap:
                    seen.add("growth")
                if n < prev_chunks:
                    seen.add("smaller after larger")
                if other_since:
                    seen.add("another form between two fused launches")
            run = run + 1 if (n == prev_chunks and not other_since) or run == 0 else 1
            if run >= 3:
                seen.add("three launches of one shape")
            cap, prev_chunks, other_since = sq.grown(cap, n), n, False
    want = {"growth", "smaller after larger", "another form between two fused launches", "three launches of one shape"}
    assert not want - seen, f"fused records: not covered: {sorted(want - seen)}"


def test_partials(things):
    seen = set()
    for name, steps in CHAINS.items():
        pls = plans(things, steps)
        for i in range(1, len(steps)):
            (op0, _, prm0), (op1, _, prm1) = steps[i - 1], steps[i]
            f0, f1 = family(op0), family(op1)
            b = bits_of(op1)
            if f0 == f1 == "project" and bits_of(op0) == b:
                s0, s1 = pls[i - 1]["segments"], pls[i]["segments"]
                if s0 > 1 and s1 == 1:
                    seen.add((b, "segments > 1 then 1"))
                if s0 == 1 and s1 > 1:
                    seen.add((b, "segments 1 then > 1"))
                if s0 > 1 and s1 > 1 and prm0.get("stats", sq.ALL4) != prm1.get("stats", sq.ALL4) \
                        and pls[i - 1]["workspace_bytes"] != pls[i]["workspace_bytes"]:
                    seen.add((b, "statistics change between two segmented calls"))
            if (f0, f1) == ("traces", "project") and bits_of(op0) == b:
                seen.add((b, "project after traces"))
            if (f0, f1) == ("project", "traces") and bits_of(op0) == b:
                seen.add((b, "traces after project"))
            if bits_of(op0) == b and "project_weighted" in (f0, f1):
                s0, s1 = pls[i - 1].get("segments"), pls[i].get("segments")
                w0, w1 = pls[i - 1].get("workspace_bytes"), pls[i].get("workspace_bytes")
                if f0 == f1:
                    if s0 > 1 and s1 == 1:
                        seen.add((b, "weighted: segments > 1 then 1"))
                    if s0 == 1 and s1 > 1:
                        seen.add((b, "weighted: segments 1 then > 1"))
                    if s0 > 1 and s1 == 1 and prm1.get("one") and pls[i]["index"]["n"] == pls[i - 1]["index"]["n"]:
                        seen.add((b, "weighted: one_segment=True directly after a segmented call of as many frames"))
                    if s0 == 1 and s1 > 1 and prm0.get("one") and pls[i]["index"]["n"] == pls[i - 1]["index"]["n"]:
                        seen.add((b, "weighted: a segmented call directly after one_segment=True of as many frames"))
                    if s0 > 1 and s1 > 1 and pls[i - 1]["regressors"] != pls[i]["regressors"] and w0 != w1:
                        seen.add((b, "weighted: the regressors change between two segmented calls"))
                elif "project" in (f0, f1):
                    stats = (prm0 if f0 == "project" else prm1).get("stats", sq.ALL4)
                    if s0 > 1 and s1 > 1 and w0 != w1 and set(stats) == set(sq.ALL4):
                        seen.add((b, "weighted: segmented, directly after a segmented project of all four statistics"
                                  if f0 == "project" else "weighted: segmented, directly before a segmented project of all four statistics"))
                elif "traces" in (f0, f1):
                    seen.add((b, "weighted: after traces" if f0 == "traces" else "weighted: before traces"))
        for (op, pool, prm), pl in zip(steps, pls):
            if family(op) == "traces":
                seen.add((bits_of(op), "labels", pl["n_labels"]))
                seen.add((bits_of(op), "frames", pl["index"]["n"]))
    missing = []
    for b in (8, 16):
        for what in ("segments > 1 then 1", "segments 1 then > 1", "statistics change between two segmented calls",
                     "project after traces", "traces after project", "weighted: segments > 1 then 1",
                     "weighted: segments 1 then > 1", "weighted: the regressors change between two segmented calls",
                     "weighted: one_segment=True directly after a segmented call of as many frames",
                     "weighted: a segmented call directly after one_segment=True of as many frames",
                     "weighted: segmented, directly after a segmented project of all four statistics",
                     "weighted: segmented, directly before a segmented project of all four statistics",
                     "weighted: after traces", "weighted: before traces"):
            if (b, what) not in seen:
                missing.append(f"{b}-bit: {what}")
        for what in ("labels", "frames"):
            if len({s[2] for s in seen if s[:2] == (b, what)}) < 2:
                missing.append(f"{b}-bit traces: fewer than two {what} counts")
    assert not missing, "\n".join(missing)


def test_continuations(things):
    missing = []
    for want in ("project", "project16", "histogram", "histogram16", "project_groups", "project_groups16",
                 "project_weighted", "project_weighted16"):
        found = False
        for name, steps in CHAINS.items():
            parts = [i for i, (op, _, prm) in enumerate(steps) if op == want and prm.get("acc") is not None]
            for key in {steps[i][2]["acc"] for i in parts}:
                at = [i for i in parts if steps[i][2]["acc"] == key]
                if len(at) != 3:
                    continue
                pool = things[steps[at[0]][1]]
                spans = [(steps[i][2]["f0"], steps[i][2]["f0"] + steps[i][2]["n"]) for i in at]
                whole = spans[0][0] == steps[at[0]][2]["acc_from"] == 0 and spans[-1][1] == pool.n and \
                    all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
                others = all(len({family(steps[j][0]) for j in range(a + 1, b)} - {family(want)}) >= 3
                             for a, b in zip(at, at[1:]))
                found |= whole and others
        if not found:
            missing.append(f"{want}: no accumulation over a whole pool in three parts with three other families between them")
    assert not missing, "\n".join(missing)


def test_scan_order(things):
    want = ["speculative", "hop", "speculative cut by max_frames", "speculative garbage", "speculative truncated",
            "speculative"]
    ok = False
    for name, steps in CHAINS.items():
        got = []
        for op, pool, prm in steps:
            if op != "index_stream":
                got.append(None)
                continue
            pl = sq.OPS[op].plan(things[pool], prm)
            what = "speculative" if pl["speculative"] else "hop"
            if pl["max_frames"] < pl["present"]:
                what += " cut by max_frames"
            elif pl["tail"] != "plain":
                what += " " + pl["tail"]
            if pl["speculative"]:
                assert pl["stream_bytes"] >= 4 * pl["max_frame_bytes"] and pl["n_seg"] >= 2, pl
            got.append(what)
        ok |= any(got[i:i + len(want)] == want for i in range(len(got)))
    assert ok, f"no chain walks streams in the order {want}"


def test_table_integrity(things):
    sq.assert_pool_properties(sq.pools(None, None))
    for name, steps in CHAINS.items():
        assert 0 < len(steps) <= 300, (name, len(steps))
        for step, pl in zip(steps, plans(things, steps)):     # a plan function that rejects a step raises here
            op, pool, prm = step
            assert isinstance(pl, dict), step
            spec = sq.OPS[op].outputs(things[pool], prm)
            assert all(int(np.prod(v[0])) >= 0 for v in spec.values()), step
            if sq.OPS[op].kind == "consumer":
                assert things[pool].bits == sq.OPS[op].bits and pl.get("index"), step
    assert set(EXPERIMENT_CHAINS) == {"interveners", "encoders", "fused", "continuations"}, EXPERIMENT_CHAINS
    forms = sq.image_sets()
    assert sq.encode16_path(forms["persistent16"].W, forms["persistent16"].H, forms["persistent16"].n) == "persistent16"
    assert sq.encode16_path(forms["legacy16"].W, forms["legacy16"].H, forms["legacy16"].n) == "legacy16"
