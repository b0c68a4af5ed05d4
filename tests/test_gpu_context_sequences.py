"""GPU: chains of calls of different families on ONE context (tests/sequences.py runs them, tests/test_context_sequences.py
holds the chains and proves what state each step meets).

Every other GPU test module gives each family a context of its own; a client holds one context for days and calls
histogram, then decode_roi on another file, then project, encodes a frame, crops.  Each case here creates a context,
runs one chain on it and closes it, so that a failure reproduces from that case alone: in "stepwise" mode with a
synchronisation and a check after every step, and in "queued" mode with the whole chain enqueued before anything is
checked -- workspaces are then re-laid-out while the call before may still be running.  Chains that reach the
encoders, the fused decoder or the small encoder also run on a context created under DBDE_HIP_EXPERIMENT=81 (bits 0,
4 and 6: forced tickets, the fused decoder's fallback, silent odd chunks of the small encoder), the encoder chain
once more under bit 5 (the DBDE16 encoder's legacy kernel for every DBDE16 launch).  Every comparison is equality.
"""
import pytest

import sequences as sq
from test_context_sequences import CHAINS, EXPERIMENT_CHAINS
from test_gpu_crafted_decode import _codec
from test_oracle_u16 import o16   # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

CONTEXTS = {"default": None, "experiment81": 81, "experiment32": 32}
CASES = [(chain, ctx, mode) for chain in CHAINS for ctx in CONTEXTS for mode in ("stepwise", "queued")
         if ctx == "default" or (ctx == "experiment81" and chain in EXPERIMENT_CHAINS)
         or (ctx == "experiment32" and chain == "encoders" and mode == "queued")]


@pytest.fixture(scope="module")
def dv():
    import dbde_video_cpp_amd as m
    return m


@pytest.fixture(scope="module")
def things(oracle, o16):   # noqa: F811
    return sq.everything(oracle, o16)


@pytest.mark.parametrize("chain,ctx,mode", CASES, ids=["-".join(c) for c in CASES])
def test_chain_on_one_context(dv, things, tmp_path, chain, ctx, mode):
    codec = _codec(dv, CONTEXTS[ctx])
    try:
        outputs, elements = sq.run_chain(codec, things, f"{chain} on the {ctx} context", CHAINS[chain], mode, tmp=tmp_path)
    finally:
        codec.close()
    # (the runner compared something for every step that has outputs: a chain cannot pass by checking nothing)
    with_outputs = [s for s in CHAINS[chain] if sq.OPS[s[0]].outputs(things[s[1]], s[2])]
    assert outputs >= len(with_outputs) and elements > 0, (outputs, elements)
    print(f"{chain} {ctx} {mode}: {len(CHAINS[chain])} steps, {outputs} outputs of {elements} elements compared")


def test_the_runner_sees_one_wrong_element(dv, things):
    """One element of one step's expectation changed: the chain fails at that step, in both modes with the same
    message, and the fresh context -- which cannot match the wrong expectation either -- is reported as mismatching
    too.  Two prefixes: the second ends in a patch_moments step, and the element is one of one moments entry."""
    for chain, output in (("relations", None), ("relations_new", "moments")):
        steps = CHAINS[chain][:4]
        assert output is None or steps[3][0] == "patch_moments"
        codec = _codec(dv)
        try:
            sq.run_chain(codec, things, "pristine", steps, "stepwise")
            want = sq.expected_dev(things, steps[3])
            name = output or next(k for k in want if k != "results")
            kept = want[name]
            want[name] = kept.clone()
            want[name].view(-1)[-1] += 1
            try:
                said = []
                for mode in ("stepwise", "queued"):
                    with pytest.raises(AssertionError, match=r"step 3 .* after .*first differing element.*ALSO mismatches") as e:
                        sq.run_chain(codec, things, "one wrong element", steps, mode)
                    said.append(str(e.value).replace(f"({mode})", "(mode)"))
                assert said[0] == said[1], said
                assert output is None or f"{output}: first differing element" in said[0], said[0]
            finally:
                want[name] = kept
            sq.run_chain(codec, things, "restored", steps, "queued")
        finally:
            codec.close()
