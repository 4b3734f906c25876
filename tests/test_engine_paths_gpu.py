"""Every path through the engine's sampling front end, pinned token for token.

One scenario per mode level (0 greedy, 1 sampling, 2 logit processors, 3 token constraints) walks the first-token path (a
single admission and a batched one, with and without num_prompt_tokens), three graph cycles, a non-speculative step, a cycle
with a slot left out, a free_slot and a final cycle.  Every out_tokens row and the final generated() must equal
tests/golden/engine_sampling_paths.json, recorded by this test on an MI355X from the commit before the sampling state moved
into SlotSampling (QSPEC_RECORD_ENGINE_PATHS=<file> writes instead of comparing; two recordings in separate processes were
identical for every level).  A missing fixture fails."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_sampling_paths.json")
RECORD = os.environ.get("QSPEC_RECORD_ENGINE_PATHS")
GRAPHS = ("_graph", "_graph_s", "_graph_p", "_graph_c")   # the whole-cycle graph of mode level 0 .. 3
B, K = 4, 3


@pytest.fixture(scope="module")
def tiny():
    assert torch.cuda.is_available()
    from qspec_amd.model import QuarotLlamaConfig, QuarotLlamaForCausalLM
    cfg = QuarotLlamaConfig(1024, 3584, 8, 2, 2, 2048, 1e-5, 10000.0, 512, "tiny")
    return QuarotLlamaForCausalLM(cfg, DEV).init_synthetic(seed=0)


def _params(level):
    """slot -> set_sampling_params keywords; each level adds to the one below."""
    p = {b: {} for b in range(B)}
    if level >= 1:
        p[1] = dict(temperature=0.8, top_k=50, top_p=0.9, seed=20261017)
        p[2] = dict(temperature=0.7)
    if level >= 2:
        p[2].update(min_p=0.05, repetition_penalty=1.2, min_tokens=4, stop_token_ids=(3, 5))
    if level >= 3:
        p[3] = dict(logit_bias={7: 4.0, 11: -3.0}, allowed_token_ids=list(range(0, 512, 2)), bad_words_token_ids=[[6, 8]])
    return p


def _run(tiny, level):
    from qspec_amd.spec_decode import QSpecEngine
    rng = np.random.default_rng(17)
    prompts = [rng.integers(0, tiny.config.vocab_size, n).tolist() for n in (5, 9, 17, 33)]
    eng = QSpecEngine(tiny, K, B, max_model_len=256, block_size=16, max_new_tokens=64, use_graph=True, seed=0)
    for b, kw in _params(level).items():
        eng.set_sampling_params(b, **kw)
    rows = []

    def record():
        torch.cuda.synchronize()
        rows.append(eng.out_tokens.cpu().tolist())
    eng.add_sequences_to([0], prompts[:1])                                        # the single-prompt pass
    eng.add_sequences_to([1, 2, 3], prompts[1:], num_prompt_tokens=[None, 16, None])   # slot 2 comes back with 1 output
    rows.append(eng.last_token.cpu().tolist())                                    # the four first tokens
    for _ in range(3):
        eng.step()
        record()
    eng.step_no_spec()
    record()
    eng.step(participants=[1, 2, 3])
    record()
    graphs = [getattr(eng, name) for name in GRAPHS]
    eng.free_slot(1)
    eng.step()
    record()
    # the level's whole-cycle graph and no other, and the same object behind the free_slot: never re-captured
    assert [g is not None for g in graphs] == [i == level for i in range(4)], graphs
    assert all(getattr(eng, name) is g for name, g in zip(GRAPHS, graphs))
    return {"out_tokens": rows, "generated": eng.generated()}


@pytest.mark.parametrize("level", [0, 1, 2, 3])
def test_engine_paths_emit_the_recorded_tokens(tiny, level):
    got = _run(tiny, level)
    if RECORD:
        done = json.load(open(RECORD)) if os.path.exists(RECORD) else {}
        done[f"level{level}"] = got
        with open(RECORD, "w") as f:
            json.dump(done, f, separators=(",", ":"))
        return
    want = json.load(open(GOLDEN))[f"level{level}"]
    assert got["out_tokens"] == want["out_tokens"]
    assert got["generated"] == want["generated"]
