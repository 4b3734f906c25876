"""Logprobs on the GPU: both entry points of csrc/logprobs.hip over the shared case list against the float64 restatement of
the same input values (tests/logprob_cases.py), the engine's prompt and decode forms on the tiny model, and the worker end to
end."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import logprob_cases as lc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def tiny_cfg():
    from qspec_amd.model import QuarotLlamaConfig
    return QuarotLlamaConfig(1024, 3584, 8, 2, 2, 2048, 1e-5, 10000.0, 512, "tiny")


@pytest.fixture(scope="module")
def tiny():
    assert torch.cuda.is_available()
    from qspec_amd.model import QuarotLlamaForCausalLM
    return QuarotLlamaForCausalLM(tiny_cfg(), DEV).init_synthetic(seed=1, lm_head_std=0.05)


def run_kernel(c, canary=None):
    from qspec_amd import ops
    wide = torch.from_numpy(c.wide.copy()).to(DEV)
    x = wide[:, c.off:c.off + c.vocab]
    rows, n = x.shape[0], c.num_top
    lp = torch.full((rows + 1,), 7.0, dtype=torch.float32, device=DEV)        # one entry more: nothing is written past the end
    rank = torch.full((rows + 1,), 77, dtype=torch.int32, device=DEV)
    top = torch.full((rows * n + 1,), 77, dtype=torch.int32, device=DEV)
    tlp = torch.full((rows * n + 1,), 7.0, dtype=torch.float32, device=DEV)
    fn = ops.token_logprobs_from_logits if c.kind == "logits" else ops.token_logprobs_from_probs
    fn(x, torch.from_numpy(c.tokens).to(DEV), n, lp, rank, top if n else None, tlp if n else None)
    torch.cuda.synchronize()
    assert lp[-1].item() == 7.0 and rank[-1].item() == 77 and top[-1].item() == 77 and tlp[-1].item() == 7.0
    assert torch.equal(wide.cpu(), torch.from_numpy(c.wide.copy()))           # the input is only read
    return lc.Result(lp[:rows].cpu().numpy(), rank[:rows].cpu().numpy(), top[:rows * n].cpu().numpy().reshape(rows, n),
                     tlp[:rows * n].cpu().numpy().reshape(rows, n))


@pytest.mark.parametrize("c", lc.cases(), ids=lambda c: c.name)
def test_kernel_equals_the_restatement(c):
    """Ranks exact, top ids exact (ties lowest id first), surplus entries -1 / -inf, tokens outside the vocabulary 0.0 / -1,
    logprobs within 1e-5 + 1e-6 |ref| (probs) or 1e-4 (logits): lc.compare."""
    got, ref = run_kernel(c), lc.reference(c)
    out = (c.tokens < 0) | (c.tokens >= c.vocab)
    assert np.all(got.rank[out] == -1) and np.all(got.logprob[out] == 0.0)
    assert lc.compare(got, ref, c.kind) == []


def torch_expression(probs, ids, num_top):
    """What the worker computed before the kernel (on [rows, V] fp32 probabilities)."""
    logp = torch.log(probs.clamp_min(torch.finfo(torch.float32).tiny))
    sel = logp.gather(-1, ids.unsqueeze(-1)).squeeze(-1)
    ranks = (logp > sel.unsqueeze(-1)).sum(-1) + 1
    top_lp, top_id = logp.topk(num_top, dim=-1)
    return sel.cpu(), ranks.cpu(), top_id.cpu(), top_lp.cpu()


def check_against_torch(got, probs, ids, num_top):
    lp, rank, top, tlp = got
    sel, ranks, top_id, top_lp = torch_expression(probs, ids, num_top)
    assert torch.equal(rank.long().view(-1), ranks.view(-1))
    assert torch.allclose(lp.view(-1), sel.view(-1), rtol=1e-6, atol=1e-5)
    assert torch.allclose(tlp.view(-1, num_top), top_lp.view(-1, num_top), rtol=1e-6, atol=1e-5)
    # ids: equal where the values are untied (torch.topk leaves tie order open); always the same VALUES
    p = probs.cpu()
    assert torch.equal(p.gather(-1, top.long().view(-1, num_top)), p.gather(-1, top_id.view(-1, num_top)))


def make_engine(tiny, **kw):
    from qspec_amd.spec_decode.engine import QSpecEngine
    return QSpecEngine(tiny, 3, 4, max_model_len=256, block_size=16, max_new_tokens=64, use_graph=False, seed=3, **kw)


def test_engine_prompt_logprobs_against_log_softmax(tiny, monkeypatch):
    """add_sequences_to with two prompts of unequal length, one asking for prompt_logprobs=3, and a single prompt that crosses
    the chunk boundary (PROMPT_LOGPROB_ROWS set to 8): against log_softmax of model.compute_logits over the SAME hidden rows
    (captured where the engine hands them to the lm_head), computed here in float64."""
    from qspec_amd.spec_decode.engine import QSpecEngine
    monkeypatch.setattr(QSpecEngine, "PROMPT_LOGPROB_ROWS", 8)
    rng = np.random.default_rng(11)
    V = tiny.config.vocab_size
    prompts = [rng.integers(0, V, n).tolist() for n in (7, 21, 19)]
    eng = make_engine(tiny)
    seen = []
    inner = eng._prompt_logits

    def spy(hs):
        seen.append(hs.clone())
        return inner(hs)
    eng._prompt_logits = spy
    eng.add_sequences_to([0, 1], prompts[:2], prompt_logprobs=[None, 3])
    eng.add_sequence(2, prompts[2], prompt_logprobs=2)
    assert eng.take_prompt_logprobs(0) is None
    assert [h.shape[0] for h in seen] == [8, 8, 4, 8, 8, 2] and eng._plp_logits.shape == (8, V)
    for slot, chunks, n in ((1, seen[:3], 3), (2, seen[3:], 2)):
        lp, rank, top, tlp = eng.take_prompt_logprobs(slot)
        assert eng.take_prompt_logprobs(slot) is None
        T = len(prompts[slot])
        assert lp.shape == (T - 1,) and rank.shape == (T - 1,) and top.shape == (T - 1, n) and tlp.shape == (T - 1, n)
        holder = SimpleNamespace(logits=torch.empty(8, V, dtype=torch.float16, device=DEV))
        logits = torch.cat([tiny.compute_logits(h, holder).clone() for h in chunks])
        ref = lc.ref_token_logprobs(logits.cpu().numpy(), np.asarray(prompts[slot][1:]), n, "logits")
        assert lc.compare(lc.Result(lp.numpy(), rank.numpy(), top.numpy(), tlp.numpy()), ref, "logits") == []
        want = torch.log_softmax(logits.double(), dim=-1).cpu()
        assert torch.allclose(lp.double(), want.gather(-1, torch.tensor(prompts[slot][1:]).unsqueeze(-1)).squeeze(-1), rtol=0, atol=1e-4)
    eng.add_sequence(3, prompts[0], prompt_logprobs=0)
    eng.free_slot(3)
    assert eng.take_prompt_logprobs(3) is None            # free_slot drops what nobody took


def test_engine_decode_forms_against_the_torch_expression(tiny):
    """"first", "no_spec" and "cycle" against the expression the worker evaluated before, on the engine's own probability
    tensors; greedy and sampled slots."""
    rng = np.random.default_rng(12)
    V = tiny.config.vocab_size
    prompts = [rng.integers(0, V, n).tolist() for n in (9, 14, 11)]
    eng = make_engine(tiny)
    eng.set_sampling_params(1, temperature=0.9, top_k=40, top_p=0.95, seed=4)
    eng.add_sequences_to([0, 1], prompts[:2])
    eng.add_sequence(3, prompts[2])
    slots = [0, 1, 3]
    first = eng.gen_tokens[slots, 0]
    probs = torch.stack([eng._first_probs[b][0][eng._first_probs[b][1]] for b in slots])
    check_against_torch(eng.token_logprobs("first", slots, first.tolist(), 4), probs, first, 4)
    got = eng.token_logprobs("first", [3], [first[2].item()], 0)
    assert got[0].shape == (1,) and got[2].shape == (1, 0) and got[1].item() >= 1
    eng.step_no_spec(participants=[0, 3])
    torch.cuda.synchronize()
    tok = eng.out_tokens[[0, 3], 0]
    check_against_torch(eng.token_logprobs("no_spec", [0, 3], tok.tolist(), 5), eng.draft_probs_kbv[0][[0, 3]], tok, 5)
    eng.note_emitted([1, 0, 0, 1])
    eng.step()
    out, err = eng.read_outputs()
    assert err == 0
    ids = out[slots].clamp_min(0).to(DEV)
    got = eng.token_logprobs("cycle", slots, ids.tolist(), 3)
    assert got[0].shape == (3, 4) and got[2].shape == (3, 4, 3)
    check_against_torch(got, eng.target_probs[slots].reshape(-1, V), ids.reshape(-1), 3)
    lp, rank, _, _ = eng.token_logprobs("cycle", [1], [[-1] * 4], 0)      # no token at a position: the dummy entry
    assert torch.all(lp == 0.0) and torch.all(rank == -1)


def _worker(tiny, disable_logprobs):
    from qspec_amd.spec_decode import create_spec_worker
    c = tiny.config
    hf = SimpleNamespace(model_type="llama_quarot", hidden_size=c.hidden_size, intermediate_size=c.intermediate_size,
                         num_attention_heads=c.num_attention_heads, num_key_value_heads=c.num_key_value_heads,
                         num_hidden_layers=c.num_hidden_layers, vocab_size=c.vocab_size, rms_norm_eps=c.rms_norm_eps,
                         rope_theta=c.rope_theta, max_position_embeddings=c.max_position_embeddings)
    cfg = SimpleNamespace(
        model_config=SimpleNamespace(hf_config=hf, max_model_len=256, model="/nonexistent", seed=0, max_logprobs=5),
        cache_config=SimpleNamespace(block_size=16, gpu_memory_utilization=0.9, swap_space_bytes=0),
        scheduler_config=SimpleNamespace(max_num_seqs=2, max_num_batched_tokens=512),
        parallel_config=SimpleNamespace(tensor_parallel_size=1, pipeline_parallel_size=1),
        load_config=SimpleNamespace(load_format="auto"),
        speculative_config=SimpleNamespace(num_speculative_tokens=3, speculative_disable_by_batch_size=None,
                                           disable_log_stats=True, disable_logprobs=disable_logprobs,
                                           draft_token_acceptance_method="rejection_sampler"))
    w = create_spec_worker(vllm_config=cfg, local_rank=0, rank=0, model=tiny)
    w.init_device()
    w.load_model()
    w.initialize_cache(32, 0)
    return w


def test_worker_end_to_end(tiny):
    """disable_logprobs=False with logprobs=2, prompt_logprobs=2: real prompt entries, a real first-token entry, real entries on
    the non-speculative step and in the cycle -- and the same token ids as the same run with disable_logprobs=True, whose
    outputs are the dummies."""
    from qspec_amd.spec_decode import ExecuteModelRequest, Logprob, SamplingParams, SequenceData, SequenceGroupMetadata
    rng = np.random.default_rng(6)
    prompts = [rng.integers(0, tiny.config.vocab_size, n).tolist() for n in (9, 14)]
    runs = {}
    for disable in (False, True):
        w = _worker(tiny, disable)
        sp = SamplingParams(logprobs=2, prompt_logprobs=2)
        sgs = [SequenceGroupMetadata(f"r{i}", True, {i: SequenceData(list(p))}, sampling_params=sp) for i, p in enumerate(prompts)]
        outs = [w.execute_model(ExecuteModelRequest(sgs, num_lookahead_slots=0))]
        for s, tok in zip(sgs, outs[0][0].token_ids()):
            s.seq_data[next(iter(s.seq_data))].output_token_ids.append(tok)
        dec = [SequenceGroupMetadata(s.request_id, False, s.seq_data, sampling_params=sp) for s in sgs]
        outs.append(w.execute_model(ExecuteModelRequest(dec, num_lookahead_slots=0)))
        for s, tok in zip(sgs, outs[1][0].token_ids()):
            s.seq_data[next(iter(s.seq_data))].output_token_ids.append(tok)
        outs.append(w.execute_model(ExecuteModelRequest(dec, num_lookahead_slots=3)))
        runs[disable] = outs
    tokens = {d: [[o.token_ids() for o in step] for step in outs] for d, outs in runs.items()}
    assert tokens[False] == tokens[True]                     # logprobs must not perturb generation
    real, dummy = runs[False], runs[True]
    for i, p in enumerate(prompts):
        plp = real[0][0].outputs[i].prompt_logprobs
        assert len(plp) == len(p) - 1
        for t, d in zip(p[1:], plp):
            assert t in d and 2 <= len(d) <= 3 and all(v.rank >= 1 and v.logprob <= 0.0 for v in d.values())
            assert 1 in [v.rank for v in d.values()]
        assert dummy[0][0].outputs[i].prompt_logprobs == [{t: Logprob(0.0, -1)} for t in p[1:]]
    for step in (real[0][0], real[1][0], real[2][0]):        # first token, non-speculative step, first cycle position
        for o in step.outputs:
            s = o.samples[0]
            e = s.logprobs[s.output_token]
            assert e.rank >= 1 and e.logprob <= 0.0 and 2 <= len(s.logprobs) <= 3 and 1 in [v.rank for v in s.logprobs.values()]
    for outs in dummy:
        for step in outs:
            for o in step.outputs:
                assert o.samples[0].logprobs == {o.samples[0].output_token: Logprob(0.0, -1)}
