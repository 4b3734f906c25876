"""Logprobs without a GPU: the float64 restatement of tests/logprob_cases.py against CPU torch, the shared comparison against
deliberately faulty variants (in the manner of tests/test_gemm_cases.py), the C ABI's new symbols, and the worker's logic on the
scripted engine of tests/test_worker_cpu.py / the host engine of tests/host_engine.py."""
import ctypes

import numpy as np
import pytest
import torch

import logprob_cases as lc
from host_engine import HostEngine
from test_worker_cpu import FakeEngine, worker_from_vllm_config
from qspec_amd import _lib
from qspec_amd.spec_decode.worker import (ExecuteModelRequest, Logprob, SamplingParams, SequenceData, SequenceGroupMetadata)


# ---------------------------------------------------------------------- the restatement

@pytest.mark.parametrize("c", lc.cases(), ids=lambda c: c.name)
def test_restatement_equals_cpu_torch(c):
    """log_softmax(dtype=float64) / log(clamp_min(tiny)), the _get_ranks expression and torch.topk's VALUES (ids only where the
    values are untied: topk leaves tie order open)."""
    x, ref = torch.from_numpy(lc.case_input(c).copy()), lc.reference(c)
    if c.kind == "logits":
        logp = torch.log_softmax(x, dim=-1, dtype=torch.float64)
    else:
        logp = torch.log(x.clamp_min(torch.finfo(torch.float32).tiny).double())
    tok = torch.from_numpy(c.tokens)
    ok = (tok >= 0) & (tok < c.vocab)
    sel = logp.gather(-1, tok.clamp(0, c.vocab - 1).unsqueeze(-1)).squeeze(-1)
    xs = x.gather(-1, tok.clamp(0, c.vocab - 1).unsqueeze(-1))
    ranks = (x > xs).sum(-1) + 1                                   # _get_ranks (sampler.py:861-879)
    assert torch.equal(torch.where(ok, ranks, torch.full_like(ranks, -1)), torch.from_numpy(ref.rank))
    assert torch.allclose(torch.where(ok, sel, torch.zeros_like(sel)), torch.from_numpy(ref.logprob), rtol=0, atol=1e-12)
    n = min(c.num_top, c.vocab)
    if n:
        top_v, top_i = x.double().topk(n, dim=-1)
        got_v = np.take_along_axis(lc.case_input(c).astype(np.float64), ref.top_ids[:, :n], axis=1)
        assert np.array_equal(top_v.numpy(), got_v)
        ref_lp = torch.from_numpy(ref.top_logprobs[:, :n])
        assert torch.allclose(logp.gather(-1, top_i).nan_to_num(neginf=-1e30), ref_lp.nan_to_num(neginf=-1e30), rtol=0, atol=1e-12)
        for r in range(x.shape[0]):
            v = top_v[r].numpy()
            untied = np.ones(n, dtype=bool)
            untied[1:] &= v[1:] != v[:-1]
            untied[:-1] &= v[:-1] != v[1:]
            below = np.sort(lc.case_input(c)[r].astype(np.float64))[::-1]
            if n < c.vocab and below[n] == v[-1]:   # the last kept value ties with the first dropped one
                untied[-1] = False
            assert np.array_equal(top_i[r].numpy()[untied], ref.top_ids[r, :n][untied])
    assert np.all(ref.top_ids[:, n:] == -1) and np.all(np.isneginf(ref.top_logprobs[:, n:]))


def test_case_list_covers_what_the_kernel_branches_on():
    cs = lc.cases()
    assert {c.vocab for c in cs} == {1, 7, 2048, 2049, 32000, 128256}
    assert {c.wide.shape[0] for c in cs} == {1, 5, 33}
    assert {c.num_top for c in cs} >= {0, 1, 5, 20, 32}
    assert any(c.num_top > c.vocab for c in cs) and any(c.wide.shape[1] > c.vocab for c in cs) and any(c.off for c in cs)
    assert all((c.tokens == -1).sum() == 1 for c in cs) and any((c.tokens >= c.vocab).any() for c in cs)
    big = [c for c in cs if c.vocab == 128256 and "normal" in c.name and c.kind == "logits"][0]
    row = lc.case_input(big)[0]
    assert len(np.unique(row)) < row.size // 4          # many exact ties
    assert any("onehot" in c.name for c in cs) and any("equal" in c.name for c in cs) and any("peaked" in c.name for c in cs)


@pytest.mark.parametrize("fault", ["rank_ge", "ties_high", "lse_stride"])
def test_comparison_rejects_faulty_variants(fault):
    """>= in place of > in the rank, highest-id-first ties, the normaliser over row_stride instead of vocab: each is caught by
    the comparison the GPU test uses, on the shared case list (only cases small enough to keep this quick)."""
    caught = 0
    for c in lc.cases():
        if c.vocab > 32000:
            continue
        bad = lc.ref_token_logprobs(lc.case_input(c), c.tokens, c.num_top, c.kind, fault=fault, wide=c.wide)
        caught += bool(lc.compare(bad, lc.reference(c), c.kind))
        assert lc.compare(lc.reference(c), lc.reference(c), c.kind) == []
    assert caught >= 3


def test_comparison_holds_the_stated_tolerances():
    c = [c for c in lc.cases() if c.name.startswith("probs-v2048-r5")][0]
    ref = lc.reference(c)
    off = ref._replace(logprob=ref.logprob + 3e-5 + 2e-6 * np.abs(ref.logprob))
    assert lc.compare(off, ref, "probs") and not lc.compare(ref._replace(logprob=ref.logprob + 5e-6), ref, "probs")
    c = [c for c in lc.cases() if c.name.startswith("logits-v2048-r5")][0]
    ref = lc.reference(c)
    assert lc.compare(ref._replace(logprob=ref.logprob + 2e-4), ref, "logits")
    assert not lc.compare(ref._replace(logprob=ref.logprob + 5e-5), ref, "logits")


# ---------------------------------------------------------------------- C ABI

def test_new_symbols_are_declared_bound_and_exported():
    names = ("qspec_token_logprobs_from_probs", "qspec_token_logprobs_from_logits")
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in names:
        assert name in _lib.header_symbols() and name in _lib.SIGNATURES and hasattr(lib, name)
    assert "#define QS_MAX_LOGPROBS 32" in open(_lib.HEADER_PATH).read()
    lib = _lib.load()
    one = ctypes.c_void_p(16)   # never dereferenced: the argument checks come first
    for name in names:
        fn = getattr(lib, name)
        assert fn(one, 8, one, 0, 8, 0, one, one, None, None, None) == 0                     # rows == 0: a no-op
        assert fn(one, 8, one, 1, 0, 0, one, one, None, None, None) != 0 and b"vocab" in lib.qspec_last_error()
        assert fn(one, 8, one, 1, 8, 33, one, one, one, one, None) != 0 and b"num_top" in lib.qspec_last_error()
        assert fn(one, 7, one, 1, 8, 0, one, one, None, None, None) != 0 and b"row_stride" in lib.qspec_last_error()


# ---------------------------------------------------------------------- worker logic on a scripted engine

class LogprobEngine(FakeEngine):
    """FakeEngine + the two engine calls the worker's real logprobs come from, scripted: token t has logprob -t / 8, rank
    t % 7 + 1, and the best are ids 900, 901, ... with logprobs -0.5, -1.5, ...; prompt token t: logprob -t / 4, rank 2."""

    def add_sequences_to(self, slots, prompts, block_tables=None, prompt_logprobs=None):
        super().add_sequences_to(slots, prompts, block_tables)
        self.calls.append(("prompt_logprobs", None if prompt_logprobs is None else tuple(prompt_logprobs)))
        self.prompt_results = getattr(self, "prompt_results", {})
        for b, p, n in zip(slots, prompts, prompt_logprobs or [None] * len(slots)):
            if n is not None:
                ids = torch.tensor(p[1:], dtype=torch.float32)
                self.prompt_results[b] = (-ids / 4, torch.full((len(p) - 1,), 2, dtype=torch.int32),
                                          (900 + torch.arange(n, dtype=torch.int32)).repeat(len(p) - 1, 1),
                                          (-0.5 - torch.arange(n, dtype=torch.float32)).repeat(len(p) - 1, 1))

    def take_prompt_logprobs(self, slot):
        return getattr(self, "prompt_results", {}).pop(slot, None)

    def token_logprobs(self, kind, slots, token_ids, num_top=0):
        self.calls.append(("token_logprobs", kind, tuple(slots), num_top))
        ids = torch.as_tensor(token_ids, dtype=torch.int64)
        shape = tuple(ids.shape)
        return (-ids.float() / 8, (ids % 7 + 1).int(), (900 + torch.arange(num_top, dtype=torch.int32)).expand(*shape, num_top),
                (-0.5 - torch.arange(num_top, dtype=torch.float32)).expand(*shape, num_top))


def _requests():
    sp = SamplingParams(logprobs=2, prompt_logprobs=1)
    a = SequenceGroupMetadata("a", True, {1: SequenceData([5, 6, 7])}, sampling_params=sp)
    b = SequenceGroupMetadata("b", True, {2: SequenceData([5, 6, 7, 8])}, sampling_params=SamplingParams())
    return sp, a, b


def test_worker_real_logprobs_on_every_path():
    w, _, _ = worker_from_vllm_config(k=2, disable_logprobs=False)
    w._engine_factory = LogprobEngine
    w.initialize_cache(w.engine.num_blocks, 0)
    sp, a, b = _requests()
    out = w.execute_model(ExecuteModelRequest([a, b], num_lookahead_slots=0))
    assert ("prompt_logprobs", (1, None)) in w.engine.calls and ("token_logprobs", "first", (0, 1), 2) in w.engine.calls
    # prompt step: the scripted prompt logprobs (token, rank 2, + the best one) and the first tokens' real entries
    assert out[0].outputs[0].prompt_logprobs == [{6: Logprob(-1.5, 2), 900: Logprob(-0.5, 1)}, {7: Logprob(-1.75, 2), 900: Logprob(-0.5, 1)}]
    assert out[0].outputs[1].prompt_logprobs is None
    first = out[0].outputs[0].samples[0]
    assert first.output_token == 1000 and first.logprobs == {1000: Logprob(-125.0, 1000 % 7 + 1), 900: Logprob(-0.5, 1), 901: Logprob(-1.5, 2)}
    assert out[0].outputs[1].samples[0].logprobs == {1001: Logprob(-125.125, 1001 % 7 + 1)}     # logprobs=None: the token's own entry
    # speculative step with a rider: cycle entries for a (a position without a token is asked about token 0), no_spec for b
    dec = [SequenceGroupMetadata(s.request_id, False, s.seq_data, sampling_params=s.sampling_params) for s in (a, b)]
    dec[1].num_speculative_tokens = 0
    w.engine.out_script = lambda step, slots: {0: [9, 10, -1]} if step == 0 else None
    outs = w.execute_model(ExecuteModelRequest(dec, num_lookahead_slots=2))
    assert ("token_logprobs", "cycle", (0,), 2) in w.engine.calls and ("token_logprobs", "no_spec", (1,), 0) in w.engine.calls
    assert [o.token_ids() for o in outs] == [[9, 501], [10, -1]]
    assert outs[0].outputs[0].samples[0].logprobs == {9: Logprob(-1.125, 3), 900: Logprob(-0.5, 1), 901: Logprob(-1.5, 2)}
    assert outs[0].outputs[1].samples[0].logprobs == {501: Logprob(-62.625, 501 % 7 + 1)}
    assert outs[1].outputs[1].samples[0].logprobs == {-1: Logprob(0.0, -1)}
    # a non-speculative decode step
    out = w.execute_model(ExecuteModelRequest([dec[0]], num_lookahead_slots=0))
    assert out[0].outputs[0].samples[0].logprobs == {500: Logprob(-62.5, 500 % 7 + 1), 900: Logprob(-0.5, 1), 901: Logprob(-1.5, 2)}


def test_worker_default_keeps_the_dummy_outputs():
    """disable_logprobs=True: the engine is never asked (FakeEngine has neither call nor keyword) and the outputs are today's."""
    w, _, _ = worker_from_vllm_config(k=2)
    sp, a, b = _requests()
    out = w.execute_model(ExecuteModelRequest([a, b], num_lookahead_slots=0))
    assert out[0].outputs[0].prompt_logprobs == [{6: Logprob(0.0, -1)}, {7: Logprob(0.0, -1)}]
    assert out[0].outputs[0].samples[0].logprobs == {1000: Logprob(0.0, -1)}
    w.engine.out_script = lambda step, slots: {0: [9, 10, -1]}
    outs = w.execute_model(ExecuteModelRequest([SequenceGroupMetadata("a", False, a.seq_data, sampling_params=sp)],
                                               num_lookahead_slots=2))
    assert [o.outputs[0].samples[0].logprobs for o in outs] == [{9: Logprob(0.0, -1)}, {10: Logprob(0.0, -1)}]
    out = w.execute_model(ExecuteModelRequest([SequenceGroupMetadata("a", False, a.seq_data, sampling_params=sp)],
                                              num_lookahead_slots=0))
    assert out[0].outputs[0].samples[0].logprobs == {500: Logprob(0.0, -1)}


def test_logprob_caps():
    with pytest.raises(ValueError, match="max_logprobs"):
        _worker_with(max_logprobs=33, disable_logprobs=False)
    _worker_with(max_logprobs=33, disable_logprobs=True)       # the default never computes any: no cap
    w = _worker_with(max_logprobs=5, disable_logprobs=False)
    for sp in (SamplingParams(logprobs=6), SamplingParams(prompt_logprobs=6)):
        with pytest.raises(ValueError, match="max_logprobs"):
            w.execute_model(ExecuteModelRequest([SequenceGroupMetadata("x", True, {1: SequenceData([1, 2, 3])}, sampling_params=sp)]))
        assert w.engine.calls == []          # before anything is enqueued


def _worker_with(max_logprobs, disable_logprobs):
    from types import SimpleNamespace
    from test_worker_cpu import CFG, fake_memory_probe
    from qspec_amd.spec_decode.worker import create_spec_worker
    spec = SimpleNamespace(num_speculative_tokens=2, speculative_disable_by_batch_size=None, disable_log_stats=True,
                           disable_logprobs=disable_logprobs, draft_token_acceptance_method="rejection_sampler")
    w = create_spec_worker(model_config=CFG, model=object(), speculative_config=spec, max_num_seqs=2, max_model_len=256,
                           block_size=16, device="cpu", engine_factory=LogprobEngine, memory_probe=fake_memory_probe,
                           max_logprobs=max_logprobs)
    w.init_device()
    w.initialize_cache(64, 0)
    return w


# ---------------------------------------------------------------------- engine bookkeeping on the host engine

class HostLogprobEngine(HostEngine):
    """HostEngine + scripted results, as an engine holds them between the prompt pass and the worker's read."""

    def keep(self, slot):
        self._prompt_results = self._prompt_results or {}
        self._prompt_results[slot] = (torch.zeros(2), torch.ones(2, dtype=torch.int32), torch.zeros(2, 0, dtype=torch.int32),
                                      torch.zeros(2, 0))
        self._first_probs = self._first_probs or {}
        self._first_probs[slot] = (torch.zeros(1, 64), 0)


def test_engine_hands_prompt_logprobs_over_once_and_free_slot_drops_them():
    e = HostLogprobEngine()
    assert e.take_prompt_logprobs(0) is None and e._lp_dev is None and e._plp_logits is None     # nothing asked: nothing made
    e.free_slot(1)                                   # (an engine that never kept anything)
    e.keep(0)
    e.keep(2)
    assert e.take_prompt_logprobs(0) is not None and e.take_prompt_logprobs(0) is None
    e.free_slot(2)
    assert e.take_prompt_logprobs(2) is None and 2 not in e._first_probs and 0 in e._first_probs
    for bad in (-1, 33):
        with pytest.raises(ValueError, match="logprobs"):
            e._check_num_top(bad)
