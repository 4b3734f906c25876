"""Guided decoding on the host: the restatement against the reference's mask lines run literally, the TokenFSM builders, the
numpy model of the device layout, the refusals, the arena's bookkeeping, the engine's slot state and the worker's recognition of
lowered guided processors (no GPU)."""
import ctypes
import os
import re
import sys
from collections import defaultdict
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guide_cases as gc  # noqa: E402
from host_engine import HostEngine  # noqa: E402

from qspec_amd import _lib  # noqa: E402
from qspec_amd.spec_decode import guides as G  # noqa: E402
from qspec_amd.spec_decode import worker as W  # noqa: E402
from qspec_amd.spec_decode.guides import GuideArena, TokenFSM  # noqa: E402

NEW = ("qspec_process_logits_guided", "qspec_guide_build", "qspec_guide_catch_up")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


# ---------------------------------------------------------------------- the mask arithmetic
def _reference_mask_lines(scores: torch.Tensor, allowed_tokens) -> torch.Tensor:
    """outlines_logits_processors.py:80-92, literally (device = CPU)."""
    mask = torch.full((scores.shape[-1], ), -torch.inf, device=scores.device)
    allowed_tokens = np.array(allowed_tokens, dtype=np.int64)
    allowed_tokens = torch.tensor(allowed_tokens, device=scores.device)
    allowed_tokens = allowed_tokens.masked_select(allowed_tokens < scores.shape[-1])
    mask.index_fill_(0, allowed_tokens, 0)
    scores.add_(mask)
    return scores


def _edge_row(V, seed):
    rng = np.random.default_rng(seed)
    raw = (rng.standard_normal(V) * 4).astype(np.float16)
    special = np.array([0.0, -0.0, 6e-8, -6e-8, 5.96e-8, 6.1e-5, -6.1e-5, 65504.0, -65504.0, 1.0, -1.0], dtype=np.float16)
    raw[rng.permutation(V)[:4 * len(special)]] = np.tile(special, 4)
    return raw


def test_restated_mask_equals_the_reference_lines_bit_for_bit():
    V = 1003
    fsm = gc.random_fsm(V, 4, seed=3, density=0.5)
    for state in range(fsm.num_states):
        raw = _edge_row(V, 10 + state)
        raw[fsm.allowed(state)[0]] = np.float16(-0.0)               # (a -0.0 at an allowed id of every state, the final one too)
        allowed = fsm.allowed(state).tolist() + [V, V + 7]          # ids >= vocab: dropped by the reference's masked_select
        want = _reference_mask_lines(torch.from_numpy(raw.copy()), allowed).numpy()
        got = gc.guide_row(raw, fsm, state)
        assert np.array_equal(_bits(got), _bits(want)), state
        kept = fsm.allowed(state)
        assert np.isneginf(got[np.setdiff1d(np.arange(V), kept)]).all() and np.isfinite(got[kept]).all()
        zeros = kept[raw[kept] == 0]
        assert len(zeros) and not np.signbit(got[zeros]).any()      # -0.0 became +0.0 at the allowed ids
    # the documented divergence: a masked +inf (or NaN) logit is NaN in the reference, -inf here
    raw = _edge_row(V, 99)
    banned = int(np.setdiff1d(np.arange(V), fsm.allowed(0))[0])
    raw[banned] = np.float16(np.inf)
    ref = _reference_mask_lines(torch.from_numpy(raw.copy()), fsm.allowed(0).tolist()).numpy()
    got = gc.guide_row(raw, fsm, 0)
    assert np.isnan(ref[banned]) and np.isneginf(got[banned])
    rest = np.arange(V) != banned
    assert np.array_equal(_bits(got[rest]), _bits(ref[rest]))


# ---------------------------------------------------------------------- builders
def test_from_transitions_renumbers_and_adds_the_final_state():
    f = TokenFSM.from_transitions({70: {5: 10, 9: 70, 200: 10}, 10: {3: -1, 4: None, 6: 999, 2: 70}}, initial=70, eos_token_id=4, vocab=100)
    assert f.num_states == 3 and f.initial == 1 and f.miss == 2                    # keys ascending: 10 -> 0, 70 -> 1, final -> 2
    assert f.allowed(1).tolist() == [5, 9] and f.allowed(0).tolist() == [2, 3, 4, 6]   # 200 >= vocab dropped
    assert [f.next(1, t) for t in (5, 9, 7)] == [0, 1, 2]                          # 7 is not allowed: miss
    assert [f.next(0, t) for t in (2, 3, 4, 6)] == [1, 2, 2, 2]                    # -1, None, an unknown state: final
    assert f.allowed(2).tolist() == [4] and f.next(2, 4) == 2 and f.next(2, 5) == 2
    assert f.advance(f.initial, [5, 2, 9, 9]) == 1 and f.advance(f.initial, [5, 3]) == 2
    assert f.accepts([5, 2, 9]) and not f.accepts([5, 5]) and f.accepts([5, 4, 4])
    g = TokenFSM.from_transitions({0: {1: 0, 7: 5}}, 0, 7, 8)                       # eos always leads to the final state
    assert g.next(0, 7) == g.miss
    with pytest.raises(ValueError):
        TokenFSM.from_transitions({0: {1: 0}}, 0, 8, 8)                             # eos outside the vocabulary
    with pytest.raises(ValueError):
        TokenFSM.from_transitions({0: {9: 0}}, 0, 1, 8)                             # a state left without a token
    with pytest.raises(ValueError):
        TokenFSM.from_transitions({0: {-2: 0}}, 0, 1, 8)


def test_from_token_sequences_builds_the_trie():
    f = TokenFSM.from_token_sequences([[3, 4, 5], [3, 4], [3, 6], [7]], eos_token_id=1, vocab=16)
    assert f.allowed(f.initial).tolist() == [3, 7]
    s34 = f.advance(f.initial, [3, 4])
    assert f.allowed(s34).tolist() == [1, 5]                                        # complete here, or on to 5
    assert f.allowed(f.advance(f.initial, [3])).tolist() == [4, 6]
    for seq in ([3, 4, 5, 1], [3, 4, 1], [3, 6, 1], [7, 1, 1]):
        assert f.accepts(seq), seq
    for seq in ([3, 5], [4], [3, 4, 5, 5], [7, 7], [1]):
        assert not f.accepts(seq), seq
    for bad in ([], [[]], [[1, 2]]):
        with pytest.raises(ValueError):
            TokenFSM.from_token_sequences(bad, 1, 16)


class Generate:
    def __init__(self, tokens):
        self.tokens = tokens


class Write:
    def __init__(self, tokens):
        self.tokens = tokens


_MAPS = {0: {11: 4, 12: 0, 40: 4}, 4: {13: 9, 2: 4}, 9: {14: 0, 15: -1, 2: 9}}    # 4 and 9 are final states: eos = 2 allowed


class _AttrGuide:   # the shape of an Outlines RegexGuide, by attribute
    def __init__(self):
        self.states_to_token_maps, self.initial_state, self.eos_token_id = _MAPS, 0, 2


class _CallGuide:   # the same automaton behind the Guide protocol only
    initial_state = 0

    def get_next_instruction(self, state):
        m = _MAPS.get(state)
        return Write([2, 2, 2]) if m is None else Generate(list(m.keys()))

    def get_next_state(self, state, token_id):
        if token_id == 2 or state not in _MAPS:
            return -1
        n = _MAPS[state].get(token_id)
        return -1 if n is None else n


def _same(a, b):
    return (a.initial, a.miss, a.vocab) == (b.initial, b.miss, b.vocab) and all(
        np.array_equal(x, y) for x, y in ((a.row_ptr, b.row_ptr), (a.tokens, b.tokens), (a.next_states, b.next_states)))


def test_from_guide_attribute_path_breadth_first_path_write_and_cache():
    attr, call = _AttrGuide(), _CallGuide()
    fa, fc = TokenFSM.from_guide(attr, 32), TokenFSM.from_guide(call, 32)
    assert _same(fa, fc) and fa.num_states == 4 and fa.eos_token_id == 2
    assert fa.allowed(0).tolist() == [11, 12] and fa.allowed(fa.miss).tolist() == [2]   # 40 >= vocab dropped; Write: first token only
    assert fa.accepts([12, 11, 13, 14, 11, 2, 2]) and not fa.accepts([11, 11])
    assert TokenFSM.from_guide(attr, 32) is fa and TokenFSM.from_guide(call, 32) is fc  # cached on the object's identity
    assert TokenFSM.from_guide(_AttrGuide(), 32) is not fa and TokenFSM.from_guide(fa, 32) is fa
    assert TokenFSM.from_guide(attr, 64) is not fa                                      # another vocabulary: lowered again
    with pytest.raises(TypeError):
        TokenFSM.from_guide(object(), 32)

    class CFGish(_CallGuide):
        initial_state = SimpleNamespace(parser_state=None)
    with pytest.raises(TypeError, match="int states"):
        TokenFSM.from_guide(CFGish(), 32)

    class Endless(_CallGuide):
        def get_next_instruction(self, state):
            return Write([2]) if state == -1 else Generate([5])

        def get_next_state(self, state, token_id):
            return -1 if state == -1 else state + 1
    with pytest.raises(ValueError, match="states"):
        TokenFSM.from_guide(Endless(), 32)                                              # the state cap


def test_numpy_model_of_the_device_layout_against_dictionary_lookup():
    V, S = 1003, 40
    rng = np.random.default_rng(5)
    maps = {}
    for s in range(S):
        toks = np.nonzero(rng.random(V) < rng.choice([0.002, 0.1, 0.9]))[0]
        toks = toks[toks != 1]
        if len(toks) == 0:
            toks = np.array([int(rng.integers(2, V))])
        maps[s * 3 + 1] = {int(t): int(rng.integers(0, S)) * 3 + 1 for t in toks}
    f = TokenFSM.from_transitions(maps, 1, eos_token_id=1, vocab=V)
    allow, rank, off, nxt = f.tables()
    assert allow.shape == (S + 1, 32) and allow.dtype == np.uint32 and rank.shape == allow.shape and G.guide_words(V) == 32
    assert G.guide_words(128256) == 4008 and G.guide_words(33) == 4
    number = {k: i for i, k in enumerate(sorted(maps))}
    for s_key, row in maps.items():
        s = number[s_key]
        pop = np.array([bin(int(w)).count("1") for w in allow[s]])
        assert np.array_equal(rank[s], np.cumsum(pop) - pop)
        for t in range(V):
            want = number[row[t]] if t in row else f.miss
            assert G.table_next(allow, rank, off, nxt, s, t, f.miss) == want == f.next(s, t), (s, t)
    assert all(G.table_next(allow, rank, off, nxt, f.miss, t, f.miss) == f.miss for t in range(V))
    assert (allow[:, -1] >> np.uint32(1003 - 31 * 32)).max() == 0                       # no bit at or beyond the vocabulary


def test_csr_validation_refuses_bad_guides():
    ok = dict(row_ptr=[0, 2, 3], tokens=[1, 5, 2], next_states=[0, 1, 1], initial=0, miss=1, vocab=8)
    TokenFSM(**ok)
    for change in (dict(tokens=[5, 1, 2]), dict(tokens=[1, 1, 2]), dict(row_ptr=[0, 3, 3]), dict(tokens=[1, 8, 2]),
                   dict(tokens=[-1, 5, 2]), dict(next_states=[0, 2, 1]), dict(next_states=[0, -1, 1]), dict(initial=2),
                   dict(miss=-1), dict(row_ptr=[0, 2, 4]), dict(row_ptr=[1, 2, 3]), dict(vocab=0)):
        with pytest.raises(ValueError):
            TokenFSM(**{**ok, **change})
    with pytest.raises(ValueError, match="states"):
        TokenFSM(np.arange(G.MAX_GUIDE_STATES + 2), np.zeros(G.MAX_GUIDE_STATES + 1), np.zeros(G.MAX_GUIDE_STATES + 1), 0, 0, 8)


# ---------------------------------------------------------------------- arena
def _fsm(n_states, V=64, eos=1):
    return TokenFSM.from_transitions({i: {2 + i % 50: (i + 1) % (n_states - 1), 60: i} for i in range(n_states - 1)}, 0, eos, V)


def test_arena_shares_counts_references_and_reuses_least_recently_used_room():
    a = GuideArena(max_states=10, max_transitions=100, keep=2)
    f4, g4, h4, big = _fsm(4), _fsm(4), _fsm(4), _fsm(7)
    r1, fresh1 = a.acquire(f4)
    r2, fresh2 = a.acquire(f4)
    assert fresh1 and not fresh2 and r1 is r2 and r1.refs == 2 and (r1.state_base, r1.trans_base) == (0, 0)   # one copy, shared
    rg, _ = a.acquire(g4)
    assert (rg.state_base, rg.trans_base) == (4, f4.num_transitions)
    with pytest.raises(ValueError, match="no room"):
        a.plan(h4)                                                                   # 4 + 4 + 4 > 10 and both are in use
    a.release(f4)
    with pytest.raises(ValueError, match="no room"):
        a.acquire(h4)                                                                # still referenced by one slot
    assert a.resident(h4) is None and a.resident(f4).refs == 1
    a.release(f4)
    assert a.resident(f4) is not None and a.resident(f4).refs == 0                   # kept by the LRU after the last release
    r3, fresh3 = a.acquire(f4)
    assert not fresh3 and r3 is r1                                                   # ... and found again without a build
    a.release(f4)
    rh, fresh = a.acquire(h4)                                                        # needs room: the idle guide goes
    assert fresh and a.resident(f4) is None and (rh.state_base, rh.trans_base) == (0, 0)
    a.release(h4); a.release(g4)
    evict, sb, tb = a.plan(big)                                                      # least recently used first: h4, then g4
    assert [e.fsm for e in evict] == [h4, g4] and (sb, tb) == (0, 0)
    with pytest.raises(ValueError, match="arena holds"):
        a.plan(_fsm(12))                                                             # over the state cap outright
    with pytest.raises(ValueError, match="arena holds"):
        GuideArena(100, 5).plan(f4)                                                  # over the transition cap
    with pytest.raises(ValueError):
        a.release(f4)
    b = GuideArena(100, 1000, keep=1)
    fs = [_fsm(3) for _ in range(3)]
    for f in fs:
        b.acquire(f)
    for f in fs:
        b.release(f)
    assert [b.resident(f) is not None for f in fs] == [False, False, True]           # at most `keep` idle guides stay


# ---------------------------------------------------------------------- engine slot state (host tensors)
@pytest.fixture
def recorded(monkeypatch):
    from qspec_amd import ops
    calls = []
    monkeypatch.setattr(ops, "guide_build", lambda tg, sb, tb, rp, tk, nx: calls.append((sb, tb, len(rp) - 1, len(tk))))
    monkeypatch.setattr(ops, "token_constraints_set", lambda tc, slot, *a: None)
    return calls


def test_engine_guides_follow_set_sampling_params_fork_and_free_slot(recorded):
    eng = HostEngine()
    s = eng.sampling
    eng.set_sampling_params(0, 0.8, 50, 0.9)
    assert s.tg is None and s.guide_arena is None and s._g_host is None and s.level([0]) == 1   # nothing asked for: nothing allocated
    f, g = _fsm(4), _fsm(5)
    eng.set_sampling_params(1, 0.0, guide=f)
    assert s.tg is not None and s.tg.allow.shape == (1024, 4) and s.tg.gslot.shape == (4, 4) and s.tc is not None and s.tok_table is not None
    assert recorded == [(0, 0, 4, f.num_transitions)] and s.tg.gslot[1].tolist() == [f.initial, 0, f.miss, 1]
    assert s.level([0]) == 1 and s.level([0, 1]) == 4 and not s.constraints_on([1]) and s.guides_on([1])
    eng.set_sampling_params(2, 0.7, seed=3, guide=f)                                  # the same object: shared, not built again
    eng.set_sampling_params(3, 0.0, guide=g, allowed_token_ids=[2, 3, 60])
    assert len(recorded) == 2 and recorded[1][:3] == (4, f.num_transitions, 5) and s.guide_arena.resident(f).refs == 2
    assert s.tg.gslot[3].tolist() == [4 + g.initial, 0, 4 + g.miss, 1] and s.level([3]) == 4
    eng.set_sampling_params(1, 0.0, guide=f)
    assert len(recorded) == 2                                                         # unchanged: nothing enqueued
    s.admit_tokens(3, [9, 9, 9, 2, 3], 3)                                             # re-admitted with two outputs: walked on the host
    assert s.tg.gslot[3].tolist() == [4 + g.advance(g.initial, [2, 3]), 0, 4 + g.miss, 1]
    eng._len_ub[1] = 10
    with pytest.raises(ValueError, match="admitted"):
        eng.set_sampling_params(1, 0.0, guide=g)                                      # a guide on an admitted request
    with pytest.raises(ValueError, match="admitted"):
        eng.set_sampling_params(1, 0.0)
    s.tg.gslot[1] = torch.tensor([2, 5, f.miss, 1], dtype=torch.int32)
    eng._len_ub[1] = 0
    s.fork(1, 0)                                                                      # reference, state and g_len travel
    assert s._g_host[0] is f and s.tg.gslot[0].tolist() == [2, 5, f.miss, 1] and s.guide_arena.resident(f).refs == 3
    for b in (0, 1, 2):
        eng.free_slot(b)
    assert s.guide_arena.resident(f).refs == 0 and s._g_host[:3] == [None] * 3 and s.tg.gslot[:3].abs().sum() == 0
    assert s.level([0, 1, 2]) == 0 and s.level([3]) == 4
    eng.set_sampling_params(1, 0.0, guide=f)                                          # still resident: no build
    assert len(recorded) == 2


def test_engine_refuses_guides_it_cannot_hold_and_enqueues_nothing(recorded):
    eng = HostEngine()
    eng.sampling.guide_states, eng.sampling.guide_transitions = 8, 64
    for bad in (_fsm(10), TokenFSM.from_transitions({i: {t: i for t in range(2, 40)} for i in range(3)}, 0, 1, 64), _fsm(4, V=32),
                {0: {1: 0}}, "regex"):
        with pytest.raises(ValueError):
            eng.set_sampling_params(1, 0.8, guide=bad)
        assert eng.sampling.tg is None and recorded == [] and eng.sampling._samp_host[1] == (0.0, -1, 1.0)
    a, b = _fsm(5), _fsm(5)
    eng.set_sampling_params(0, 0.0, guide=a)
    with pytest.raises(ValueError, match="no room"):
        eng.set_sampling_params(1, 0.0, guide=b)                                      # 5 + 5 > 8 while the first is in use
    assert len(recorded) == 1 and eng.sampling._g_host[1] is None
    eng.set_sampling_params(0, 0.0, guide=b)                                          # the slot's own guide makes room for its successor
    assert len(recorded) == 2 and eng.sampling._g_host[0] is b


# ---------------------------------------------------------------------- worker, on a scripted engine
class RegexLogitsProcessor:   # attribute holders written for this test: the worker lowers processors, it never calls them
    def __init__(self, guide):
        self._guide, self._fsm_state = guide, defaultdict(int)


class JSONLogitsProcessor(RegexLogitsProcessor):
    pass


class CFGLogitsProcessor(RegexLogitsProcessor):
    pass


class SomeProcessor(RegexLogitsProcessor):
    pass


class AllowedTokenIdsLogitsProcessor:
    def __init__(self, allowed_ids):
        self.allowed_ids, self.mask = allowed_ids, None


class NoBadWordsLogitsProcessor:
    def __init__(self, bad_words_ids):
        self.bad_words_ids = bad_words_ids


class _ScriptedEngine:
    def __init__(self):
        self.calls = []

    def set_sampling_params(self, slot, *a, **kw):
        self.calls.append(("set", slot, a, kw))

    def add_sequences_to(self, *a, **kw):
        self.calls.append(("add", a, kw))

    def free_slot(self, slot):
        self.calls.append(("free", slot))


def _worker(engine, vocab=32):
    w = W.SpecDecodeWorker.__new__(W.SpecDecodeWorker)
    w.engine, w.max_num_seqs, w._slots = engine, 4, {}
    w.model_config = SimpleNamespace(vocab_size=vocab)
    w._request_id_seq_id_mapping = defaultdict(set)
    return w


def _req(rid, sp, prompt=(1, 2, 3), outputs=()):
    return W.SequenceGroupMetadata(request_id=rid, is_prompt=True, seq_data={0: W.SequenceData(list(prompt), list(outputs))},
                                   sampling_params=sp)


def _vsp(**kw):
    return SimpleNamespace(**{**dict(temperature=0.0, top_k=-1, top_p=1.0, seed=None, logit_bias=None, allowed_token_ids=None), **kw})


def test_worker_recognises_lowered_guided_processors_and_merges_in_the_reference_order():
    import functools

    def logit_bias_logits_processor(logit_bias, token_ids, logits):
        raise AssertionError("never called")
    unknown = lambda ids, logits: logits   # noqa: E731
    guide = _AttrGuide()
    for proc in (RegexLogitsProcessor(guide), JSONLogitsProcessor(guide), SomeProcessor(_CallGuide())):
        eng = _ScriptedEngine()
        procs = [proc, functools.partial(logit_bias_logits_processor, {3: 100.0}), AllowedTokenIdsLogitsProcessor([11, 12, 13]),
                 NoBadWordsLogitsProcessor([[12, 11]]), unknown]                       # the guide at index 0, as the engine lowers it
        _worker(eng)._admit([_req("a", _vsp(logits_processors=procs), outputs=(12,)), _req("b", _vsp(logits_processors=[unknown]))])
        kw = [c for c in eng.calls if c[0] == "set"][0][3]
        assert set(kw) == {"guide", "logit_bias", "allowed_token_ids", "bad_words_token_ids"}
        assert isinstance(kw["guide"], TokenFSM) and kw["guide"].accepts([12, 11, 13, 14]) and kw["guide"].vocab == 32
        assert kw["logit_bias"] == {3: 100.0} and kw["allowed_token_ids"] == [11, 12, 13] and kw["bad_words_token_ids"] == [[12, 11]]
        assert [c for c in eng.calls if c[0] == "set"][1] == ("set", 1, (0.0, -1, 1.0), {})   # unrecognised callables: ignored as before
        # a guided request that comes back with outputs tells the engine where its prompt ends
        assert [c for c in eng.calls if c[0] == "add"][0][2] == dict(num_prompt_tokens=[3, None])
    # two requests that share a processor's guide share the lowered automaton (one resident copy in the engine)
    eng = _ScriptedEngine()
    _worker(eng)._admit([_req("a", _vsp(logits_processors=[RegexLogitsProcessor(guide)])),
                         _req("b", _vsp(logits_processors=[JSONLogitsProcessor(guide)]))])
    sets = [c for c in eng.calls if c[0] == "set"]
    assert sets[0][3]["guide"] is sets[1][3]["guide"]
    # the worker's own field
    own = TokenFSM.from_token_sequences([[4, 5]], 1, 32)
    eng = _ScriptedEngine()
    _worker(eng)._admit([_req("a", W.SamplingParams(temperature=0.5, guided_fsm=own))])
    assert [c for c in eng.calls if c[0] == "set"][0][3] == {"guide": own}


def test_worker_refuses_what_it_cannot_guide_by_name():
    guide = _AttrGuide()

    class CFGState:
        pass

    class CFGGuide(_CallGuide):
        initial_state = CFGState()
    cases = [(_vsp(logits_processors=[CFGLogitsProcessor(CFGGuide())]), "CFGLogitsProcessor"),
             (_vsp(logits_processors=[CFGLogitsProcessor(guide)]), "CFGLogitsProcessor"),
             (_vsp(logits_processors=[SomeProcessor(CFGGuide())]), "SomeProcessor"),
             (_vsp(logits_processors=[RegexLogitsProcessor(None)]), "RegexLogitsProcessor"),
             (_vsp(logits_processors=[JSONLogitsProcessor(object())]), "JSONLogitsProcessor"),
             (_vsp(guided_decoding=SimpleNamespace(regex="a+")), "guided_decoding"),
             (_vsp(guided_decoding=SimpleNamespace(json={}), logits_processors=[RegexLogitsProcessor(guide)]), "guided_decoding"),
             (_vsp(logits_processors=[RegexLogitsProcessor(guide), JSONLogitsProcessor(_AttrGuide())]), "more than one")]
    for sp, word in cases:
        eng = _ScriptedEngine()
        with pytest.raises(NotImplementedError, match=word):
            _worker(eng)._admit([_req("a", sp)])
        assert not [c for c in eng.calls if c[0] in ("set", "add")]
    with pytest.raises(ValueError):
        _worker(_ScriptedEngine())._admit([_req("a", W.SamplingParams(guided_fsm={0: {1: 0}}))])
    eng = _ScriptedEngine()
    _worker(eng)._admit([_req("a", _vsp(guided_decoding=None, logits_processors=None))])
    assert [c for c in eng.calls if c[0] == "set"][0][3] == {}


# ---------------------------------------------------------------------- C ABI
def test_new_symbols_declared_bound_exported_and_validating():
    declared = _lib.header_symbols()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(raw, name), name
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
        assert m is not None and len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert _lib.header_symbols() == sorted(_lib.SIGNATURES)
    lib = _lib.load()
    assert lib.qspec_abi_version() == 6
    P = 16   # dummy non-NULL pointers are never dereferenced: validation comes before any HIP call

    def pl(**kw):
        a = dict(logits=P, out=P + 16, tokens=4, vocab=64, table=P, num_slots=4, slot_ids=None, active=None, rep=P, freq=P, pres=P,
                 min_tokens=P, gen_base=P, gen_lens=P, stop_ids=P, n_stop=P, stop_w=16, draft=P, draft_rows=3, sb=1, sk=4, rps=4,
                 j_base=0, deny=P, deny_words=2, meta=P, bias_ids=P, bias_vals=P, words=P, word_lens=P, tail=P, gen_tokens=P,
                 gen_cap=8, allow=P, rank=P, off=P, nxt=P, gslot=P, gwords=4, gstates=8, gtrans=100)
        a.update(kw)
        return lib.qspec_process_logits_guided(*a.values(), None)
    for kw, word in ((dict(tokens=-1), b"tokens"), (dict(out=P), b"out of place"), (dict(deny=None), b"deny"), (dict(allow=None), b"guide_allow"),
                     (dict(rank=None), b"guide_rank"), (dict(off=None), b"guide_off"), (dict(nxt=None), b"guide_next"),
                     (dict(gslot=None), b"guide_slots"), (dict(gwords=1), b"guide_words"), (dict(gwords=6), b"guide_words"),
                     (dict(gstates=0), b"guide_states"), (dict(gtrans=0), b"guide_transitions"), (dict(draft_rows=2), b"in-flight")):
        assert pl(**kw) != 0 and word in lib.qspec_last_error(), (kw, lib.qspec_last_error())
        assert lib.qspec_last_error().startswith(b"qspec_process_logits_guided:")

    def gb(**kw):
        a = dict(allow=P, rank=P, off=P, nxt=P, words=4, stride=4, vocab=64, max_states=8, max_trans=100, sb=0, tb=0, ns=3, nt=10,
                 row_ptr=P, tokens=P, nexts=P)
        a.update(kw)
        return lib.qspec_guide_build(*a.values(), None)
    for kw, word in ((dict(allow=None), b"guide_allow"), (dict(row_ptr=None), b"row_ptr"), (dict(nexts=None), b"next_states"),
                     (dict(words=2), b"guide_words"), (dict(words=6, stride=8), b"guide_words"), (dict(words=8196, stride=8196), b"guide_words"),
                     (dict(stride=6), b"row_stride"), (dict(words=8, stride=4), b"row_stride"), (dict(vocab=0), b"vocab"),
                     (dict(vocab=129), b"guide_words"), (dict(sb=6), b"states"), (dict(sb=-1), b"states"), (dict(ns=0), b"states"),
                     (dict(tb=91), b"transitions"), (dict(nt=0), b"transitions"), (dict(tb=-1), b"transitions")):
        assert gb(**kw) != 0 and word in lib.qspec_last_error(), (kw, lib.qspec_last_error())

    def cu(**kw):
        a = dict(gslot=P, num_slots=4, vocab=64, allow=P, rank=P, off=P, nxt=P, words=4, states=8, trans=100, gen_tokens=P, gen_cap=8,
                 gen_lens=P)
        a.update(kw)
        return lib.qspec_guide_catch_up(*a.values(), None)
    assert cu(num_slots=0) == 0
    for kw, word in ((dict(gslot=None), b"guide_slots"), (dict(num_slots=-1), b"num_slots"), (dict(gen_tokens=None), b"gen_tokens"),
                     (dict(gen_lens=None), b"gen_lens"), (dict(gen_cap=0), b"gen_cap"), (dict(words=1), b"guide_words"),
                     (dict(states=0), b"guide_states"), (dict(vocab=0), b"vocab")):
        assert cu(**kw) != 0 and word in lib.qspec_last_error(), (kw, lib.qspec_last_error())
