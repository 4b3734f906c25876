"""Token constraints (logit_bias, allowed_token_ids, bad words), the parts that need no GPU: the CPU restatement against the
reference fixture, the C ABI surface, the engine's validation and slot bookkeeping, the worker's lowering."""
import ctypes
import functools
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import constraint_cases as cc  # noqa: E402
import logit_cases as lc  # noqa: E402

from qspec_amd import _lib  # noqa: E402
from qspec_amd.spec_decode import worker as W  # noqa: E402
from host_engine import HostEngine  # noqa: E402

NEW = ("qspec_process_logits_constrained", "qspec_token_constraints_set")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "token_constraints.npz")


def fixture_rows(g):
    """(i, name, raw, prompt, outputs, in flight, Params, Constraints) of every fixture row."""
    V = g["tc_raw"].shape[1]
    strip = lambda a: [int(t) for t in a if 0 <= t < V]   # noqa: E731  (padding: V, or -1)
    for i in range(g["tc_raw"].shape[0]):
        p = lc.Params(repetition=float(g["tc_rep"][i]), frequency=float(g["tc_freq"][i]), presence=float(g["tc_pres"][i]),
                      min_tokens=int(g["tc_min_tokens"][i]), stop_ids=tuple(strip(g["tc_stop"][i])))
        nb = int((g["tc_bias_ids"][i] >= 0).sum())
        c = cc.Constraints(
            logit_bias={int(t): float(b) for t, b in zip(g["tc_bias_ids"][i][:nb], g["tc_bias_vals"][i][:nb])},
            allowed=tuple(int(t) for t in np.nonzero(g["tc_allowed"][i])[0]) if g["tc_has_allowed"][i] else None,
            bad_words=tuple(tuple(int(t) for t in w[:n]) for w, n in zip(g["tc_words"][i], g["tc_word_lens"][i]) if n > 0))
        yield i, str(g["tc_names"][i]), g["tc_raw"][i], strip(g["tc_prompt"][i]), strip(g["tc_outputs"][i]), \
            strip(g["tc_inflight"][i]), p, c


def test_restatement_reproduces_the_reference_fixture_bit_for_bit():
    g = np.load(GOLDEN)
    names = []
    for i, name, raw, prompt, outs, infl, p, c in fixture_rows(g):
        mid = cc.constrain_row(raw, outs, infl, c)
        assert np.array_equal(mid.view(np.uint16), g["tc_constrained"][i].view(np.uint16)), name
        got = cc.process_row_constrained(raw, prompt, outs, infl, p, c)
        assert np.array_equal(got.view(np.uint16), g["tc_expected"][i].view(np.uint16)), name
        names.append(name)
    assert len(names) >= 26
    # what the fixture must hold: both zero signs and -inf under a bias, the fp16 ceiling, allowed sets of 1 and V - 1, the shared
    # processor with only its mask, words of 1 / 2 / 8 tokens, a match through in-flight tokens, NO NaN (the one divergence)
    raw, V = g["tc_raw"], g["tc_raw"].shape[1]
    assert (raw.view(np.uint16) == 0x8000).any() and (raw.view(np.uint16) == 0).any() and np.isneginf(raw).any()
    sizes = set(int(a.sum()) for a, h in zip(g["tc_allowed"], g["tc_has_allowed"]) if h)
    assert {1, V - 1} <= sizes and g["tc_mask_only"].sum() >= 1
    assert {1, 2, 8} <= set(g["tc_word_lens"].ravel().tolist())
    assert not np.isnan(g["tc_expected"]).any() and np.isposinf(g["tc_constrained"]).any()
    i = names.index("bad_single")
    assert not (g["tc_constrained"][i].view(np.uint16) == 0x8000).any() and (raw[i].view(np.uint16) == 0x8000).any()
    i = names.index("bias_zero_inf_a")
    assert (g["tc_constrained"][i].view(np.uint16) == 0x8000).any()      # no bad words: a -0.0 survives


def test_bad_words_look_at_outputs_and_in_flight_tokens_never_at_the_prompt():
    assert cc.banned_last_tokens([3, 70], [(70, 71), (3, 70, 72), (9, 3, 70, 73), (70,)]) == [71, 72]
    assert cc.banned_last_tokens([], [(70, 71)]) == []
    assert cc.banned_last_tokens([70, 71], [(70, 71, 75), (71, 75)]) == [75, 75]
    # the position rule: row j of a cycle == one-token-at-a-time decoding of the same prefix
    rng = np.random.default_rng(3)
    V, k = 64, 5
    seq = [int(t) for t in rng.integers(0, 6, 60)]
    c = cc.Constraints(logit_bias={1: 2.0}, allowed=tuple(range(0, 40)),
                       bad_words=tuple(tuple(seq[s:s + n]) for s, n in ((3, 2), (10, 3), (20, 8), (31, 4))) + ((5,),))
    for start in (0, 1, 2, 9, 19, 27):
        raws = (rng.standard_normal((k + 1, V)) * 3).astype(np.float16)
        for j in range(k + 1):
            a = cc.constrain_row(raws[j], seq[:start], seq[start:start + j], c)
            b = cc.constrain_row(raws[j], seq[:start + j], [], c)
            assert np.array_equal(a.view(np.uint16), b.view(np.uint16))


def test_new_symbols_declared_bound_exported_and_validating():
    declared = _lib.header_symbols()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(raw, name), name
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
        assert m is not None and len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert _lib.header_symbols() == sorted(_lib.SIGNATURES)
    for cap, val in (("QS_MAX_LOGIT_BIAS", 512), ("QS_MAX_BAD_WORDS", 32), ("QS_MAX_BAD_WORD_LEN", 8)):
        assert re.search(r"#define\s+%s\s+%d\b" % (cap, val), text), cap
    lib = _lib.load()
    assert lib.qspec_abi_version() == 6
    P = 16   # dummy non-NULL pointers are never dereferenced: validation comes before any HIP call

    def pl(**kw):
        a = dict(logits=P, out=P + 16, tokens=4, vocab=64, table=P, num_slots=4, slot_ids=None, active=None, rep=P, freq=P, pres=P,
                 min_tokens=P, gen_base=P, gen_lens=P, stop_ids=P, n_stop=P, stop_w=16, draft=P, draft_rows=3, sb=1, sk=4, rps=4,
                 j_base=0, deny=P, deny_words=2, meta=P, bias_ids=P, bias_vals=P, words=P, word_lens=P, tail=P, gen_tokens=P,
                 gen_cap=8)
        a.update(kw)
        return lib.qspec_process_logits_constrained(*a.values(), None)
    for kw, word in ((dict(tokens=-1), b"tokens"), (dict(out=P), b"out of place"), (dict(deny=None), b"deny"),
                     (dict(deny_words=1), b"deny_words"), (dict(meta=None), b"meta"), (dict(gen_tokens=None), b"gen_tokens"),
                     (dict(gen_cap=0), b"gen_cap"), (dict(tail=None), b"tail"), (dict(draft_rows=2), b"in-flight")):
        assert pl(**kw) != 0 and word in lib.qspec_last_error(), (kw, lib.qspec_last_error())

    def ts(**kw):
        a = dict(deny=P, deny_words=2, meta=P, bias_ids=P, bias_vals=P, words=P, word_lens=P, num_slots=4, vocab=64, slot=0,
                 allowed=P, n_allowed=1, banned=None, n_banned=0, sbi=None, sbv=None, n_bias=0, sw=None, swl=None, n_words=0, bw=0)
        a.update(kw)
        return lib.qspec_token_constraints_set(*a.values(), None)
    for kw, word in ((dict(slot=4), b"slot"), (dict(n_bias=513, sbi=P, sbv=P), b"num_bias"), (dict(n_words=33, sw=P, swl=P), b"num_words"),
                     (dict(allowed=None), b"allowed_ids"), (dict(n_banned=1), b"banned_ids"), (dict(deny_words=1), b"deny_words"),
                     (dict(n_bias=1), b"src_bias_ids"), (dict(n_words=1), b"src_words")):
        assert ts(**kw) != 0 and word in lib.qspec_last_error(), (kw, lib.qspec_last_error())


@pytest.fixture
def recorded(monkeypatch):
    from qspec_amd import ops
    calls = []
    monkeypatch.setattr(ops, "token_constraints_set", lambda tc, slot, *a: calls.append((slot,) + a))
    return calls


def test_engine_constraints_follow_set_sampling_params_and_free_slot(recorded):
    eng = HostEngine()
    s = eng.sampling
    eng.set_sampling_params(1, 0.8, 50, 0.9, min_p=0.1)
    assert s._tc_host is None and s.tc is None and not s.constraints_on(eng.active_slots())   # nothing asked for: nothing allocated
    eng.set_sampling_params(2, 0.0, logit_bias={"7": 1.5, 3: -100.0}, allowed_token_ids=[9, 3, 3, 7],
                            bad_words_token_ids=[[5], [4, 9], [4, 9], [5]])
    assert s.tc is not None and s.tc.deny.shape == (4, 2) and s.tc.meta.shape == (4, 4) and s.tok_table is not None
    assert s.tc.bias_ids.shape == (4, 512) and s.tc.words.shape == (4, 32, 8) and s.tc.tail.shape == (4, 7)
    assert recorded == [(2, {3: -100.0, 7: 1.5}, (3, 7, 9), [[5], [4, 9]])]
    assert not s.constraints_on(eng.active_slots()) and not s.processing_on(eng.active_slots())   # the slot is not occupied yet
    eng._len_ub[2] = 10
    assert s.constraints_on(eng.active_slots()) and s.processing_on(eng.active_slots()) and not s.sampling_on(eng.active_slots())
    eng.set_sampling_params(2, 0.0, logit_bias={3: -100.0, 7: 1.5}, allowed_token_ids=(9, 7, 3), bad_words_token_ids=[(5,), (4, 9)])
    assert len(recorded) == 1                                                      # the same constraints: nothing uploaded
    with pytest.raises(ValueError, match="admitted"):
        eng.set_sampling_params(2, 0.0, logit_bias={3: 1.0})
    eng.free_slot(2)
    assert recorded[-1] == (2,) and s._tc_host[2] is None and not s.constraints_on(eng.active_slots()) and not s.processing_on(eng.active_slots())


def test_engine_refuses_bad_constraints_and_enqueues_nothing(recorded):
    eng = HostEngine()
    s = eng.sampling
    many = {t: 1.0 for t in range(513)}
    big = HostEngine(V=1024)
    for e, kw in ((eng, dict(logit_bias={64: 1.0})), (eng, dict(logit_bias={-1: 1.0})), (eng, dict(logit_bias={"x": 1.0})),
                  (eng, dict(logit_bias={1: float("nan")})), (eng, dict(logit_bias={1: float("inf")})),
                  (eng, dict(allowed_token_ids=[])), (eng, dict(allowed_token_ids=[64])), (eng, dict(bad_words_token_ids=[[]])),
                  (eng, dict(bad_words_token_ids=[[1, 64]])), (eng, dict(bad_words_token_ids=[list(range(9))])),
                  (eng, dict(bad_words_token_ids=[[t, t + 1] for t in range(33)])), (big, dict(logit_bias=many)),
                  (eng, dict(allowed_token_ids=[3, 4], bad_words_token_ids=[[3], [4]])),
                  (eng, dict(allowed_token_ids=[3, 4, 5], bad_words_token_ids=[[3]], min_tokens=2, stop_token_ids=(4, 5)))):
        with pytest.raises(ValueError):
            e.set_sampling_params(1, 0.8, **kw)
        assert e.sampling._tc_host is None and e.sampling.tc is None and e.sampling._samp_host[1] == (0.0, -1, 1.0) and recorded == []
    # the same allowed set is fine once min_tokens leaves a token, and 32 words of 8 tokens / 512 biases are inside the caps
    eng.set_sampling_params(1, 0.8, allowed_token_ids=[3, 4, 5, 6], bad_words_token_ids=[[3]], min_tokens=2, stop_token_ids=(4, 5))
    big.set_sampling_params(1, 0.0, logit_bias={t: 1.0 for t in range(512)},
                            bad_words_token_ids=[list(range(t, t + 8)) for t in range(32)] + [[t] for t in range(900)])
    assert len(recorded) == 2


# ---------------------------------------------------------------------- worker, on a scripted engine
def logit_bias_logits_processor(logit_bias, token_ids, logits):   # a stand-in by NAME only: the worker never calls it
    raise AssertionError("the worker lowers processors, it does not run them")


class AllowedTokenIdsLogitsProcessor:   # attribute holders written for this test
    def __init__(self, allowed_ids=None, mask=None):
        self.allowed_ids, self.mask = allowed_ids, mask


class NoBadWordsLogitsProcessor:
    def __init__(self, bad_words_ids):
        self.bad_words_ids, self.word_bias = bad_words_ids, None


class _ScriptedEngine:
    def __init__(self):
        self.calls = []
        self.gen_tokens = torch.zeros(4, 8, dtype=torch.int64)

    def set_sampling_params(self, slot, *a, **kw):
        self.calls.append(("set", slot, a, kw))

    def add_sequences_to(self, *a, **kw):
        self.calls.append(("add", a, kw))

    def free_slot(self, slot):
        self.calls.append(("free", slot))


class _OldEngine(_ScriptedEngine):
    def set_sampling_params(self, slot, temperature=0.0, top_k=-1, top_p=1.0):   # knows none of the newer keywords
        self.calls.append(("set", slot, (temperature, top_k, top_p), {}))


def _worker(engine):
    w = W.SpecDecodeWorker.__new__(W.SpecDecodeWorker)
    w.engine, w.max_num_seqs, w._slots = engine, 4, {}
    from collections import defaultdict
    w._request_id_seq_id_mapping = defaultdict(set)
    return w


def _req(rid, sp, prompt=(1, 2, 3), outputs=()):
    return W.SequenceGroupMetadata(request_id=rid, is_prompt=True, seq_data={0: W.SequenceData(list(prompt), list(outputs))},
                                   sampling_params=sp)


def _set_kw(eng, i=0):
    return [c for c in eng.calls if c[0] == "set"][i][3]


def test_worker_forwards_the_plain_fields_and_only_when_set():
    eng = _ScriptedEngine()
    w = _worker(eng)
    sp = W.SamplingParams(temperature=0.7, logit_bias={"5": 150.0, 6: -250.0, "7": 0.5}, allowed_token_ids=[9, 5, 5],
                          bad_words_token_ids=[[4], [2, 3], [2, 3]])
    w._admit([_req("a", sp), _req("b", W.SamplingParams(temperature=0.7)), _req("c", None)])
    assert _set_kw(eng, 0) == dict(logit_bias={5: 100.0, 6: -100.0, 7: 0.5}, allowed_token_ids=[5, 9],
                                   bad_words_token_ids=[[4], [2, 3]])          # string keys, clamped as the lowering clamps
    sets = [c for c in eng.calls if c[0] == "set"]
    assert sets[1] == ("set", 1, (0.7, -1, 1.0), {}) and sets[2] == ("set", 2, (0.0, -1, 1.0), {})
    assert [c for c in eng.calls if c[0] == "add"][0][2] == {}
    old = _OldEngine()                                                          # an engine double that knows no new keyword
    _worker(old)._admit([_req("d", W.SamplingParams(temperature=0.7)), _req("e", None)])
    assert len([c for c in old.calls if c[0] == "set"]) == 2
    for bad in (W.SamplingParams(logit_bias={"x": 1.0}), W.SamplingParams(allowed_token_ids=[])):
        with pytest.raises(ValueError):
            _worker(_ScriptedEngine())._admit([_req("f", bad)])


def test_worker_lowers_the_three_reference_processors_by_duck_typing():
    mask = torch.ones(32, dtype=torch.bool)
    mask[[3, 8, 20]] = False
    unknown = lambda ids, logits: logits   # noqa: E731
    for allowed_proc in (AllowedTokenIdsLogitsProcessor(allowed_ids=[20, 3, 8]), AllowedTokenIdsLogitsProcessor(mask=mask),
                         AllowedTokenIdsLogitsProcessor(mask=mask.tolist())):
        eng = _ScriptedEngine()
        vsp = SimpleNamespace(temperature=0.0, top_k=-1, top_p=1.0, seed=None, logit_bias=None, allowed_token_ids=None,
                              bad_words=["foo"], logits_processors=[unknown, functools.partial(logit_bias_logits_processor, {3: 100.0, 8: -1.5}),
                                                                    allowed_proc, NoBadWordsLogitsProcessor([[7], [3, 8], [8, 3, 20]])])
        _worker(eng)._admit([_req("a", vsp)])
        assert _set_kw(eng) == dict(logit_bias={3: 100.0, 8: -1.5}, allowed_token_ids=[3, 8, 20],
                                    bad_words_token_ids=[[7], [3, 8], [8, 3, 20]])
    # a field and a processor that say the same thing are ONE constraint; allowed sets intersect; words are deduplicated
    eng = _ScriptedEngine()
    sp = W.SamplingParams(logit_bias={"3": 150.0, 4: 1.0}, allowed_token_ids=[3, 8, 20, 21], bad_words_token_ids=[[7], [1, 2]],
                          logits_processors=[functools.partial(logit_bias_logits_processor, {3: 100.0}),
                                             AllowedTokenIdsLogitsProcessor(allowed_ids=[3, 8, 20]), NoBadWordsLogitsProcessor([[7], [3, 8]])])
    _worker(eng)._admit([_req("a", sp)])
    assert _set_kw(eng) == dict(logit_bias={3: 100.0, 4: 1.0}, allowed_token_ids=[3, 8, 20], bad_words_token_ids=[[7], [1, 2], [3, 8]])
    # only unknown callables / bad_words strings without a lowered processor: ignored, exactly the old calls
    eng = _ScriptedEngine()
    _worker(eng)._admit([_req("a", SimpleNamespace(temperature=0.0, top_k=-1, top_p=1.0, seed=None, bad_words=["foo"],
                                                   logits_processors=[unknown, functools.partial(unknown)]))])
    assert eng.calls[0] == ("set", 0, (0.0, -1, 1.0), {})
    with pytest.raises(ValueError):    # disjoint allowed sets
        _worker(_ScriptedEngine())._admit([_req("a", W.SamplingParams(allowed_token_ids=[1], logits_processors=[
            AllowedTokenIdsLogitsProcessor(allowed_ids=[2])]))])


def test_worker_passes_the_prompt_length_of_a_recomputed_constrained_request():
    eng = _ScriptedEngine()
    sp = W.SamplingParams(bad_words_token_ids=[[7, 8]])
    _worker(eng)._admit([_req("a", sp, prompt=(1, 2, 3), outputs=(9, 7)), _req("b", sp, prompt=(4, 5))])
    add = [c for c in eng.calls if c[0] == "add"][0]
    assert add[1][1] == [[1, 2, 3, 9, 7], [4, 5]] and add[2] == dict(num_prompt_tokens=[3, None])
