"""Logit processors (min_p, presence / frequency / repetition penalties, min_tokens), the parts that need no GPU: the CPU
restatement against the reference fixture, the position rule of a speculative cycle, the C ABI surface, the engine's slot
bookkeeping and the worker's forwarding."""
import ctypes
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logit_cases as lc  # noqa: E402

from qspec_amd import _lib  # noqa: E402
from qspec_amd.spec_decode import worker as W  # noqa: E402
from host_engine import HostEngine  # noqa: E402

NEW = ("qspec_process_logits", "qspec_logit_table_set_prompt", "qspec_logit_table_catch_up",
       "qspec_sample_top_k_top_p_min_p", "qspec_sample_top_k_top_p_min_p_seeded")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "logit_processors.npz")


def _fixture_rows(g):
    V = g["pen_raw"].shape[1]
    for i in range(g["pen_raw"].shape[0]):
        strip = lambda a: [int(t) for t in a if 0 <= t < V]   # noqa: E731  (padding: V, or -1 for the stop ids)
        p = lc.Params(repetition=float(g["pen_rep"][i]), frequency=float(g["pen_freq"][i]), presence=float(g["pen_pres"][i]),
                      min_tokens=int(g["pen_min_tokens"][i]), stop_ids=tuple(strip(g["pen_stop"][i])))
        yield i, g["pen_raw"][i], strip(g["pen_prompt"][i]), strip(g["pen_outputs"][i]), strip(g["pen_inflight"][i]), p


def test_process_row_reproduces_the_reference_fixture_bit_for_bit():
    g = np.load(GOLDEN)
    n = 0
    for i, raw, prompt, outs, infl, p in _fixture_rows(g):
        got = lc.process_row(raw, prompt, outs, infl, p)
        assert np.array_equal(got.view(np.uint16), g["pen_expected"][i].view(np.uint16)), i
        n += 1
    assert n >= 19
    # the fixture holds what the issue asks for: +0 / -0 / -inf logits, counts 1, 2, 7 and 300, r < 1, negative penalties, neutral
    raw = g["pen_raw"]
    assert (raw.view(np.uint16) == 0x8000).any() and (raw.view(np.uint16) == 0).any() and np.isneginf(raw).any()
    cnts = np.bincount(g["pen_outputs"][0][g["pen_outputs"][0] < raw.shape[1]])
    assert {1, 2, 7, 300} <= set(cnts.tolist())
    assert (g["pen_rep"] < 1).any() and (g["pen_freq"] < 0).any() and (g["pen_pres"] < 0).any()
    neutral = (g["pen_rep"] == 1) & (g["pen_freq"] == 0) & (g["pen_pres"] == 0) & (g["pen_min_tokens"] == 0)
    assert neutral.any()
    for i in np.nonzero(neutral)[0]:
        assert np.array_equal(g["pen_expected"][i].view(np.uint16), raw[i].view(np.uint16))


def test_min_p_keep_reproduces_the_reference_fixture_exactly():
    g = np.load(GOLDEN)
    T, V = g["mp_logits"].shape
    assert set(np.round(g["mp_min_p"].astype(np.float64), 3).tolist()) == {0.02, 0.1, 0.5, 1.0}
    for t in range(T):
        probs, keep = lc.sampler_probs(g["mp_logits"][t], float(g["mp_temperature"][t]), int(g["mp_top_k"][t]),
                                       float(g["mp_top_p"][t]), float(g["mp_min_p"][t]))
        assert np.array_equal(keep, g["mp_keep"][t]), (t, keep.sum(), g["mp_keep"][t].sum())      # no token exempted
        assert np.abs(probs - g["mp_probs"][t]).max() <= 1e-6, t
        if int(g["mp_top_k"][t]) == V and float(g["mp_top_p"][t]) == 1.0:      # min_p alone: the one-line form
            lf = g["mp_logits"][t].astype(np.float32)
            assert np.array_equal(lc.min_p_keep(lf, float(g["mp_temperature"][t]), float(g["mp_min_p"][t])), g["mp_keep"][t]), t
    assert g["mp_keep"][-1].sum() == 4        # min_p = 1: exactly the tokens tied at the maximum


def test_cycle_rows_equal_one_token_at_a_time_decoding():
    """The position rule: decoding a toy sequence one token at a time (everything before the position is a committed output)
    gives the same processed rows as the cycle view of the same sequence (some committed, d_1 .. d_j in flight), for every j."""
    rng = np.random.default_rng(7)
    V, k = 97, 5
    prompt = [3, 5, 5, 8]
    seq = [int(t) for t in rng.integers(0, 12, 40)]                     # the tokens the sequence ends up with
    p = lc.Params(repetition=1.3, frequency=0.2, presence=0.4, min_tokens=9, stop_ids=(1, 2, 3))
    for start in (0, 1, 4, 7, 8, 20):                                   # committed outputs at the start of the cycle
        raws = (rng.standard_normal((k + 1, V)) * 3).astype(np.float16)
        rows = lc.cycle_rows(raws, prompt, seq[:start], seq[start:start + k], p)
        for j in range(k + 1):
            one = lc.process_row(raws[j], prompt, seq[:start + j], [], p)
            assert np.array_equal(rows[j].view(np.uint16), one.view(np.uint16)), (start, j)
            masked = np.isneginf(rows[j][[1, 2, 3]]).all()
            assert masked == (start + j < 9)


def test_new_symbols_declared_bound_exported_and_validating():
    declared = _lib.header_symbols()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES, name
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
    lib = _lib.load()
    assert lib.qspec_abi_version() == 6
    # header prototypes and ctypes signatures agree on the number of arguments
    import re
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    for name in NEW:
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % name, text, flags=re.S)
        assert m is not None and len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    # argument validation happens before any HIP call (dummy non-NULL pointers are never dereferenced)
    P = 16

    def pl(**kw):
        a = dict(logits=P, out=P + 16, tokens=4, vocab=64, table=P, num_slots=4, slot_ids=None, active=None, rep=P, freq=P, pres=P,
                 min_tokens=P, gen_base=P, gen_lens=P, stop_ids=P, n_stop=P, stop_w=16, draft=P, draft_rows=3, sb=1, sk=4, rps=4,
                 j_base=0)
        a.update(kw)
        return lib.qspec_process_logits(*a.values(), None)
    for kw, word in ((dict(tokens=-1), b"tokens"), (dict(vocab=0), b"vocab"), (dict(rps=0), b"rows_per_seq"),
                     (dict(stop_w=17), b"stop_ids_per_slot"), (dict(draft_rows=2), b"in-flight"), (dict(j_base=1), b"in-flight"),
                     (dict(out=P), b"out of place"), (dict(table=None), b"tok_table"), (dict(num_slots=0), b"num_slots"),
                     (dict(tokens=17), b"does not cover"), (dict(draft=None), b"draft_ids")):
        assert pl(**kw) != 0 and word in lib.qspec_last_error(), (kw, lib.qspec_last_error())
    assert lib.qspec_logit_table_set_prompt(P, P, 4, 64, 4, P, 1, None, 0, None) != 0 and b"slot" in lib.qspec_last_error()
    assert lib.qspec_logit_table_set_prompt(P, P, 4, 64, 0, None, 1, None, 0, None) != 0 and b"prompt_ids" in lib.qspec_last_error()
    assert lib.qspec_logit_table_catch_up(P, P, None, 4, 64, P, 8, P, None) != 0 and b"need_counts" in lib.qspec_last_error()
    assert lib.qspec_logit_table_catch_up(P, P, P, 4, 64, P, 0, P, None) != 0 and b"gen_cap" in lib.qspec_last_error()
    rc = lib.qspec_sample_top_k_top_p_min_p(None, None, None, None, None, None, 0, 0, None, P, P, 1, 4, 16, P, None)
    assert rc != 0 and b"logits" in lib.qspec_last_error()
    rc = lib.qspec_sample_top_k_top_p_min_p_seeded(P, None, None, None, None, None, 0, 0, None, P, P, 1, 8, 16, P, P, P, 1, 4, 0, 2,
                                                   P, None)
    assert rc != 0 and b"does not cover" in lib.qspec_last_error()


def test_engine_slot_arrays_follow_set_sampling_params_and_free_slot():
    eng = HostEngine()
    s = eng.sampling
    eng.set_sampling_params(1, 0.8, 50, 0.9)                      # nothing new asked for: nothing new allocated
    assert s._lp_host is None and s.tok_table is None and not s.processing_on(eng.active_slots())
    eng.set_sampling_params(2, 0.8, min_p=0.05, repetition_penalty=1.2, frequency_penalty=0.1, presence_penalty=-0.5,
                            min_tokens=4, stop_token_ids=(7, 9))
    assert s.tok_table.shape == (4, 64) and s.proc_logits_v.shape == (16, 64)
    assert s.samp_minp.tolist() == pytest.approx([0, 0, 0.05, 0]) and s.v_samp_minp[8:12].tolist() == pytest.approx([0.05] * 4)
    assert s.lp_rep.tolist() == [1, 1, float(np.float16(1.2)), 1] and s.lp_freq[2] == np.float16(0.1) and s.lp_pres[2] == -0.5
    assert s.lp_min_tokens.tolist() == [0, 0, 4, 0] and s.lp_n_stop.tolist() == [0, 0, 2, 0]
    assert s.lp_stop_ids[2, :2].tolist() == [7, 9] and s.lp_need.tolist() == [0, 0, 1, 0]
    assert not s.processing_on(eng.active_slots())   # the slot is not occupied yet
    eng._len_ub[2] = 10
    assert s.processing_on(eng.active_slots())
    eng.set_sampling_params(3, 0.0, min_p=0.3, min_tokens=2, stop_token_ids=(1,))     # greedy: min_p is reset, the rest stays
    assert float(s.samp_minp[3]) == 0.0 and int(s.lp_min_tokens[3]) == 2 and int(s.lp_need[3]) == 0
    eng.set_sampling_params(0, 1.0, min_tokens=5)                 # min_tokens without stop ids masks nothing: neutral
    assert s._lp_host[0] == s._LP_NEUTRAL
    eng.free_slot(2)
    assert s._lp_host[2] == s._LP_NEUTRAL and s.lp_need.tolist() == [0, 0, 0, 0] and float(s.samp_minp[2]) == 0.0
    assert float(s.lp_rep[2]) == 1.0 and int(s.lp_n_stop[2]) == 0 and not s.processing_on(eng.active_slots())


def test_engine_refuses_bad_values_and_enqueues_nothing():
    eng = HostEngine()
    s = eng.sampling
    for kw in (dict(stop_token_ids=tuple(range(17)), min_tokens=1), dict(min_p=1.5), dict(min_p=-0.1),
               dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(min_tokens=-1), dict(presence_penalty=float("nan")),
               dict(frequency_penalty=1e9)):
        with pytest.raises(ValueError):
            eng.set_sampling_params(1, 0.8, **kw)
        assert s._lp_host is None or s._lp_host[1] == s._LP_NEUTRAL
        assert s._samp_host[1] == (0.0, -1, 1.0)   # refused before anything was uploaded
    eng._len_ub[1] = 5                                            # an occupied slot has no table row to count in
    with pytest.raises(ValueError, match="admitted"):
        eng.set_sampling_params(1, 0.8, repetition_penalty=1.1)
    eng.set_sampling_params(1, 0.8, min_p=0.1)                    # (min_p needs none)


# ---------------------------------------------------------------------- worker, on a scripted engine
class _ScriptedEngine:
    def __init__(self, *a, **kw):
        self.calls = []
        self.gen_tokens = torch.zeros(4, 8, dtype=torch.int64)

    def set_sampling_params(self, slot, *a, **kw):
        if len(kw.get("stop_token_ids", ())) > 16:
            raise ValueError("too many stop ids")
        self.calls.append(("set", slot, a, kw))

    def add_sequences_to(self, *a, **kw):
        self.calls.append(("add", a, kw))

    def free_slot(self, slot):
        self.calls.append(("free", slot))


def _worker(engine):
    w = W.SpecDecodeWorker.__new__(W.SpecDecodeWorker)
    w.engine, w.max_num_seqs, w._slots = engine, 4, {}
    from collections import defaultdict
    w._request_id_seq_id_mapping = defaultdict(set)
    return w


def _req(rid, sp, prompt=(1, 2, 3), outputs=()):
    return W.SequenceGroupMetadata(request_id=rid, is_prompt=True, seq_data={0: W.SequenceData(list(prompt), list(outputs))},
                                   sampling_params=sp)


def test_worker_forwards_the_new_fields_only_when_set():
    eng = _ScriptedEngine()
    w = _worker(eng)
    sp = W.SamplingParams(temperature=0.7, min_p=0.05, presence_penalty=0.1, frequency_penalty=0.2, repetition_penalty=1.2,
                          min_tokens=32, stop_token_ids=[9, 4])
    w._admit([_req("a", sp), _req("b", W.SamplingParams(temperature=0.7)), _req("c", None)])
    sets = [c for c in eng.calls if c[0] == "set"]
    assert sets[0][3] == dict(min_p=0.05, presence_penalty=0.1, frequency_penalty=0.2, repetition_penalty=1.2, min_tokens=32,
                              stop_token_ids=(4, 9))
    # default-valued requests: exactly the calls they produced before -- positional temperature / top_k / top_p, no keyword
    assert sets[1] == ("set", 1, (0.7, -1, 1.0), {}) and sets[2] == ("set", 2, (0.0, -1, 1.0), {})
    add = [c for c in eng.calls if c[0] == "add"][0]
    assert add[2] == {} and len(add[1]) == 3
    # a vLLM object: all_stop_token_ids (stop ids + EOS) wins
    eng.calls.clear()
    vsp = SimpleNamespace(temperature=1.0, top_k=-1, top_p=1.0, seed=None, min_p=0.0, presence_penalty=0.0, frequency_penalty=0.0,
                          repetition_penalty=1.0, min_tokens=3, stop_token_ids=[5], all_stop_token_ids={5, 2})
    w._admit([_req("d", vsp)])
    assert eng.calls[0][3] == dict(min_tokens=3, stop_token_ids=(2, 5))


def test_worker_passes_the_prompt_length_of_a_recomputed_request_and_refuses_17_stop_ids():
    eng = _ScriptedEngine()
    w = _worker(eng)
    sp = W.SamplingParams(repetition_penalty=1.3)
    w._admit([_req("a", sp, prompt=(1, 2, 3), outputs=(7, 7)), _req("b", sp, prompt=(4, 5))])
    add = [c for c in eng.calls if c[0] == "add"][0]
    assert add[1][1] == [[1, 2, 3, 7, 7], [4, 5]] and add[2] == dict(num_prompt_tokens=[3, None])
    # a recomputed request WITHOUT the new fields is admitted as before (prompt + outputs as one prompt, no keyword)
    eng.calls.clear()
    w._admit([_req("c", W.SamplingParams(), prompt=(1, 2), outputs=(3,))])
    assert [c for c in eng.calls if c[0] == "add"][0][2] == {}
    eng.calls.clear()
    bad = W.SamplingParams(min_tokens=2, stop_token_ids=list(range(17)))
    with pytest.raises(ValueError):
        w._admit([_req("e", bad)])
    assert not any(c[0] == "add" for c in eng.calls) and "e" not in w._slots
