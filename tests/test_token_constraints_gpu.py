"""Token constraints on the GPU: the constrained pre-pass kernel and the admission kernel against tests/constraint_cases.py
(itself pinned to the reference fixture by tests/test_token_constraints_cpu.py), the engine's constrained cycle, and requests
through the worker."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import constraint_cases as cc  # noqa: E402
import logit_cases as lc  # noqa: E402
from test_token_constraints_cpu import fixture_rows  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


@pytest.fixture(scope="module")
def ops():
    from qspec_amd import ops as O
    return O


def _slot_state(ops, V, slots, gen_cap=512):
    """Device state of `slots` (dicts: prompt, outputs, n_pre, params, constraints, active).  The first n_pre outputs are those
    the request had BEFORE its admission (token table + tail), the rest sit in gen_tokens.  Returns (plain kwargs, constraint
    arrays + gen_tokens)."""
    n = len(slots)
    table, counted = ops.new_logit_table(n, V, DEV)
    tc = ops.TokenConstraints(n, V, DEV)
    tc.deny.fill_(0x5A5A5A5A)                        # stale rows: only a slot whose flag says so may read its row
    tc.bias_ids.fill_(7); tc.bias_vals.fill_(50.0); tc.words.fill_(3); tc.word_lens.fill_(2); tc.tail.fill_(3)
    gen = np.full((n, gen_cap), -1, np.int64)
    for s, sl in enumerate(slots):
        outs, n_pre = sl["outputs"], sl.get("n_pre", 0)
        ops.logit_table_set_prompt(table, counted, s, dev(np.array(sl["prompt"], np.int64)),
                                   dev(np.array(outs, np.int64)) if outs else None)
        gen[s, :len(outs) - n_pre] = outs[n_pre:]
        c = sl.get("constraints")
        if c is not None and not c.empty():
            ops.token_constraints_set(tc, s, c.logit_bias, c.allowed, [list(w) for w in c.bad_words])
            ops.token_constraints_set_tail(tc, s, outs[:n_pre])
    P = [sl["params"] for sl in slots]
    stop = np.zeros((n, 16), np.int32)
    for s, p in enumerate(P):
        stop[s, :len(p.stop_ids)] = p.stop_ids
    plain = dict(tok_table=table, repetition=dev(np.array([p.repetition for p in P], np.float16)),
                 frequency=dev(np.array([p.frequency for p in P], np.float16)),
                 presence=dev(np.array([p.presence for p in P], np.float16)),
                 min_tokens=dev(np.array([p.min_tokens for p in P], np.int32)),
                 gen_base=dev(np.array([sl.get("n_pre", 0) for sl in slots], np.int32)),
                 gen_lens=dev(np.array([len(sl["outputs"]) - sl.get("n_pre", 0) for sl in slots], np.int32)), stop_ids=dev(stop),
                 num_stop_ids=dev(np.array([len(p.stop_ids) for p in P], np.int32)),
                 active_lens=dev(np.array([5 if sl["active"] else 0 for sl in slots], np.int32)))
    return plain, tc.arrays() + (dev(gen),)


def _constrained(ops, raw, out, plain, cons, **kw):
    names = ("deny", "meta", "bias_ids", "bias_vals", "words", "word_lens", "tail", "gen_tokens")
    return ops.process_logits_constrained(raw, out, **plain, **dict(zip(names, cons)), **kw)


def test_constrained_prepass_reference_fixture_bit_exact(ops, golden_dir):
    g = np.load(os.path.join(golden_dir, "token_constraints.npz"))
    V = g["tc_raw"].shape[1]
    n = 0
    for i, name, raw_row, prompt, outs, infl, p, c in fixture_rows(g):
        for n_pre in sorted({0, len(outs) // 2, len(outs)}):     # committed / split over the admission / all before it
            plain, cons = _slot_state(ops, V, [dict(prompt=prompt, outputs=outs, n_pre=n_pre, params=p, constraints=c, active=True)])
            raw = dev(g["tc_raw"][i:i + 1])
            out = torch.full_like(raw, float("nan"))
            _constrained(ops, raw, out, plain, cons, draft_ids=dev(np.array(infl, np.int64).reshape(-1, 1)) if infl else None,
                         rows_per_seq=1, j_base=len(infl))
            assert np.array_equal(_bits(host(out)[0]), _bits(g["tc_expected"][i])), (name, n_pre)
            assert np.array_equal(_bits(host(raw)[0]), _bits(g["tc_raw"][i]))           # out of place
            n += 1
    assert n >= 40


@pytest.mark.parametrize("T,rows_per_seq", cc.PREPASS_SHAPES)
def test_constrained_prepass_full_vocabulary_bit_exact(ops, T, rows_per_seq):
    V = cc.FULL_VOCAB
    case = cc.make_constrained_case(V, T, rows_per_seq, seed=2000 * T + rows_per_seq)
    plain, cons = _slot_state(ops, V, case["slots"])
    raw = dev(case["raw"])
    buf = torch.full((T + 2, V), float("nan"), dtype=torch.float16, device=DEV)      # a guard row on either side
    kw = dict(draft_ids=dev(case["drafts"]) if case["n_draft"] else None, rows_per_seq=rows_per_seq, j_base=case["j_base"])
    _constrained(ops, raw, buf[1:T + 1], plain, cons, **kw)
    want, got = cc.expected_constrained(case), host(buf)
    assert np.isnan(got[0]).all() and np.isnan(got[T + 1]).all()
    for t in range(T):
        assert np.array_equal(_bits(got[t + 1]), _bits(want[t])), (t, int((_bits(got[t + 1]) != _bits(want[t])).sum()))
    kinds = [0, 0, 0]
    for sl in case["slots"]:
        c = sl["constraints"]
        kinds = [kinds[0] + bool(c.logit_bias), kinds[1] + (c.allowed is not None), kinds[2] + bool(c.bad_words)]
    if T >= 16:
        assert all(kinds), kinds
    # unconstrained slots inside the constrained call: the bits of the plain entry
    ref = torch.full((T, V), float("nan"), dtype=torch.float16, device=DEV)
    ops.process_logits(raw, ref, **plain, **kw)
    ref = host(ref)
    free = [t for t in range(T) if case["slots"][t // rows_per_seq]["constraints"].empty()]
    assert free or len(case["slots"]) == 1
    for t in free:
        assert np.array_equal(_bits(got[t + 1]), _bits(ref[t])), t
    assert np.array_equal(_bits(host(raw)), _bits(case["raw"]))


def test_constrained_prepass_odd_vocabulary_slot_ids_and_slot_reuse(ops):
    """A vocabulary that is no multiple of 8 (scalar path), rows mapped to slots through slot_ids, and a slot whose constraints
    are cleared: its rows are the plain entry's again although its deny row and lists still hold the old request's."""
    V = 1003
    case = cc.make_constrained_case(V, 4, 1, seed=5)
    case["j_base"], case["n_draft"], case["drafts"] = 0, 0, np.zeros((0, 4), np.int64)
    for sl in case["slots"]:
        sl["active"] = True
    case["slots"][2]["constraints"] = cc.Constraints({5: 1.0, 1002: -2.0, 1000: 100.0}, tuple(range(3, 1003)), ((1001,), (4,)))
    case["slots"][3]["outputs"].append(9)
    case["slots"][3]["constraints"] = cc.Constraints({}, None, ((9, 1002), (8,)))
    plain, cons = _slot_state(ops, V, case["slots"])
    raw = dev(case["raw"])
    order = [3, 2, 1, 0]
    out = torch.full_like(raw, float("nan"))
    _constrained(ops, raw, out, plain, cons, slot_ids=dev(np.array(order, np.int32)))
    for t, s in enumerate(order):
        sl = case["slots"][s]
        want = cc.process_row_constrained(case["raw"][t], sl["prompt"], sl["outputs"], [], sl["params"], sl["constraints"])
        assert np.array_equal(_bits(host(out)[t]), _bits(want)), (t, s)
    assert np.isneginf(host(out)[0][1002]) and np.isneginf(host(out)[1][:3]).all()
    tc = ops.TokenConstraints(4, V, DEV)
    tc.deny, tc.meta, tc.bias_ids, tc.bias_vals, tc.words, tc.word_lens, tc.tail = cons[:7]
    ops.token_constraints_set(tc, 2)                                                  # the request in slot 2 has left
    assert host(tc.meta)[2].tolist() == [0, 0, 0, 0] and int(host(tc.deny)[2].view(np.uint32)[0] & 7) == 7
    _constrained(ops, raw, out, plain, cons, slot_ids=dev(np.array(order, np.int32)))
    sl = case["slots"][2]
    assert np.array_equal(_bits(host(out)[1]), _bits(lc.process_row(case["raw"][1], sl["prompt"], sl["outputs"], [], sl["params"])))


def test_admission_kernel_builds_the_deny_row_and_the_lists(ops):
    V = 1000
    tc = ops.TokenConstraints(3, V, DEV)
    tc.deny.fill_(-1)
    ops.token_constraints_set(tc, 1, {900: -1.5, 3: 2.0, 31: 0.25}, [999, 0, 31, 32, 64], [[31], [5], [7, 8], [9, 10, 11], [7, 8]])
    deny = host(tc.deny).view(np.uint32)
    bits = ((deny[1][:, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1)[:V]
    assert sorted(np.nonzero(bits == 0)[0].tolist()) == [0, 32, 64, 999]             # allowed minus the single-token bad word 31
    assert (deny[0] == 0xFFFFFFFF).all() and (deny[2] == 0xFFFFFFFF).all()           # other slots untouched
    assert host(tc.meta).tolist() == [[0, 0, 0, 0], [3, 3, 2, 0], [0, 0, 0, 0]]
    assert host(tc.bias_ids)[1, :3].tolist() == [3, 31, 900] and host(tc.bias_vals)[1, :3].tolist() == [2.0, 0.25, -1.5]
    assert host(tc.words)[1, 0, :2].tolist() == [7, 8] and host(tc.words)[1, 1, :3].tolist() == [9, 10, 11]
    assert host(tc.word_lens)[1, :2].tolist() == [2, 3]
    ops.token_constraints_set(tc, 1, None, None, [[4]])                               # no allowed set: only the bad word's bit
    bits = ((host(tc.deny).view(np.uint32)[1][:, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(-1)[:V]
    assert np.nonzero(bits)[0].tolist() == [4] and host(tc.meta)[1].tolist() == [3, 0, 0, 0]
    ops.token_constraints_set_tail(tc, 1, list(range(100, 120)))
    assert host(tc.tail)[1].tolist() == list(range(113, 120)) and host(tc.meta)[1].tolist() == [3, 0, 0, 7]
    ops.token_constraints_set_tail(tc, 1, [41, 42])
    assert host(tc.tail)[1].tolist() == [-1] * 5 + [41, 42] and int(host(tc.meta)[1][3]) == 2
    for bad in (dict(logit_bias={t: 1.0 for t in range(513)}), dict(bad_words_token_ids=[[t, t + 1] for t in range(33)]),
                dict(bad_words_token_ids=[list(range(9))])):
        with pytest.raises(ValueError):
            ops.token_constraints_set(tc, 0, **bad)


def test_row_without_a_finite_logit_is_all_minus_inf_and_samples_token_zero(ops):
    """An allowed set of one token that a matched bad word bans: NaN in the reference; here the row is -inf everywhere and the
    sampling front end emits token 0 (its argmax finds no candidate).  Plain arithmetic, nothing faults."""
    V = 4096
    c = cc.Constraints({}, (77,), ((5, 77),))
    plain, cons = _slot_state(ops, V, [dict(prompt=[1], outputs=[9, 5], n_pre=0, params=lc.Params(), constraints=c, active=True)])
    raw = dev((np.random.default_rng(0).standard_normal((1, V)) * 3).astype(np.float16))
    out = torch.full_like(raw, float("nan"))
    _constrained(ops, raw, out, plain, cons)
    assert np.isneginf(host(out)).all()
    probs = torch.zeros(1, V, dtype=torch.float32, device=DEV)
    for temp in (0.0, 1.0):
        tok = torch.full((1,), -7, dtype=torch.int64, device=DEV)
        ops.sample_top_k_top_p(out, probs, tok, dev(np.array([temp], np.float32)), None, None)
        assert int(tok[0]) == 0


# ---------------------------------------------------------------------- engine
@pytest.fixture(scope="module")
def tiny():
    from qspec_amd.model import QuarotLlamaConfig, QuarotLlamaForCausalLM
    cfg = QuarotLlamaConfig(1024, 3584, 8, 2, 2, 2048, 1e-5, 10000.0, 512, "tiny")
    return QuarotLlamaForCausalLM(cfg, DEV).init_synthetic(seed=1, lm_head_std=0.05)


def _engine(tiny, use_graph, seed=0):
    from qspec_amd.spec_decode import QSpecEngine
    return QSpecEngine(tiny, 3, 4, max_model_len=256, block_size=16, max_new_tokens=64, use_graph=use_graph, seed=seed)


def _prompts():
    rng = np.random.default_rng(31)
    return [rng.integers(0, 60, n).tolist() for n in (21, 30, 9, 44)]


def _plain_outputs(tiny, prompts, cycles=10):
    eng = _engine(tiny, False)
    eng.add_sequences_to(list(range(len(prompts))), prompts)
    for _ in range(cycles):
        eng.step()
    return eng.generated()


def _kws(plain):
    """Four requests: words cut from the request's own unconstrained greedy output (so they WOULD be emitted), a tiny and a large
    allowed set, biases, penalties and min_tokens beside them, one sampled and seeded, one unconstrained."""
    g0, g1, g3 = plain[0], plain[1], plain[3]
    return [dict(temperature=0.0, bad_words_token_ids=[g0[1:3], g0[3:6], g0[4:6] + [g0[7]], [g0[0]], g0[2:10]],
                 logit_bias={g0[1]: -2.0, 5: 3.0}, repetition_penalty=1.2),
            dict(temperature=0.9, seed=77, allowed_token_ids=sorted(set(g1[:6]) | set(range(100, 140))),
                 logit_bias={t: 1.5 for t in range(100, 120)}, bad_words_token_ids=[[101], [g1[0], g1[1]]], min_p=0.02),
            dict(temperature=0.8, seed=5),
            dict(temperature=0.0, allowed_token_ids=[t for t in range(2048) if t != g3[0]], min_tokens=30,
                 stop_token_ids=(g3[1], 17), bad_words_token_ids=[g3[2:4]], frequency_penalty=0.3)]


def _pc(kw):
    p = lc.Params(kw.get("repetition_penalty", 1.0), kw.get("frequency_penalty", 0.0), kw.get("presence_penalty", 0.0),
                  kw.get("min_tokens", 0), tuple(kw.get("stop_token_ids", ())))
    a = kw.get("allowed_token_ids")
    c = cc.Constraints(dict(kw.get("logit_bias") or {}), None if a is None else tuple(a),
                       tuple(tuple(w) for w in kw.get("bad_words_token_ids") or ()))
    return p, c


class _Tap:
    """Records every pre-pass call of an eager engine: (raw logits, processed logits, rows_per_seq, j_base, in-flight ids)."""

    def __init__(self, eng):
        self.calls, inner = [], eng._process

        def process(logits, out, rows_per_seq, j_base, draft_ids, active_lens, slot_ids=None, constrained=None):
            res = inner(logits, out, rows_per_seq, j_base, draft_ids, active_lens, slot_ids=slot_ids, constrained=constrained)
            torch.cuda.synchronize()
            self.calls.append((host(logits).copy(), host(res).copy(), rows_per_seq, j_base,
                               None if draft_ids is None else host(draft_ids).copy()))
            return res
        eng._process = process


def test_engine_every_draft_and_verify_row_equals_the_restatement(tiny):
    prompts = _prompts()
    kws = _kws(_plain_outputs(tiny, prompts))
    eng = _engine(tiny, False)
    for b in range(4):
        eng.set_sampling_params(b, **kws[b])
    tap = _Tap(eng)
    eng.add_sequences_to([0, 1, 2, 3], prompts)
    assert len(tap.calls) == 1                                                   # the first token: j = 0, nothing in flight
    raw, proc, _, _, _ = tap.calls.pop()
    for b in range(4):
        p, c = _pc(kws[b])
        assert np.array_equal(_bits(proc[b]), _bits(cc.process_row_constrained(raw[b], prompts[b], [], [], p, c))), b
    k, rows = eng.k, 0
    for cyc in range(5):
        before = eng.generated()
        eng.step()
        assert len(tap.calls) == k + 1
        for raw, proc, rps, j_base, drafts in tap.calls:
            for t in range(raw.shape[0]):
                b, j = t // rps, j_base + t % rps
                p, c = _pc(kws[b])
                want = cc.process_row_constrained(raw[t], prompts[b], before[b], [int(d) for d in drafts[:j, b]], p, c)
                assert np.array_equal(_bits(proc[t]), _bits(want)), (cyc, rps, b, j)
                rows += 1
        tap.calls.clear()
    assert rows == 5 * (3 * 4 + 16) and eng._mode_constrained and eng._mode_processing
    g = eng.generated()
    assert all(len(x) >= 6 for x in g)
    eng.step_no_spec()                                                           # the non-speculative step: j = 0
    raw, proc, rps, j_base, _ = tap.calls.pop()
    for b in range(4):
        p, c = _pc(kws[b])
        assert np.array_equal(_bits(proc[b]), _bits(cc.process_row_constrained(raw[b], prompts[b], g[b], [], p, c))), b


def _violations(tokens, kw):
    """Positions where `tokens` (a request's whole output) breaks its constraints."""
    bad = []
    allowed = kw.get("allowed_token_ids")
    for i, t in enumerate(tokens):
        if allowed is not None and t not in allowed:
            bad.append(("allowed", i, t))
        for w in kw.get("bad_words_token_ids") or ():
            if i + 1 >= len(w) and list(tokens[i + 1 - len(w):i + 1]) == list(w):
                bad.append(("word", i, tuple(w)))
    return bad


def test_engine_graph_equals_eager_recover_replays_and_constraints_hold(tiny):
    prompts = _prompts()
    plain = _plain_outputs(tiny, prompts)
    kws = _kws(plain)
    runs = []
    for use_graph, disturbed in ((False, False), (True, False), (True, True)):
        eng = _engine(tiny, use_graph)
        for b in range(4):
            eng.set_sampling_params(b, **kws[b])
        eng.add_sequences_to([0, 1, 2, 3], prompts)
        for i in range(5):
            eng.step()
            torch.cuda.synchronize()
            if disturbed and i in (1, 3):
                eng.recover()                                                    # after a healthy cycle: the same tokens again
        runs.append(eng.generated())
        if use_graph:
            assert eng._graph_c is not None and eng._graph is None and eng._graph_s is None and eng._graph_p is None
            # a new request with other constraints in a freed slot: same graph object, no capture
            g = eng._graph_c
            eng.free_slot(2)
            eng.set_sampling_params(2, 0.0, allowed_token_ids=[11, 12, 13], logit_bias={12: 100.0})
            eng.add_sequence(2, prompts[2])
            eng.step(); eng.step()
            g2 = eng.generated()[2]
            assert eng._graph_c is g and len(g2) >= 3 and set(g2) == {12}, g2
    assert runs[0] == runs[1] == runs[2]
    for b in (0, 1, 3):
        assert _violations(runs[0][b], kws[b]) == [], b
        assert _violations(plain[b], kws[b]) != []                               # the unconstrained output breaks every one
    assert not any(t in (plain[3][1], 17) for t in runs[0][3][:30])              # min_tokens behind the constraints


def test_engine_isolation_slot_reuse_and_return_to_the_parent_graphs(tiny):
    prompts = _prompts()
    seeded = dict(temperature=0.8, top_k=50, top_p=0.9, seed=20261016)
    alone = _engine(tiny, True)
    alone.set_sampling_params(0, **seeded)
    alone.add_sequence(0, prompts[0])
    both = _engine(tiny, True, seed=7)
    both.set_sampling_params(2, **seeded)
    both.add_sequence(2, prompts[0])
    both.set_sampling_params(1, 0.0, allowed_token_ids=list(range(50, 90)), bad_words_token_ids=[[60], [61, 62]])
    both.add_sequence(1, prompts[1])
    for _ in range(3):
        alone.step(); both.step()
    # an engine that never saw a constraint: none of the new arrays, only the graphs it always held
    assert alone._graph_s is not None and alone._graph_c is None and alone._graph_p is None and alone._graph is None
    assert alone.tc is None and alone._tc_host is None and alone._lp_host is None and alone.tok_table is None
    assert both._graph_c is not None and both._graph_s is None and both._graph_p is None and both._mode_constrained
    assert alone.generated()[0] == both.generated()[2] and len(alone.generated()[0]) >= 4
    assert all(50 <= t < 90 and t != 60 for t in both.generated()[1])
    both.free_slot(1)                                                            # the last constrained request leaves
    alone.step(); both.step()
    assert not both._mode_constrained and not both._mode_processing and both._graph_s is not None
    assert alone.generated()[0] == both.generated()[2]
    # slot reuse: an unconstrained request in the slot the constrained one left emits what it emits in a fresh engine
    assert host(both.tc.meta)[1].tolist() == [0, 0, 0, 0] and int(host(both.tc.deny)[1].view(np.uint32).max()) != 0
    # (a SEEDED sampled request: its tokens depend on its own seed and positions alone, whoever shares the batch)
    reuse = dict(temperature=0.8, seed=5)
    both.set_sampling_params(1, **reuse)
    both.add_sequence(1, prompts[3])
    fresh = _engine(tiny, False)
    fresh.set_sampling_params(1, **reuse)
    fresh.add_sequence(1, prompts[3])
    for _ in range(3):
        both.step(); fresh.step()
    assert both.generated()[1] == fresh.generated()[1] and not both._mode_constrained
    # ... and with a penalty (the processed cycle, plain entry) while the old deny row still sits in the slot
    pen = dict(temperature=0.9, min_p=0.05, repetition_penalty=1.2, presence_penalty=-0.25, seed=77)
    both.free_slot(1); fresh.free_slot(1)
    both.set_sampling_params(1, **pen); fresh.set_sampling_params(1, **pen)
    both.add_sequence(1, prompts[3]); fresh.add_sequence(1, prompts[3])
    for _ in range(2):
        both.step(); fresh.step()
    assert both._mode_processing and not both._mode_constrained and both._graph_p is not None and fresh.tc is None
    assert both.generated()[1] == fresh.generated()[1]


# ---------------------------------------------------------------------- worker: requests through execute_model
def _worker(tiny, seed=0):
    from qspec_amd.spec_decode import create_spec_worker
    from qspec_amd.spec_decode.worker import SpeculativeConfig
    w = create_spec_worker(model_config=tiny.config, model=tiny, speculative_config=SpeculativeConfig(3), max_num_seqs=4,
                           max_model_len=256, block_size=16, device=DEV, seed=seed)
    w.init_device()
    w.initialize_cache(64, 0)
    return w


def _run(w, reqs, cycles, preempt=None):
    """reqs: [(request id, prompt, SamplingParams)].  Returns the tokens per request.  preempt = (request id, cycle): before that
    cycle the request comes back as a prompt carrying its outputs (recomputation after a preemption)."""
    from qspec_amd.spec_decode import ExecuteModelRequest, SequenceGroupMetadata
    from qspec_amd.spec_decode.worker import SequenceData
    sgs, toks = [], {rid: [] for rid, _, _ in reqs}
    for i, (rid, prompt, sp) in enumerate(reqs):
        sg = SequenceGroupMetadata(rid, True, {i: SequenceData(list(prompt))}, sampling_params=sp)
        out = w.execute_model(ExecuteModelRequest([sg], num_lookahead_slots=0))
        toks[rid].append(out[0].token_ids()[0])
        sg.is_prompt = False
        sgs.append(sg)
    for cyc in range(cycles):
        if preempt is not None and preempt[1] == cyc:
            pos = [s.request_id for s in sgs].index(preempt[0])
            sg = sgs[pos]
            data = next(iter(sg.seq_data.values()))
            data.output_token_ids = list(toks[preempt[0]])
            sg.is_prompt = True
            out = w.execute_model(ExecuteModelRequest([sg], num_lookahead_slots=0))
            toks[preempt[0]].append(out[0].token_ids()[0])
            sg.is_prompt = False
            data.output_token_ids = []
        outs = w.execute_model(ExecuteModelRequest(sgs, num_lookahead_slots=3))
        for pos, sg in enumerate(sgs):
            toks[sg.request_id] += [t for t in (o.token_ids()[pos] for o in outs) if t != -1]
    return toks


def _ngram_positions(tokens, w):
    return [i for i in range(len(tokens) - len(w) + 1) if list(tokens[i:i + len(w)]) == list(w)]


def test_execute_model_allowed_banned_and_biased_tokens(tiny):
    from qspec_amd.spec_decode.worker import SamplingParams
    prompts = _prompts()
    base = _run(_worker(tiny), [("a", prompts[0], SamplingParams()), ("b", prompts[1], SamplingParams())], 5)
    allowed = sorted(set(range(200, 260)) | {base["a"][0]})
    banned = base["a"][0]
    reqs = [("a", prompts[0], SamplingParams(allowed_token_ids=allowed, bad_words_token_ids=[[banned]])),
            ("b", prompts[1], SamplingParams(temperature=0.9, seed=3, allowed_token_ids=list(range(300, 420)), logit_bias={"301": -100.0})),
            ("c", prompts[2], SamplingParams(logit_bias={1234: 100.0})),
            ("d", prompts[3], SamplingParams(temperature=1.0, seed=9, bad_words_token_ids=[[t] for t in range(0, 2048, 2)]))]
    got = _run(_worker(tiny), reqs, 5)
    assert all(len(v) >= 6 for v in got.values())
    assert all(t in allowed and t != banned for t in got["a"]), got["a"]
    assert all(300 <= t < 420 and t != 301 for t in got["b"]), got["b"]
    assert got["c"] == [1234] * len(got["c"])                                    # +100 on one id makes it the greedy token
    assert all(t % 2 == 1 for t in got["d"]), got["d"]
    assert any(t not in allowed for t in base["a"]) and banned in base["a"]      # (what an engine that ignores the fields emits)


@pytest.mark.parametrize("temperature", [0.0, 0.7])
def test_execute_model_banned_ngrams_across_cycles_drafts_and_preemption(tiny, temperature):
    """Bigrams / trigrams cut from the request's OWN unconstrained output at chosen places: straddling the first token and the
    first cycle, straddling two cycles, inside one cycle's draft tokens, and straddling a preemption.  Unconstrained they are
    emitted verbatim (that is where they were cut from); constrained they never appear.  A greedy request under speculation
    is rejection-sampled from the engine's stream (the reference does not make its probabilities one-hot), so only the seeded
    request is also required to follow its unconstrained output up to the banned token."""
    from qspec_amd.spec_decode.worker import SamplingParams
    prompts = _prompts()
    sp = dict(temperature=temperature, seed=11) if temperature else {}
    base = _run(_worker(tiny), [("a", prompts[0], SamplingParams(**sp))], 9)["a"]
    assert len(base) >= 10                                                       # (every cycle emits at least one token)
    # base[0] is the prompt pass's token, base[1:] come from the cycles, at most 4 per cycle: base[0:2] straddles the first token
    # and the first cycle, base[1:4] lies inside one cycle's rows wherever the cycles split, base[3:6] and base[7:10] each
    # straddle a cycle boundary or sit in draft tokens depending on the acceptance -- all banned at once, with a single token
    words = [base[0:2], base[1:4], base[3:6], base[7:10]]
    assert all(_ngram_positions(base, w) for w in words)
    for ws in ([words[0]], [words[1]], words[2:]):
        got = _run(_worker(tiny), [("a", prompts[0], SamplingParams(bad_words_token_ids=[list(w) for w in ws], **sp))], 9)["a"]
        assert len(got) >= 10 and all(_ngram_positions(got, w) == [] for w in ws), (ws, got)
        if temperature:   # a seeded request's tokens depend on its seed and positions alone: unchanged up to the first ban
            cut = min(_ngram_positions(base, w)[0] + len(w) - 1 for w in ws)
            assert got[:cut] == base[:cut] and got[cut] != base[cut], (ws, cut, got, base)
    # straddling a preemption: the request is re-admitted before cycle 2 with its outputs; the banned word starts in them
    pre = _run(_worker(tiny), [("a", prompts[0], SamplingParams(**sp))], 2)["a"]
    n = len(pre)                                                                 # outputs at the re-admission
    base_p = _run(_worker(tiny), [("a", prompts[0], SamplingParams(**sp))], 5, preempt=("a", 2))["a"]
    assert base_p[:n] == pre and len(base_p) >= n + 3
    for w in (base_p[n - 2:n + 1], base_p[n - 1:n + 2]):    # last token(s) before + first token(s) after
        if _ngram_positions(base_p, w)[0] + len(w) - 1 < n:
            continue                                                             # (the word already occurs earlier: not this case)
        got = _run(_worker(tiny), [("a", prompts[0], SamplingParams(bad_words_token_ids=[list(w)], **sp))], 5, preempt=("a", 2))["a"]
        assert _ngram_positions(got, w) == [], (w, got)
        if temperature:   # the word really came up: same tokens until its last one, which is replaced
            cut = _ngram_positions(base_p, w)[0] + len(w) - 1
            assert cut >= n and got[:cut] == base_p[:cut] and got[cut] != base_p[cut], (w, cut, got, base_p)
