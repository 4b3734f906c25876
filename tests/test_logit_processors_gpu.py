"""Logit processors on the GPU: the pre-pass kernel, the token table, min_p in the selection kernel and the engine's processed
cycle, against tests/logit_cases.py (itself pinned to the reference fixture by tests/test_logit_processors_cpu.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import logit_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def ops():
    from qspec_amd import ops as O
    return O


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def _slot_arrays(ops, V, slots):
    """Device state of `slots` (dicts: prompt, outputs, params, active): table built by set_prompt, parameter arrays."""
    n = len(slots)
    table, counted = ops.new_logit_table(n, V, DEV)
    table.fill_(0x5A5A5A5A)                                      # stale rows: set_prompt must clear what it builds on
    for s, sl in enumerate(slots):
        ops.logit_table_set_prompt(table, counted, s, dev(np.array(sl["prompt"], np.int64)),
                                   dev(np.array(sl["outputs"], np.int64)) if sl["outputs"] else None)
    P = [sl["params"] for sl in slots]
    stop = np.zeros((n, 16), np.int32)
    for s, p in enumerate(P):
        stop[s, :len(p.stop_ids)] = p.stop_ids
    return dict(tok_table=table, repetition=dev(np.array([p.repetition for p in P], np.float16)),
                frequency=dev(np.array([p.frequency for p in P], np.float16)),
                presence=dev(np.array([p.presence for p in P], np.float16)),
                min_tokens=dev(np.array([p.min_tokens for p in P], np.int32)), gen_base=dev(np.zeros(n, np.int32)),
                gen_lens=dev(np.array([len(sl["outputs"]) for sl in slots], np.int32)), stop_ids=dev(stop),
                num_stop_ids=dev(np.array([len(p.stop_ids) for p in P], np.int32)),
                active_lens=dev(np.array([5 if sl["active"] else 0 for sl in slots], np.int32)))


def test_process_logits_reference_fixture_bit_exact(ops, golden_dir):
    g = np.load(os.path.join(golden_dir, "logit_processors.npz"))
    V = g["pen_raw"].shape[1]
    strip = lambda a: [int(t) for t in a if 0 <= t < V]   # noqa: E731
    for i in range(g["pen_raw"].shape[0]):
        p = lc.Params(float(g["pen_rep"][i]), float(g["pen_freq"][i]), float(g["pen_pres"][i]), int(g["pen_min_tokens"][i]),
                      tuple(strip(g["pen_stop"][i])))
        infl = strip(g["pen_inflight"][i])
        arrs = _slot_arrays(ops, V, [dict(prompt=strip(g["pen_prompt"][i]), outputs=strip(g["pen_outputs"][i]), params=p, active=True)])
        raw = dev(g["pen_raw"][i:i + 1])
        out = torch.empty_like(raw)
        ops.process_logits(raw, out, draft_ids=dev(np.array(infl, np.int64).reshape(-1, 1)) if infl else None, rows_per_seq=1,
                           j_base=len(infl), **arrs)
        assert np.array_equal(_bits(host(out)[0]), _bits(g["pen_expected"][i])), i
        assert np.array_equal(_bits(host(raw)[0]), _bits(g["pen_raw"][i]))           # out of place


@pytest.mark.parametrize("T,rows_per_seq", lc.PREPASS_SHAPES)
def test_process_logits_full_vocabulary_bit_exact(ops, T, rows_per_seq):
    V = lc.FULL_VOCAB
    case = lc.make_prepass_case(V, T, rows_per_seq, seed=1000 * T + rows_per_seq)
    arrs = _slot_arrays(ops, V, case["slots"])
    raw = dev(case["raw"])
    out = torch.full_like(raw, float("nan"))
    ops.process_logits(raw, out, draft_ids=dev(case["drafts"]) if case["n_draft"] else None, rows_per_seq=rows_per_seq,
                       j_base=case["j_base"], **arrs)
    want = lc.expected_prepass(case)
    got = host(out)
    for t in range(T):
        assert np.array_equal(_bits(got[t]), _bits(want[t])), (t, int((_bits(got[t]) != _bits(want[t])).sum()))
    assert np.array_equal(_bits(got[0]), _bits(case["raw"][0]))                      # slot 0 is neutral: the input bits
    # neutral parameters everywhere: output bits == input bits
    for sl in case["slots"]:
        sl["params"], sl["active"] = lc.Params(), True
    arrs = _slot_arrays(ops, V, case["slots"])
    out.fill_(float("nan"))
    ops.process_logits(raw, out, draft_ids=dev(case["drafts"]) if case["n_draft"] else None, rows_per_seq=rows_per_seq,
                       j_base=case["j_base"], **arrs)
    assert np.array_equal(_bits(host(out)), _bits(case["raw"]))


def test_process_logits_odd_vocabulary_and_slot_ids(ops):
    """A vocabulary that is no multiple of 8 (scalar path) and rows mapped to slots through slot_ids."""
    V = 1003
    case = lc.make_prepass_case(V, 2, 1, seed=5)
    case["j_base"], case["n_draft"], case["drafts"] = 0, 0, np.zeros((0, 2), np.int64)
    arrs = _slot_arrays(ops, V, case["slots"] + case["slots"][::-1])                 # four slots; rows use slots 3 and 2
    raw = dev(case["raw"])
    out = torch.empty_like(raw)
    ops.process_logits(raw, out, slot_ids=dev(np.array([3, 2], np.int32)), **arrs)
    want = lc.expected_prepass(case)
    assert np.array_equal(_bits(host(out)[0]), _bits(lc.process_row(case["raw"][0], case["slots"][0]["prompt"],
                                                                    case["slots"][0]["outputs"], [], case["slots"][0]["params"])))
    assert np.array_equal(_bits(host(out)[1]), _bits(lc.process_row(case["raw"][1], case["slots"][1]["prompt"],
                                                                    case["slots"][1]["outputs"], [], case["slots"][1]["params"])))
    assert want.shape == (2, V)


def test_token_table_set_prompt_and_catch_up_against_bincount(ops):
    rng = np.random.default_rng(11)
    B, V, cap = 4, 4096, 64
    table, counted = ops.new_logit_table(B, V, DEV)
    table.fill_(-1)
    prompts = [rng.integers(0, 50, n).tolist() for n in (7, 300, 1, 40)]
    prev = [[], rng.integers(0, 50, 25).tolist(), [], [3, 3, 3]]                      # outputs of re-admitted requests
    for b in range(B):
        ops.logit_table_set_prompt(table, counted, b, dev(np.array(prompts[b], np.int64)),
                                   dev(np.array(prev[b], np.int64)) if prev[b] else None)
    gen = np.full((B, cap), -1, np.int64)
    gen_tokens, gen_lens = dev(gen), torch.zeros(B, dtype=torch.int32, device=DEV)
    need = dev(np.array([1, 1, 0, 1], np.int32))
    lens = [0] * B

    def expect(b):
        w = np.bincount(np.array(prev[b] + gen[b, :lens[b]].tolist(), np.int64), minlength=V).astype(np.uint32)
        w[np.unique(prompts[b])] |= np.uint32(0x80000000)
        return w
    frozen = host(table)[2].copy()
    for step in range(6):
        for b in range(B):
            n = int(rng.integers(1, 5))                                               # 1 .. k+1 accepted tokens
            gen[b, lens[b]:lens[b] + n] = rng.integers(0, 50, n)
            lens[b] += n
        gen_tokens.copy_(dev(gen)); gen_lens.copy_(dev(np.array(lens, np.int32)))
        for _ in range(2):                                                            # the second call changes nothing
            ops.logit_table_catch_up(table, counted, need, gen_tokens, gen_lens)
            tb = host(table).view(np.uint32)
            for b in (0, 1, 3):
                assert np.array_equal(tb[b], expect(b)), (step, b)
            assert host(counted).tolist() == [lens[0], lens[1], 0, lens[3]]
    assert np.array_equal(host(table)[2], frozen)                                     # need == 0: left alone


def test_min_p_reference_fixture(ops, golden_dir):
    g = np.load(os.path.join(golden_dir, "logit_processors.npz"))
    lg = g["mp_logits"]
    T, V = lg.shape
    args = (dev(g["mp_temperature"]), dev(g["mp_top_k"]), dev(g["mp_top_p"]))
    for rep in range(2):
        probs = torch.full((T, V), -1.0, dtype=torch.float32, device=DEV)
        tok = torch.full((T,), -1, dtype=torch.int64, device=DEV)
        ops.sample_top_k_top_p(dev(lg), probs, tok, *args, exponential=dev(g["mp_E"]), min_p=dev(g["mp_min_p"]))
        pr, tk = host(probs), host(tok)
        for t in range(T):
            assert np.array_equal(pr[t] > 0, g["mp_keep"][t]), (t, (pr[t] > 0).sum(), g["mp_keep"][t].sum())
            assert np.abs(pr[t] - g["mp_probs"][t]).max() <= 1e-6 and tk[t] == g["mp_token"][t], t
    # min_p = 0 and min_p = None: the existing entry point's bits; a greedy row ignores min_p and takes the argmax
    base_p = torch.empty(T, V, dtype=torch.float32, device=DEV); base_t = torch.empty(T, dtype=torch.int64, device=DEV)
    ops.sample_top_k_top_p(dev(lg), base_p, base_t, *args, exponential=dev(g["mp_E"]))
    for mp in (None, torch.zeros(T, dtype=torch.float32, device=DEV)):
        ops.sample_top_k_top_p(dev(lg), probs, tok, *args, exponential=dev(g["mp_E"]), min_p=mp)
        assert torch.equal(probs.view(torch.int32), base_p.view(torch.int32)) and torch.equal(tok, base_t)
    temp0 = g["mp_temperature"].copy(); temp0[3] = 0.0
    ops.sample_top_k_top_p(dev(lg), probs, tok, dev(temp0), None, None, exponential=dev(g["mp_E"]), min_p=dev(g["mp_min_p"]))
    assert int(tok[3]) == int(np.argmax(lg[3])) and int((probs[3] > 0).sum()) == V
    # the seeded twin masks the same tokens
    seeds = torch.arange(T, dtype=torch.int64, device=DEV); on = torch.ones(T, dtype=torch.int32, device=DEV)
    ops.sample_top_k_top_p(dev(lg), probs, tok, *args, min_p=dev(g["mp_min_p"]), seq_seeds=seeds, seq_seeded=on,
                           base_pos=on, rows_per_seq=1, j_base=0, draw_stream=2)
    assert np.array_equal(host(probs) > 0, g["mp_keep"])
    assert all(g["mp_keep"][t][int(tok[t])] for t in range(T))


# ---------------------------------------------------------------------- engine
@pytest.fixture(scope="module")
def tiny():
    from qspec_amd.model import QuarotLlamaConfig, QuarotLlamaForCausalLM
    cfg = QuarotLlamaConfig(1024, 3584, 8, 2, 2, 2048, 1e-5, 10000.0, 512, "tiny")
    return QuarotLlamaForCausalLM(cfg, DEV).init_synthetic(seed=1, lm_head_std=0.05)


def _engine(tiny, use_graph, seed=0, sampler=None):
    from qspec_amd.spec_decode import QSpecEngine
    return QSpecEngine(tiny, 3, 4, max_model_len=256, block_size=16, max_new_tokens=64, use_graph=use_graph, seed=seed,
                       acceptance_sampler=sampler)


def _prompts(tiny):
    rng = np.random.default_rng(31)
    return [rng.integers(0, 60, n).tolist() for n in (21, 30, 9, 44)]       # a small alphabet: repeats for the penalties


STOP16 = tuple(range(0, 2048, 128))                                                      # sixteen stop ids
PEN = [dict(temperature=0.0, repetition_penalty=1.3, frequency_penalty=0.2, presence_penalty=0.5),
       dict(temperature=0.9, min_p=0.05, repetition_penalty=1.2, presence_penalty=-0.25, seed=77),
       dict(temperature=0.8, seed=5),                                                     # neutral, sampled
       dict(temperature=0.0, min_tokens=40, stop_token_ids=STOP16, frequency_penalty=0.4)]


def _params(kw):
    return lc.Params(kw.get("repetition_penalty", 1.0), kw.get("frequency_penalty", 0.0), kw.get("presence_penalty", 0.0),
                     kw.get("min_tokens", 0), tuple(kw.get("stop_token_ids", ())))


def _check_cycle(eng, prompts, before, kws):
    """After a cycle: every verify row and the last draft step's rows against process_row, target_probs against the sampler
    restatement of the processed rows."""
    k, B = eng.k, eng.B
    torch.cuda.synchronize()
    raw_v, proc_v = host(eng.scratch_verify.logits[:B * (k + 1)]), host(eng.proc_logits_v)
    raw_d, proc_d = host(eng.scratch_draft.logits[:B]), host(eng.proc_logits_d)
    drafts, probs = host(eng.draft_ids_kb), host(eng.target_probs)
    for b in range(B):
        p = _params(kws[b])
        d = [int(t) for t in drafts[:, b]]
        for j in range(k + 1):
            want = lc.process_row(raw_v[b * (k + 1) + j], prompts[b], before[b], d[:j], p)
            assert np.array_equal(_bits(proc_v[b * (k + 1) + j]), _bits(want)), (b, j)
            ref, _ = lc.sampler_probs(want, kws[b].get("temperature", 0.0), -1, 1.0, kws[b].get("min_p", 0.0))
            assert np.abs(probs[b, j] - ref).max() <= 1e-6, (b, j, np.abs(probs[b, j] - ref).max())
        want = lc.process_row(raw_d[b], prompts[b], before[b], d[:k - 1], p)
        assert np.array_equal(_bits(proc_d[b]), _bits(want)), (b, "draft")


@pytest.mark.parametrize("use_graph", [False, True])
def test_engine_processed_rows_bit_exact_over_several_cycles(tiny, use_graph):
    prompts = _prompts(tiny)
    eng = _engine(tiny, use_graph)
    for b in range(4):
        eng.set_sampling_params(b, **PEN[b])
    eng.add_sequences_to([0, 1, 2, 3], prompts)
    emitted = set()
    for _ in range(6):
        before = eng.generated()
        eng.step()
        _check_cycle(eng, prompts, before, PEN)
        after = eng.generated()
        emitted |= {len(after[b]) - len(before[b]) for b in range(4)}
        # the table after the NEXT catch-up is checked through the next cycle's rows; here: what is counted so far
        assert host(eng.counted_len).tolist()[:2] == [len(before[0]), len(before[1])]
    assert eng._mode_processing and len(emitted) >= 2, emitted             # catch-up saw different numbers of accepted tokens
    if use_graph:
        assert eng._graph_p is not None and eng._graph is None and eng._graph_s is None
    g3 = eng.generated()[3]
    assert not any(t in STOP16 for t in g3[:40]) and len(g3) >= 7           # min_tokens: no stop id so far


def test_engine_min_tokens_end_to_end_graph_equals_eager(tiny):
    prompts = _prompts(tiny)
    runs = []
    for use_graph in (False, True):
        eng = _engine(tiny, use_graph)
        eng.add_sequence(0, prompts[0])
        eng.step(); eng.step()
        plain = eng.generated()[0]
        stop = tuple(sorted(set(plain[:6])))
        eng.free_slot(0)
        eng.set_sampling_params(0, 0.0, min_tokens=6, stop_token_ids=stop)
        eng.add_sequence(0, prompts[0])
        eng.step(); eng.step()
        got = eng.generated()[0]
        assert len(got) >= 3 and not any(t in stop for t in got[:6]), (stop, got)
        assert plain[0] in stop and got[0] != plain[0]                      # the first token (prompt pass) is masked too
        runs.append((plain, got))
    assert runs[0] == runs[1]


def test_engine_recover_replays_the_processed_cycle(tiny):
    prompts = _prompts(tiny)
    engs = []
    for disturbed in (False, True):
        eng = _engine(tiny, True)
        for b in range(4):
            eng.set_sampling_params(b, **PEN[b])
        eng.add_sequences_to([0, 1, 2, 3], prompts)
        for i in range(4):
            eng.step()
            torch.cuda.synchronize()
            if disturbed and i in (1, 2):
                eng.recover()                                               # after a healthy cycle: same tokens, same table
        eng.step()
        engs.append(eng)
    a, b = engs
    assert a.generated() == b.generated() and b.recoveries == 2
    assert torch.equal(a.tok_table[:2], b.tok_table[:2]) and torch.equal(a.counted_len, b.counted_len)
    assert host(a.counted_len)[0] == len(a.generated()[0]) - int(host(a.gen_lens)[0] - host(a.counted_len)[0])


def test_engine_isolation_and_return_to_the_sampling_graph(tiny):
    prompts = _prompts(tiny)
    seeded = dict(temperature=0.8, top_k=50, top_p=0.9, seed=20261016)
    alone = _engine(tiny, True)
    alone.set_sampling_params(0, **seeded)
    alone.add_sequence(0, prompts[0])
    both = _engine(tiny, True, seed=7)
    both.set_sampling_params(2, **seeded)
    both.add_sequence(2, prompts[0])
    both.set_sampling_params(1, **PEN[1])
    both.add_sequence(1, prompts[1])
    for _ in range(3):
        alone.step(); both.step()
    assert alone._graph_s is not None and alone._graph_p is None and alone._lp_host is None
    assert both._graph_p is not None and both._graph_s is None and both._mode_processing
    assert alone.generated()[0] == both.generated()[2] and len(alone.generated()[0]) >= 4
    old_row = both.tok_table[1].clone()
    assert int(old_row.abs().max()) != 0
    both.free_slot(1)                                                       # back to the sampling graph
    alone.step(); both.step()
    assert not both._mode_processing and both._graph_s is not None
    assert alone.generated()[0] == both.generated()[2]
    # a new penalised request in the freed slot: its rows know nothing of the old table row (a SEEDED request: its tokens
    # depend on its own seed and positions alone, so an engine that never held the old request must emit the same)
    both.set_sampling_params(1, **PEN[1])
    both.add_sequence(1, prompts[3])
    fresh = _engine(tiny, False)
    fresh.set_sampling_params(1, **PEN[1])
    fresh.add_sequence(1, prompts[3])
    for _ in range(2):
        both.step(); fresh.step()
    assert both._mode_processing and both.generated()[1] == fresh.generated()[1]
    torch.cuda.synchronize()
    assert torch.equal(both.tok_table[1], fresh.tok_table[1])


def test_engine_preempted_request_gives_the_same_processed_row(tiny):
    prompts = _prompts(tiny)
    kw = PEN[0]
    a = _engine(tiny, False)
    a.set_sampling_params(0, **kw)
    a.add_sequence(0, prompts[1])
    for _ in range(3):
        a.step()
    outs = a.generated()[0]
    n = len(outs) - 1                                                       # re-admit with all but the last token as history
    b = _engine(tiny, False)
    b.set_sampling_params(2, **kw)
    b.add_sequence(2, prompts[1] + outs[:n], num_prompt_tokens=len(prompts[1]))
    assert int(b.lp_gen_base[2]) == n
    # the re-admitted request's first token is position n of the uninterrupted one: same history, same penalties.  Its
    # logits come from a prompt pass instead of a decode step, so compare the PROCESSING: the table row, and the row
    # processed from b's own raw logits against process_row with the prompt / outputs split
    ta = np.bincount(np.array(outs[:n]), minlength=2048)
    tb = host(b.tok_table[2]).view(np.uint32)
    assert np.array_equal(tb & 0x7FFFFFFF, ta.astype(np.uint32))
    assert set(np.nonzero(tb >> 31)[0].tolist()) == set(prompts[1])
    b.step()
    before = [[], [], outs[:n] + b.generated()[2][:1], []]
    raw = host(b.scratch_verify.logits[8:12]); proc = host(b.proc_logits_v[8:12]); d = host(b.draft_ids_kb)[:, 2].tolist()
    for j in range(4):
        want = lc.process_row(raw[j], prompts[1], before[2], d[:j], _params(kw))
        assert np.array_equal(_bits(proc[j]), _bits(want)), j
    with pytest.raises(ValueError):
        b.add_sequence(3, prompts[0], num_prompt_tokens=len(prompts[0]) + 1)


def test_engine_penalties_with_typical_acceptance(tiny):
    from qspec_amd.spec_decode.typical_acceptance_sampler import TypicalAcceptanceSampler
    prompts = _prompts(tiny)
    eng = _engine(tiny, True, sampler=TypicalAcceptanceSampler(0.09, 0.3))
    for b in range(4):
        eng.set_sampling_params(b, **PEN[b])
    eng.add_sequences_to([0, 1, 2, 3], prompts)
    for _ in range(3):
        before = eng.generated()
        eng.step()
        _check_cycle(eng, prompts, before, PEN)
    assert all(len(g) >= 4 for g in eng.generated())
