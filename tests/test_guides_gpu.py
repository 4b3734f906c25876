"""Guided decoding on the GPU: the guide build kernel against the numpy model of the layout, the guided pre-pass against
tests/guide_cases.py, the catch-up, the engine's guided cycle, and requests through the worker.

Condition on the engine's inputs: every row these tests put through the sampler keeps a finite logit, so no case relies on the
all -inf rule except the one test written for it.  Every guide but the choice trie leaves at least 64 finite logits in every
state a row is in (checked on the CPU model below, row by row); a trie cannot -- a node of a trie allows as many tokens as
the choices that pass through it, and 64 children at every node down to the 22 tokens a request emits here would be 64^22
nodes -- so for the trie slot the check is `at least one`."""
import os
import sys
from collections import defaultdict

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import constraint_cases as cc  # noqa: E402
import guide_cases as gc  # noqa: E402
import logit_cases as lc  # noqa: E402
from test_token_constraints_gpu import (_constrained, _engine, _pc, _plain_outputs, _prompts, _run, _slot_state, _worker,  # noqa: E402,F401
                                        ops, tiny)

from qspec_amd.spec_decode.guides import TokenFSM, guide_words  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EOS = 2047            # of the tiny model's vocabulary of 2048


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.detach().cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


# ---------------------------------------------------------------------- the build kernel
def _build_states(V, rng):
    """[(allowed tokens)] of the states the build test needs, then CSR with random next states."""
    rows = [[0], [31], [32], [V - 1], list(range(V)), [t for t in range(V) if (t >> 5) % 2 == 1],
            sorted(set(rng.integers(0, V, 50000).tolist()))]
    row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    tokens = np.concatenate([np.array(r) for r in rows])
    return TokenFSM(row_ptr, tokens, rng.integers(0, len(rows), len(tokens)), 0, 0, V)


@pytest.mark.parametrize("V", [128256, 1003])
def test_build_kernel_equals_the_numpy_layout_bit_for_bit(ops, V):
    f = _build_states(V, np.random.default_rng(V))
    S, N, words = f.num_states, f.num_transitions, guide_words(V)
    sb, tb, stride, guard = 3, 17, words + 8, 4           # nonzero bases; 4 guard words on either side of every row
    tg = ops.TokenGuides(1, V, DEV, max_states=sb + S + 2, max_transitions=tb + N + 9)
    body = tg.max_states * stride
    buf_a = torch.full((body + 2 * guard,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
    buf_r = buf_a.clone()
    tg.allow, tg.rank = buf_a[guard:], buf_r[guard:]
    tg.off.fill_(-7); tg.nxt.fill_(-7)
    ops.guide_build(tg, sb, tb, f.row_ptr, f.tokens, f.next_states, row_stride=stride)
    allow, rank, off, nxt = f.tables(words)
    got_a, got_r = host(buf_a).view(np.uint32), host(buf_r).view(np.uint32)
    # guard words: everything outside the S x words block is what it was -- in front of the first row, between the rows, behind
    for got, want in ((got_a, allow), (got_r, rank.view(np.uint32))):
        rows = got[guard:guard + body].reshape(tg.max_states, stride).copy()
        assert np.array_equal(rows[sb:sb + S, :words], want)
        rows[sb:sb + S, :words] = 0x5A5A5A5A
        assert (rows == 0x5A5A5A5A).all() and (got[:guard] == 0x5A5A5A5A).all() and (got[guard + body:] == 0x5A5A5A5A).all()
    assert np.array_equal(host(tg.off)[sb:sb + S], off + tb) and np.array_equal(host(tg.nxt)[tb:tb + N], nxt + sb)
    for t, lo, hi in ((host(tg.off), sb, sb + S), (host(tg.nxt), tb, tb + N)):
        assert (t[:lo] == -7).all() and (t[hi:] == -7).all()
    assert int(rank[4, -1]) + bin(int(allow[4, -1])).count("1") == V                 # every token allowed: the last rank counts them
    with pytest.raises(ValueError):
        ops.guide_build(tg, tg.max_states - 2, 0, f.row_ptr, f.tokens, f.next_states, row_stride=stride)
    with pytest.raises(ValueError):
        ops.guide_build(tg, 0, tg.max_transitions - 5, f.row_ptr, f.tokens, f.next_states, row_stride=stride)


# ---------------------------------------------------------------------- the guided pre-pass
def _guided(ops, raw, out, plain, cons, tg, **kw):
    names = ("deny", "meta", "bias_ids", "bias_vals", "words", "word_lens", "tail", "gen_tokens")
    gnames = ("guide_allow", "guide_rank", "guide_off", "guide_next", "guide_slots")
    return ops.process_logits_guided(raw, out, **plain, **dict(zip(names, cons)), **dict(zip(gnames, tg.arrays())), **kw)


def _guide_state(ops, V, case):
    """The arena with the case's automata (at nonzero bases, behind stale rows) and the slots' guide state."""
    n = len(case["slots"])
    fsms = case["fsms"]
    tg = ops.TokenGuides(n, V, DEV, max_states=3 + sum(f.num_states for f in fsms), max_transitions=11 + sum(f.num_transitions for f in fsms))
    tg.allow.fill_(-1); tg.rank.fill_(12345); tg.off.fill_(3); tg.nxt.fill_(1)
    tg.gslot.copy_(torch.tensor([[2, 0, 1, 0]] * n, dtype=torch.int32))               # stale rows, flag off: must not be read
    sb, tb, base = 3, 11, {}
    for f in fsms:
        ops.guide_build(tg, sb, tb, f.row_ptr, f.tokens, f.next_states)
        base[id(f)] = sb
        sb, tb = sb + f.num_states, tb + f.num_transitions
    for s, sl in enumerate(case["slots"]):
        if sl["guide"] is not None:
            b = base[id(sl["guide"])]
            tg.set_slot(s, b + sl["gstate"], b + sl["guide"].miss, guided=True, g_len=5)
    return tg


def _check_guided_case(ops, V, case, slot_ids=None):
    T, rps = case["raw"].shape[0], case["rows_per_seq"]
    plain, cons = _slot_state(ops, V, case["slots"])
    tg = _guide_state(ops, V, case)
    raw = dev(case["raw"])
    buf = torch.full((T + 2, V), float("nan"), dtype=torch.float16, device=DEV)      # a guard row on either side
    kw = dict(draft_ids=dev(case["drafts"]) if case["n_draft"] else None, rows_per_seq=rps, j_base=case["j_base"])
    if slot_ids is not None:
        kw["slot_ids"] = dev(np.array(slot_ids, np.int32))
    gslot_before = host(tg.gslot).copy()
    _guided(ops, raw, buf[1:T + 1], plain, cons, tg, **kw)
    got = host(buf)
    assert np.isnan(got[0]).all() and np.isnan(got[T + 1]).all()
    want = gc.expected_guided(case)
    for t in range(T):
        assert np.array_equal(_bits(got[t + 1]), _bits(want[t])), (t, int((_bits(got[t + 1]) != _bits(want[t])).sum()))
    assert np.array_equal(_bits(host(raw)), _bits(case["raw"])) and np.array_equal(host(tg.gslot), gslot_before)   # nothing written but out
    # unguided rows: the bits of the constrained entry; plain rows: those of the plain entry
    ref_c = torch.full((T, V), float("nan"), dtype=torch.float16, device=DEV)
    ref_p = torch.full((T, V), float("nan"), dtype=torch.float16, device=DEV)
    _constrained(ops, raw, ref_c, plain, cons, **kw)
    ops.process_logits(raw, ref_p, **plain, **kw)
    ref_c, ref_p = host(ref_c), host(ref_p)
    seq_of = (lambda t: t // rps) if slot_ids is None else (lambda t: slot_ids[t // rps])
    unguided = [t for t in range(T) if case["slots"][seq_of(t)]["guide"] is None]
    free = [t for t in unguided if case["slots"][seq_of(t)]["constraints"].empty()]
    for t in unguided:
        assert np.array_equal(_bits(got[t + 1]), _bits(ref_c[t])), t
    for t in free:
        assert np.array_equal(_bits(got[t + 1]), _bits(ref_p[t])), t
    return want, unguided, free


@pytest.mark.parametrize("T,rows_per_seq", cc.PREPASS_SHAPES)
def test_guided_prepass_full_vocabulary_bit_exact(ops, T, rows_per_seq):
    V = cc.FULL_VOCAB
    case = gc.make_guided_case(V, T, rows_per_seq, seed=3000 * T + rows_per_seq)
    want, unguided, free = _check_guided_case(ops, V, case)
    states = gc.row_states(case)
    assert states and (len(case["slots"]) == 1 or (unguided and free))
    n_guided = len(set(s for _, s, _ in states))
    if n_guided >= 6:
        kinds = [0, 0, 0]
        for sl in case["slots"]:
            if sl["guide"] is not None:
                c = sl["constraints"]
                kinds = [kinds[0] + bool(c.logit_bias), kinds[1] + (c.allowed is not None), kinds[2] + bool(c.bad_words)]
        assert all(kinds), kinds                                                  # guided slots that also carry each kind of constraint
    if case["n_draft"] >= 1:                                                     # one walk steps onto the miss state
        assert any(sl["guide"] is not None and st == sl["guide"].miss for _, s, st in states for sl in [case["slots"][s]])
    if n_guided >= 6 and case["n_draft"]:
        assert len(set(st for _, _, st in states)) >= 3                           # the walks move through the states


def test_guided_prepass_walks_up_to_the_inflight_cap_and_onto_a_miss(ops):
    V = cc.FULL_VOCAB
    case = gc.make_guided_case(V, 6, 1, seed=77, j_base=gc.INFLIGHT_CAP)
    assert case["drafts"].shape == (64, 6)
    _check_guided_case(ops, V, case)
    states = dict((s, st) for _, s, st in gc.row_states(case))
    f2, f4 = case["slots"][2]["guide"], case["slots"][4]["guide"]
    assert states[4] == f4.miss and states[2] != f2.miss                            # slot 4 missed at its second token; slot 2 walked 64
    # the edges of the chunks and of the vocabulary, explicitly: states 0 (allowed) and 1 (forbidden) of the first automaton
    edge = gc.make_guided_case(V, 6, 1, seed=78, j_base=0)
    for s, st in ((2, 0), (4, 1)):
        edge["slots"][s]["guide"], edge["slots"][s]["gstate"] = edge["fsms"][0], st
        edge["slots"][s]["constraints"] = cc.Constraints()
        edge["slots"][s]["params"] = lc.Params()
    edge["raw"][:, [2047, 2048, V - 1]] = np.float16(1.5)
    # the guide's zero comes in FRONT of the bias: -2^-24 + 5.9e-8 rounds to -0.0 in fp16 and stays -0.0 (no zero behind it)
    edge["raw"][2, 2047] = np.float16(-5.96e-8)
    edge["slots"][2]["constraints"] = cc.Constraints({2047: 5.9e-8})
    want, _, _ = _check_guided_case(ops, V, edge)
    assert np.isfinite(want[2][[2047, 2048, V - 1]]).all() and np.isneginf(want[4][[2047, 2048, V - 1]]).all()
    assert int(_bits(want[2])[2047]) == 0x8000


def test_guided_prepass_odd_vocabulary_and_slot_ids(ops):
    """A vocabulary that is no multiple of 8 (scalar path, last allow word partial) with the rows mapped to slots through slot_ids."""
    V = 1003
    case = gc.make_guided_case(V, 6, 1, seed=9, j_base=2)
    for sl in case["slots"]:
        sl["active"] = True
    order = [4, 2, 5, 0, 1, 3]
    shuffled = dict(case, slots=[case["slots"][s] for s in order], drafts=case["drafts"][:, order])
    want = gc.expected_guided(shuffled)
    T = 6
    plain, cons = _slot_state(ops, V, case["slots"])
    tg = _guide_state(ops, V, case)
    raw = dev(case["raw"])
    out = torch.full_like(raw, float("nan"))
    _guided(ops, raw, out, plain, cons, tg, draft_ids=dev(case["drafts"]), j_base=2, slot_ids=dev(np.array(order, np.int32)))
    for t in range(T):
        assert np.array_equal(_bits(host(out)[t]), _bits(want[t])), (t, order[t])
    assert np.isneginf(want[0]).sum() > 500 and np.isneginf(want[3]).sum() < 50       # a guided row and a plain one


def test_row_a_guide_leaves_without_a_finite_logit_samples_token_zero_and_misses(ops):
    """THE test of the all -inf rule: a guided state disjoint from allowed_token_ids.  The row is -inf everywhere, the front end
    emits token 0 with NaN probabilities, nothing faults -- and token 0, not allowed in the state, leads to the miss state."""
    V = 4096
    f = TokenFSM.from_transitions({0: {t: 0 for t in range(100, 200)}}, 0, 7, V)
    c = cc.Constraints({}, tuple(range(300, 400)), ())
    sl = dict(prompt=[1], outputs=[], n_pre=0, params=lc.Params(), constraints=c, active=True, guide=f, gstate=0)
    plain, cons = _slot_state(ops, V, [sl])
    tg = _guide_state(ops, V, dict(slots=[sl], fsms=[f]))
    raw = dev((np.random.default_rng(0).standard_normal((1, V)) * 3).astype(np.float16))
    out = torch.full_like(raw, float("nan"))
    _guided(ops, raw, out, plain, cons, tg)
    assert np.isneginf(host(out)).all()
    probs = torch.zeros(1, V, dtype=torch.float32, device=DEV)
    tok = torch.full((1,), -7, dtype=torch.int64, device=DEV)
    ops.sample_top_k_top_p(out, probs, tok, dev(np.array([1.0], np.float32)), None, None)
    assert int(tok[0]) == 0
    gen = torch.full((1, 8), -1, dtype=torch.int64, device=DEV)
    gen[0, 0] = tok[0]
    tg.gslot[0, 1] = 0
    ops.guide_catch_up(*tg.arrays(), V, gen, dev(np.array([1], np.int32)))
    assert host(tg.gslot)[0].tolist() == [3 + f.miss, 1, 3 + f.miss, 1]


# ---------------------------------------------------------------------- catch-up
def test_catch_up_walks_the_new_tokens_once(ops):
    V, k = 1003, 3
    f = gc.random_fsm(V, 6, seed=4, density=0.6)
    tg = ops.TokenGuides(5, V, DEV, max_states=16, max_transitions=f.num_transitions + 5)
    sb = 2
    ops.guide_build(tg, sb, 5, f.row_ptr, f.tokens, f.next_states)
    rng = np.random.default_rng(8)
    gen = np.full((5, 16), -1, np.int64)
    walks = []
    for b in range(5):       # tokens the automaton allows, so the walk moves; slot 2's last token is a miss
        s, row = 1, []
        for _ in range(10):
            t = int(rng.choice(f.allowed(s)[:-1])) if len(f.allowed(s)) > 1 else int(f.allowed(s)[0])
            row.append(t); s = f.next(s, t)
        walks.append(row)
    walks[2][7] = int(np.setdiff1d(np.arange(V), f.allowed(f.advance(1, walks[2][:7])))[0])
    for b in range(5):
        gen[b, :10] = walks[b]
    g_len = [4, 4, 4, 4, 4]
    gen_lens = [4, 5, 4 + k + 1, 7, 9]                                               # walk 0, 1 and k + 1 tokens; slots 3, 4 below
    start = [f.advance(1, walks[b][:4]) for b in range(5)]
    rows = [[sb + start[b], g_len[b], sb + f.miss, 1] for b in range(5)]
    rows[3][3] = 0                                                                   # an unguided (inactive) slot: untouched
    rows[4][1] = 12                                                                  # g_len beyond gen_lens (a freed slot): untouched
    tg.gslot.copy_(torch.tensor(rows, dtype=torch.int32))
    args = (*tg.arrays(), V, dev(gen), dev(np.array(gen_lens, np.int32)))
    ops.guide_catch_up(*args)
    once = host(tg.gslot).copy()
    want = [list(r) for r in rows]
    for b in (0, 1, 2):
        want[b][0], want[b][1] = sb + f.advance(start[b], walks[b][4:gen_lens[b]]), gen_lens[b]
    assert once.tolist() == want and want[2][0] == sb + f.miss
    ops.guide_catch_up(*args)
    assert np.array_equal(host(tg.gslot), once)                                      # twice equals once


# ---------------------------------------------------------------------- engine
def _guides(plain):
    """The guides of the four slots: the 3-cycle automaton; a choice trie cut from the request's own unconstrained output where
    it would diverge; a 2-cycle automaton beside allowed_token_ids, min_p and a seed; none."""
    g1 = plain[1]
    rng = np.random.default_rng(17)
    fill = lambda: rng.integers(100, 2000, 30).tolist()   # noqa: E731  (choices longer than any output of these tests)
    other = lambda t: 100 + (t + 1) % 1900                # noqa: E731
    trie = TokenFSM.from_token_sequences([g1[:3] + [other(g1[3])] + fill(), g1[:1] + [other(g1[1])] + fill(), [other(g1[0])] + fill(),
                                          g1[:2] + [other(g1[2])] + fill()], EOS, 2048)
    return [gc.modular_fsm(2048, 3, EOS), trie, gc.modular_fsm(2048, 2, EOS), None]


def _kws(plain):
    g = _guides(plain)
    return [dict(temperature=0.0, guide=g[0]), dict(temperature=0.0, guide=g[1], repetition_penalty=1.1),
            dict(temperature=0.9, seed=77, min_p=0.02, allowed_token_ids=list(range(0, 1500)), guide=g[2]),
            dict(temperature=0.8, seed=5)]


class _Tap:
    """Records every pre-pass call of an eager engine: (raw, processed, rows_per_seq, j_base, in-flight ids, guided)."""

    def __init__(self, eng):
        self.calls, inner = [], eng._process

        def process(logits, out, rows_per_seq, j_base, draft_ids, active_lens, slot_ids=None, constrained=None, guided=None):
            res = inner(logits, out, rows_per_seq, j_base, draft_ids, active_lens, slot_ids=slot_ids, constrained=constrained,
                        guided=guided)
            torch.cuda.synchronize()
            self.calls.append((host(logits).copy(), host(res).copy(), rows_per_seq, j_base,
                               None if draft_ids is None else host(draft_ids).copy(), guided))
            return res
        eng._process = process


def _want_row(raw, prompt, outputs, in_flight, kw):
    p, c = _pc(kw)
    return gc.process_row_guided(raw, prompt, outputs, in_flight, p, c, kw.get("guide"))


def _enough_candidates(want, kw):
    n = int(np.isfinite(want).sum())
    return n >= (1 if kw.get("guide") is not None and kw["guide"].num_states > 8 else 64)    # (the trie: see the module docstring)


def test_engine_every_draft_and_verify_row_equals_the_restatement(tiny):
    prompts = _prompts()
    kws = _kws(_plain_outputs(tiny, prompts))
    eng = _engine(tiny, False)
    for b in range(4):
        eng.set_sampling_params(b, **kws[b])
    tap = _Tap(eng)
    eng.add_sequences_to([0, 1, 2, 3], prompts)
    assert len(tap.calls) == 1 and tap.calls[0][5] is True                       # the first token: j = 0, nothing in flight
    raw, proc = tap.calls.pop()[:2]
    for b in range(4):
        want = _want_row(raw[b], prompts[b], [], [], kws[b])
        assert np.array_equal(_bits(proc[b]), _bits(want)) and _enough_candidates(want, kws[b]), b
    k, rows = eng.k, 0
    for cyc in range(5):
        before = eng.generated()
        eng.step()
        assert len(tap.calls) == k + 1
        for raw, proc, rps, j_base, drafts, guided in tap.calls:
            assert guided is True
            for t in range(raw.shape[0]):
                b, j = t // rps, j_base + t % rps
                want = _want_row(raw[t], prompts[b], before[b], [int(d) for d in drafts[:j, b]], kws[b])
                assert np.array_equal(_bits(proc[t]), _bits(want)), (cyc, rps, b, j)
                assert _enough_candidates(want, kws[b]), (cyc, rps, b, j)
                rows += 1
        tap.calls.clear()
    assert rows == 5 * (3 * 4 + 16) and eng._mode_guided and eng._mode_constrained and eng._mode_processing
    g = eng.generated()
    assert all(len(x) >= 6 for x in g)
    eng.step_no_spec()                                                           # the non-speculative step: j = 0, after its catch-up
    raw, proc = tap.calls.pop()[:2]
    for b in range(4):
        want = _want_row(raw[b], prompts[b], g[b], [], kws[b])
        assert np.array_equal(_bits(proc[b]), _bits(want)) and _enough_candidates(want, kws[b]), b
    for b in range(3):
        assert kws[b]["guide"].accepts(eng.generated()[b]), b


def test_engine_graph_equals_eager_recover_replays_and_guides_hold(tiny):
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
            assert eng._graph_g is not None and list(eng._graphs) == [(4, "full")]   # _graph_g is the only graph captured
            g = eng._graph_g
            eng.free_slot(2)                                                     # a new guide in a freed slot: same graph object
            five = gc.modular_fsm(2048, 5, EOS)
            eng.set_sampling_params(2, 0.0, guide=five)
            eng.add_sequence(2, prompts[2])
            eng.step(); eng.step()
            g2 = eng.generated()[2]
            assert eng._graph_g is g and list(eng._graphs) == [(4, "full")] and len(g2) >= 3 and five.accepts(g2), g2
            assert [t % 5 for t in g2[:3]] == [0, 1, 2]
    assert runs[0] == runs[1] == runs[2]
    for b in range(3):
        assert kws[b]["guide"].accepts(runs[0][b]), (b, runs[0][b])
        assert not kws[b]["guide"].accepts(plain[b]), b                          # the unconstrained output of the same prompt is rejected
    assert [t % 3 for t in runs[0][0][:6]] == [0, 1, 2, 0, 1, 2] and all(t < 1500 for t in runs[0][2])
    assert all(len(r) >= 6 for r in runs[0])


def test_engine_isolation_slot_reuse_and_return_to_the_parent_graphs(tiny):
    prompts = _prompts()
    seeded = dict(temperature=0.8, top_k=50, top_p=0.9, seed=20261019, guide=gc.modular_fsm(2048, 2, EOS))
    alone = _engine(tiny, True)
    alone.set_sampling_params(0, **seeded)
    alone.add_sequence(0, prompts[0])
    both = _engine(tiny, True, seed=7)
    both.set_sampling_params(3, temperature=0.7, seed=4)                             # sampled companions first: level 1 and its graph
    both.add_sequence(3, prompts[3])
    both.step()
    parent = both._graph_s
    assert parent is not None and both.tg is None and both.guide_arena is None       # no guided request yet: nothing allocated
    both.set_sampling_params(2, **seeded)
    both.add_sequence(2, prompts[0])
    both.set_sampling_params(1, 0.0, guide=gc.modular_fsm(2048, 3, EOS), logit_bias={5: 1.0})
    both.add_sequence(1, prompts[1])
    for _ in range(3):
        alone.step(); both.step()
    assert both._graph_g is not None and both._mode_guided and both._graph_s is parent and both._graph_c is None and both._graph_p is None
    # a seeded guided request yields the same tokens in another slot with other companions
    a, b = alone.generated()[0], both.generated()[2]
    assert a == b and len(a) >= 4 and seeded["guide"].accepts(a)
    assert both.guide_arena.resident(seeded["guide"]).refs == 1 and alone.guide_arena.resident(seeded["guide"]).refs == 1
    both.free_slot(1); both.free_slot(2)                                             # the guided requests leave
    both.step()
    assert not both._mode_guided and not both._mode_constrained and both._graph_s is parent and both._level == 1
    assert both.guide_arena.resident(seeded["guide"]).refs == 0 and host(both.tg.gslot)[1:3].tolist() == [[0] * 4] * 2
    # the greedy headline: an engine that saw a guided request come and go replays the greedy graph object it had
    eng = _engine(tiny, True)
    eng.add_sequence(0, prompts[0])
    eng.step()
    g0 = eng._graph
    eng.set_sampling_params(1, 0.0, guide=seeded["guide"])
    eng.add_sequence(1, prompts[1])
    eng.step()
    eng.free_slot(1)
    eng.step()
    assert g0 is not None and eng._graph is g0 and eng._level == 0 and sorted(eng._graphs) == [(0, "full"), (4, "full")]


def test_engine_fork_keeps_both_samples_inside_the_guide(tiny):
    prompts = _prompts()
    f = gc.modular_fsm(2048, 3, EOS)
    eng = _engine(tiny, True)
    eng.set_sampling_params(0, temperature=0.9, seed=11, guide=f)
    eng.add_sequence(0, prompts[0], sample_slots=[1])                                # n = 2: two samples of one prompt
    for _ in range(3):
        eng.step()
    g = eng.generated()
    assert f.accepts(g[0]) and f.accepts(g[1]) and g[0] != g[1] and eng.guide_arena.resident(f).refs == 2
    eng.fork_slot(0, 2)                                                              # a fork mid-generation: state and g_len travel
    assert host(eng.tg.gslot)[2].tolist() == host(eng.tg.gslot)[0].tolist() and eng.guide_arena.resident(f).refs == 3
    for _ in range(2):
        eng.step()
    g = eng.generated()
    assert all(f.accepts(g[b]) and len(g[b]) >= 6 for b in range(3))


# ---------------------------------------------------------------------- worker: requests through execute_model
class RegexLogitsProcessor:   # the shape of the reference's lowered processor, by name and attributes; the worker never calls it
    def __init__(self, guide):
        self._guide, self._fsm_state = guide, defaultdict(int)

    def __call__(self, input_ids, scores):
        raise AssertionError("the worker lowers processors, it does not run them")


class _RegexGuide:
    def __init__(self, maps, eos):
        self.states_to_token_maps, self.initial_state, self.eos_token_id = maps, 0, eos


def test_execute_model_guided_tokens_across_cycles_and_a_preemption(tiny):
    from qspec_amd.spec_decode.worker import SamplingParams
    prompts = _prompts()
    guide = _RegexGuide({i: {**{t: (i + 1) % 3 for t in range(i, 2048, 3)}, EOS: i} for i in range(3)}, EOS)
    fsm = TokenFSM.from_guide(guide, 2048)
    for temperature in (0.0, 0.7):
        sp = dict(temperature=temperature, seed=11) if temperature else {}
        base = _run(_worker(tiny), [("a", prompts[0], SamplingParams(**sp))], 5)["a"]
        assert not fsm.accepts(base)                                                 # what a worker that ignores the processor emits
        guided = lambda: SamplingParams(logits_processors=[RegexLogitsProcessor(guide)], **sp)   # noqa: E731
        got = _run(_worker(tiny), [("a", prompts[0], guided()), ("b", prompts[1], SamplingParams())], 5)
        assert len(got["a"]) >= 6 and fsm.accepts(got["a"]), got["a"]
        assert [t % 3 for t in got["a"] if t != EOS][:6] == [0, 1, 2, 0, 1, 2]
        # re-admitted before cycle 2 with its outputs: the state is rebuilt from them on the host
        pre = _run(_worker(tiny), [("a", prompts[0], guided())], 5, preempt=("a", 2))["a"]
        assert len(pre) >= 6 and fsm.accepts(pre), pre
