"""CPU restatement of guided decoding (numpy) and the case matrix of its tests.

What is restated: BaseLogitsProcessor.__call__ (vllm/model_executor/guided_decoding/outlines_logits_processors.py:34-93), the
processor the reference's engine lowers guided_decoding to (vllm/engine/llm_engine.py:1950-2009), in front of the steps
tests/constraint_cases.py restates.  That file imports `outlines` at module level, which is not installed, so NO golden fixture
can be produced from it: this file is pinned to a restatement, and tests/test_guides_cpu.py executes the reference's mask lines
(:80-92) literally with torch on CPU against it.

The state of a row is the guide's initial state advanced over the request's OUTPUTS followed by the in-flight draft tokens
d_1 .. d_j of the row, never the prompt (the reference's hash chain starts from defaultdict(int) at the empty output list).
The mask: fp32, 0 at the allowed ids below the vocabulary, -inf elsewhere, added to the fp16 row -- every element becomes
fp16(fp32(x) + 0.0) (-0.0 turns into +0.0) and the others -inf.  Where the reference ADDS -inf this file SETS -inf; the two
differ only for a masked token whose logit is +inf or NaN (NaN in the reference).
"""
from __future__ import annotations

from typing import Optional, Sequence

import numpy as np

import constraint_cases as cc
from logit_cases import F16, F32, Params

from qspec_amd.spec_decode.guides import TokenFSM

NEG_INF = F16(-np.inf)


def guide_row(raw_fp16, fsm: TokenFSM, state: int) -> np.ndarray:
    """One row [V] fp16 -> the row the guided processor leaves in `state`, fp16."""
    x = np.array(raw_fp16, dtype=F16, copy=True)
    deny = np.ones(x.shape[0], dtype=bool)
    deny[fsm.allowed(state)] = False
    with np.errstate(all="ignore"):
        x = (x.astype(F32) + F32(0.0)).astype(F16)
    x[deny] = NEG_INF
    return x


def process_row_guided(raw_fp16, prompt, outputs, in_flight, params: Params, c: cc.Constraints, fsm: Optional[TokenFSM],
                       state: Optional[int] = None) -> np.ndarray:
    """The guide, then the token constraints, then min_tokens / penalties, as the reference orders them.  state: the guide's state
    after `outputs` (default: walked from the initial state); the in-flight tokens are walked here."""
    if fsm is None:
        return cc.process_row_constrained(raw_fp16, prompt, outputs, in_flight, params, c)
    s = fsm.advance(fsm.initial, outputs) if state is None else int(state)
    s = fsm.advance(s, in_flight)
    return cc.process_row_constrained(guide_row(raw_fp16, fsm, s), prompt, outputs, in_flight, params, c)


# ---------------------------------------------------------------------- builders of the test automata
def random_fsm(V: int, n_states: int, seed: int, density: float = 0.4, always: Sequence[int] = (), never: Sequence[int] = (),
               eos: Optional[int] = None, never_in_state_1: Sequence[int] = ()) -> TokenFSM:
    """n_states states that each allow a random `density` of the vocabulary plus `always` minus `never` (state 1: also minus
    never_in_state_1), with pseudo-random next states, and the final state (only eos, back to itself) as the miss state.  Built
    as CSR directly (no dictionaries)."""
    rng = np.random.default_rng(seed)
    eos = V - 1 if eos is None else int(eos)
    row_ptr, toks, nxt = [0], [], []
    for s in range(n_states):
        mask = rng.random(V) < density
        mask[list(always)] = True
        mask[list(never)] = False
        if s == 1:
            mask[list(never_in_state_1)] = False
        mask[eos] = True
        t = np.nonzero(mask)[0]
        n = (t * 31 + 7 * s + 3) % n_states
        n[t == eos] = n_states
        toks.append(t); nxt.append(n); row_ptr.append(row_ptr[-1] + len(t))
    toks.append(np.array([eos])); nxt.append(np.array([n_states])); row_ptr.append(row_ptr[-1] + 1)
    return TokenFSM(row_ptr, np.concatenate(toks), np.concatenate(nxt), 0, n_states, V, eos)


def modular_fsm(V: int, m: int, eos: int) -> TokenFSM:
    """The m-cycle automaton: state i allows the ids = i mod m plus eos and leads to state (i + 1) mod m."""
    return TokenFSM.from_transitions({i: {**{t: (i + 1) % m for t in range(i, V, m)}, eos: -1} for i in range(m)}, 0, eos, V)


# ---------------------------------------------------------------------- the case matrix of the GPU pre-pass test
INFLIGHT_CAP = 64   # QS_LP_MAX_INFLIGHT


def make_guided_case(V: int, T: int, rows_per_seq: int, seed: int, j_base: Optional[int] = None):
    """constraint_cases.make_constrained_case plus guides: every other constrained slot (2, 4, ...; the only slot of a
    one-sequence case) is guided by one of two shared automata and starts in a random state; slots 0 and 1 stay plain /
    unconstrained, the odd ones constrained but unguided.  The automata allow every in-flight token of the case (the walks move
    through their states) except one in-flight token (the second where there is one) of the last active guided slot, which steps
    onto the miss state; they allow the chunk edges 2047 / 2048 and V - 1 in state 0 and forbid them in state 1.  j_base
    (rows_per_seq == 1 only): replaces the case's, with that many in-flight tokens -- up to the cap."""
    case = cc.make_constrained_case(V, T, rows_per_seq, seed)
    rng = np.random.default_rng(seed + 104729)
    nseq = len(case["slots"])
    if j_base is not None:
        assert rows_per_seq == 1
        case["j_base"], case["n_draft"] = j_base, j_base
        case["drafts"] = rng.integers(0, V, (j_base, nseq)).astype(np.int64)
    guided = [s for s in range(nseq) if (s >= 2 and s % 2 == 0) or nseq == 1]
    drafts = case["drafts"]
    seen = sorted(set(int(t) for t in drafts.reshape(-1)))
    never = []
    live = [s for s in guided if case["slots"][s]["active"]]
    if live and case["n_draft"]:
        miss_tok = int(drafts[min(1, case["n_draft"] - 1), live[-1]])
        seen = [t for t in seen if t != miss_tok]
        never = [miss_tok]
    edges = [t for t in (2047, 2048, V - 1) if 0 <= t < V and t not in never]
    eos = next(t for t in range(V - 2, 0, -1) if t not in never)
    off1 = [t for t in edges if t not in seen]
    fsms = [random_fsm(V, 5, seed + 1, 0.4, seen + edges, never, eos, off1), random_fsm(V, 3, seed + 2, 0.02, seen, never, eos, off1)]
    for s, sl in enumerate(case["slots"]):
        sl["guide"] = None
        if s in guided:
            f = fsms[(s // 2) % 2]
            sl["guide"], sl["gstate"] = f, int(rng.integers(0, f.num_states - 1))
    case["fsms"] = fsms
    return case


def expected_guided(case) -> np.ndarray:
    raw, rps = case["raw"], case["rows_per_seq"]
    out = np.empty_like(raw)
    for t in range(raw.shape[0]):
        s, j = t // rps, case["j_base"] + t % rps
        sl = case["slots"][s]
        if not sl["active"]:
            out[t] = raw[t]
            continue
        out[t] = process_row_guided(raw[t], sl["prompt"], sl["outputs"], [int(d) for d in case["drafts"][:j, s]], sl["params"],
                                    sl["constraints"], sl["guide"], sl.get("gstate"))
    return out


def row_states(case):
    """[(row, slot, state of the row)] of the guided rows of a case."""
    rps, got = case["rows_per_seq"], []
    for t in range(case["raw"].shape[0]):
        s, j = t // rps, case["j_base"] + t % rps
        sl = case["slots"][s]
        if sl["active"] and sl["guide"] is not None:
            got.append((t, s, sl["guide"].advance(sl["gstate"], [int(d) for d in case["drafts"][:j, s]])))
    return got
