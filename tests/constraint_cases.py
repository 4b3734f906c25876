"""CPU restatement of the token constraints (numpy) and the case matrix of their tests.

What is restated: the three logits processors the reference's engine lowers logit_bias, allowed_token_ids and bad_words to
(vllm/entrypoints/openai/logits_processors.py:10-50, vllm/logits_process.py:48-119), run on the fp16 row in front of
Sampler.forward (vllm/model_executor/layers/logits_processor.py:134-170), followed by the steps tests/logit_cases.py restates.
tests/golden/token_constraints.npz holds what the reference's own functions gave on CPU
(tests/golden/make_token_constraints.py); tests/test_token_constraints_cpu.py pins this file to it, the GPU tests pin the
kernels to this file.

The roundings, as the reference's functions produce them:
  * `logits[id] += bias` (fp16 tensor element, Python float): fp16(fp32(x) + fp32(bias));
  * the allowed mask is a masked_fill with -inf;
  * the bad-words processor computes `logits + word_bias + last_token_bias` with an fp32 word_bias and the row is written back
    into the fp16 logits: every element becomes fp16(fp32(x) + 0.0) -- -0.0 turns into +0.0 -- and banned ones -inf.
Where the reference ADDS -inf (bad words) this file SETS -inf; the two differ only for a banned token whose logit is +inf or
NaN (NaN in the reference), which the fixture does not contain.

Bad words are matched against the request's OUTPUTS followed by the in-flight draft tokens d_1 .. d_j of the row, never against
the prompt; a word longer than outputs + 1 is skipped.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from logit_cases import F16, F32, Params, process_row

NEG_INF = F16(-np.inf)


@dataclass
class Constraints:
    logit_bias: Dict[int, float] = field(default_factory=dict)
    allowed: Optional[Tuple[int, ...]] = None
    bad_words: Tuple[Tuple[int, ...], ...] = ()

    def empty(self) -> bool:
        return not self.logit_bias and self.allowed is None and not self.bad_words


def banned_last_tokens(past: Sequence[int], bad_words) -> List[int]:
    """The last tokens of the multi-token bad words whose prefix the sequence `past` ends with."""
    past = [int(t) for t in past]
    out = []
    for w in bad_words:
        L = len(w)
        if L < 2 or L > len(past) + 1:
            continue
        if past[len(past) - (L - 1):] == [int(t) for t in w[:-1]]:
            out.append(int(w[-1]))
    return out


def constrain_row(raw_fp16, outputs: Sequence[int], in_flight: Sequence[int], c: Constraints) -> np.ndarray:
    """One row [V] fp16 -> the row the three processors leave, fp16."""
    x = np.array(raw_fp16, dtype=F16, copy=True)
    V = x.shape[0]
    with np.errstate(all="ignore"):
        for t, b in c.logit_bias.items():
            x[int(t)] = (F32(x[int(t)]) + F32(b)).astype(F16)
        if c.allowed is not None:
            deny = np.ones(V, dtype=bool)
            deny[list(c.allowed)] = False
            x[deny] = NEG_INF
        if c.bad_words:
            x = (x.astype(F32) + F32(0.0)).astype(F16)
            for w in c.bad_words:
                if len(w) == 1:
                    x[int(w[0])] = NEG_INF
            for t in banned_last_tokens(list(outputs) + list(in_flight), c.bad_words):
                x[t] = NEG_INF
    return x


def process_row_constrained(raw_fp16, prompt, outputs, in_flight, params: Params, c: Constraints) -> np.ndarray:
    """Token constraints, then min_tokens / penalties (tests/logit_cases.py), as the reference orders them."""
    return process_row(constrain_row(raw_fp16, outputs, in_flight, c), prompt, outputs, in_flight, params)


# ---------------------------------------------------------------------- the case matrix of the GPU pre-pass test
FULL_VOCAB = 128256
PREPASS_SHAPES = [(1, 1), (4, 1), (4, 4), (16, 4), (16, 1), (192, 6), (192, 4)]   # (T, rows_per_seq)


def make_constrained_case(V: int, T: int, rows_per_seq: int, seed: int):
    """Random inputs of one constrained pre-pass call, on top of logit_cases.make_prepass_case's: per slot a random subset of
    {biases (up to 512, clustered so that one 2048-chunk holds many), an allowed set (tiny, half the vocabulary, or all but
    one), single- and multi-token bad words, half of them built to match the slot's own outputs + in-flight tokens, some
    through the pre-admission tail}.  Slot 0 is unconstrained and neutral, slot 1 (if any) unconstrained with penalties."""
    from logit_cases import make_prepass_case
    case = make_prepass_case(V, T, rows_per_seq, seed)
    rng = np.random.default_rng(seed + 7919)
    nseq = len(case["slots"])
    for s, sl in enumerate(case["slots"]):
        outs = sl["outputs"]
        n_pre = int(rng.integers(0, len(outs) + 1)) if rng.random() < 0.5 else 0   # outputs the request had before admission
        if rng.random() < 0.25:
            n_pre = len(outs)
        sl["n_pre"] = n_pre
        c = Constraints()
        if s >= 2 or nseq == 1:
            kinds = rng.random(3) < 0.7
            if nseq == 1:
                kinds[:] = True
            if kinds[0]:
                n = int(rng.choice([1, 5, 64, 512]))
                base = int(rng.integers(0, V))
                ids = set(int(t) for t in (base + rng.integers(0, 3000, n)) % V) | set(int(t) for t in rng.integers(0, V, n // 4 + 1))
                ids = sorted(ids)[:512]
                c.logit_bias = {t: float(rng.choice([-100.0, 100.0, 0.5, -3.25, 1e-3, 0.0, 7.0])) for t in ids}
            if kinds[1]:
                mode = int(rng.integers(0, 3))
                if mode == 0:
                    c.allowed = tuple(sorted(set(int(t) for t in rng.integers(0, V, int(rng.integers(1, 6))))))
                elif mode == 1:
                    c.allowed = tuple(int(t) for t in np.nonzero(rng.random(V) < 0.5)[0])
                else:
                    drop = int(rng.integers(0, V))
                    c.allowed = tuple(t for t in range(V) if t != drop)
            if kinds[2]:
                words = [(int(t),) for t in rng.integers(0, V, int(rng.integers(0, 40)))]
                for _ in range(int(rng.integers(1, 33))):
                    L = int(rng.integers(2, 9))
                    if rng.random() < 0.5:
                        # built to match some row of the slot: a prefix ending j tokens into the in-flight ones
                        j = int(rng.integers(0, case["n_draft"] + 1))
                        past = list(outs) + [int(d) for d in case["drafts"][:j, s]]
                        if len(past) >= L - 1:
                            words.append(tuple(past[len(past) - (L - 1):]) + (int(rng.integers(0, V)),))
                            continue
                    words.append(tuple(int(t) for t in rng.integers(0, V, L)))
                multi = list(dict.fromkeys(w for w in words if len(w) > 1))[:32]
                c.bad_words = tuple(dict.fromkeys([w for w in words if len(w) == 1] + multi))
        sl["constraints"] = c
    return case


def expected_constrained(case) -> np.ndarray:
    raw, rps = case["raw"], case["rows_per_seq"]
    out = np.empty_like(raw)
    for t in range(raw.shape[0]):
        s, j = t // rps, case["j_base"] + t % rps
        sl = case["slots"][s]
        if not sl["active"]:
            out[t] = raw[t]
            continue
        out[t] = process_row_constrained(raw[t], sl["prompt"], sl["outputs"], [int(d) for d in case["drafts"][:j, s]],
                                         sl["params"], sl["constraints"])
    return out
