"""CPU restatement of the logit processors (numpy / torch-CPU) and the case matrix of their tests.

What is restated: Sampler.forward's steps in front of and behind the temperature (vllm/model_executor/layers/sampler.py:258-278 of
the reference): the min_tokens stop mask, the repetition / frequency / presence penalties -- in the logits' own dtype, fp16, every
step rounded to fp16 -- and min_p.  tests/golden/logit_processors.npz holds what the reference's own functions gave on CPU
(tests/golden/make_logit_processors.py); tests/test_logit_processors_cpu.py pins this file to it, the GPU tests pin the kernels
to this file.

The position rule of a speculative cycle: the row with in-cycle index j of a sequence is processed as the non-speculative sampler
would process that position: prompt tokens, outputs = the committed ones + the in-flight d_1 .. d_j, generated length = committed
+ j.  `process_row` takes the committed outputs and the in-flight tokens apart only to say so.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Sequence, Tuple

import numpy as np

F16, F32 = np.float16, np.float32


@dataclass
class Params:
    repetition: float = 1.0
    frequency: float = 0.0
    presence: float = 0.0
    min_tokens: int = 0
    stop_ids: Tuple[int, ...] = field(default_factory=tuple)


NEUTRAL = Params()


def _h(x) -> np.ndarray:
    """fp32 -> fp16, round to nearest even (one rounding step of the reference's fp16 arithmetic)."""
    return np.asarray(x, dtype=F32).astype(F16)


def process_row(raw_fp16, prompt: Sequence[int], outputs: Sequence[int], in_flight: Sequence[int], params: Params) -> np.ndarray:
    """One row [V] fp16 -> the processed row [V] fp16.  Steps and roundings of the reference: stop ids to -inf while fewer than
    min_tokens tokens were generated; x / r (x > 0) or x * r (x <= 0, looked at AFTER the division) where the token occurs in the
    prompt or the outputs; x -= f * fp16(count); x -= p * (count > 0).  Each fp16 operation is the fp32 operation on the fp16
    operands rounded to fp16."""
    x = np.array(raw_fp16, dtype=F16, copy=True)
    V = x.shape[0]
    outs = [int(t) for t in list(outputs) + list(in_flight)]
    if len(outs) < params.min_tokens:
        for t in params.stop_ids:
            if 0 <= t < V:
                x[t] = F16(-np.inf)
    cnt = np.bincount(np.array([t for t in outs if 0 <= t < V], dtype=np.int64), minlength=V)[:V]
    in_prompt = np.zeros(V, dtype=bool)
    in_prompt[[int(t) for t in prompt if 0 <= int(t) < V]] = True
    seen = in_prompt | (cnt > 0)
    r = np.where(seen, F16(params.repetition), F16(1.0)).astype(F16)
    with np.errstate(all="ignore"):
        pos = x > 0
        x[pos] = _h(x[pos].astype(F32) / r[pos].astype(F32))
        neg = x <= 0
        x[neg] = _h(x[neg].astype(F32) * r[neg].astype(F32))
        fc = _h(F32(F16(params.frequency)) * cnt.astype(F32).astype(F16).astype(F32))
        x = _h(x.astype(F32) - fc.astype(F32))
        pc = _h(F32(F16(params.presence)) * (cnt > 0).astype(F32))
        x = _h(x.astype(F32) - pc.astype(F32))
    return x


def cycle_rows(raw_rows, prompt, committed, drafts, params: Params):
    """The k+1 verify rows of a cycle: row j sees d_1 .. d_j in flight."""
    return [process_row(raw_rows[j], prompt, committed, list(drafts[:j]), params) for j in range(len(raw_rows))]


def _softmax32(l: np.ndarray) -> np.ndarray:
    """fp32 softmax of one row (-inf = masked), the sums in fp64 and rounded once."""
    m = l.max()
    e = np.where(np.isfinite(l), np.exp((l - m).astype(np.float64)), 0.0)
    return (e / e.sum()).astype(F32)


def min_p_keep(l, temp: float, min_p: float) -> np.ndarray:
    """The tokens min_p keeps among those still alive in `l` (fp32 logits BEFORE the temperature, -inf = masked by an earlier
    stage): probability >= min_p x the largest probability, i.e. exp(l / temp - max) >= min_p whatever the denominator."""
    z = np.asarray(l, dtype=F32) / F32(temp)
    alive = np.isfinite(z)
    ratio = np.where(alive, np.exp((z - z[alive].max()).astype(np.float64)), 0.0)
    return alive & ~(ratio < float(F32(min_p)))


def sampler_probs(l_fp16, temp: float, top_k: int, top_p: float, min_p: float):
    """Sampler.forward behind the penalties for one row with DISTINCT logits at the boundaries: temperature, top-k (ties at the
    k-th value kept), top-p (ascending cumulative probability <= 1 - p masked, never the largest), min_p, softmax.  A
    temperature < 1e-5 is a greedy row: divisor 1, no masking.  Returns (probs fp32, kept mask)."""
    l = np.asarray(l_fp16, dtype=F16).astype(F32)
    V = l.shape[0]
    if temp < 1e-5:
        return _softmax32(l), np.isfinite(l)
    z = (l / F32(temp)).astype(F32)
    if 0 < top_k < V:
        kth = np.sort(z)[V - top_k]
        z = np.where(z < kth, F32(-np.inf), z)
    if top_p < 1.0:
        order = np.argsort(z, kind="stable")
        ps = _softmax32(z)[order].astype(np.float64)
        mask = np.cumsum(ps) <= 1.0 - float(F32(top_p))
        mask[-1] = False
        z = z.copy()
        z[order[mask]] = F32(-np.inf)
    if min_p > 0.0:
        keep = min_p_keep(z, 1.0, min_p)
        z = np.where(keep, z, F32(-np.inf))
    return _softmax32(z), np.isfinite(z)


# ---------------------------------------------------------------------- the case matrix of the GPU pre-pass test
FULL_VOCAB = 128256
PREPASS_SHAPES = [(T, rps) for T in (1, 4, 16, 192) for rps in (1, 4, 6)]
# (T, rows_per_seq); a T that is no multiple of rows_per_seq ends in a partial sequence


def make_prepass_case(V: int, T: int, rows_per_seq: int, seed: int):
    """Random inputs of one pre-pass call: raw logits [T, V] (zeros, -0.0 and -inf sprinkled in), per-slot prompts / committed
    outputs / penalties / min_tokens, in-flight tokens [rows_per_seq - 1 + j_base, nslots].  Slot 0 is neutral (bits must come
    back), the last slot of three or more sits the step out (copied through)."""
    rng = np.random.default_rng(seed)
    nseq = (T + rows_per_seq - 1) // rows_per_seq
    j_base = int(rng.integers(0, 3)) if rows_per_seq == 1 else 0
    n_draft = j_base + rows_per_seq - 1
    raw = (rng.standard_normal((T, V)) * 4).astype(F16)
    raw[:, rng.integers(0, V, 64)] = F16(0.0)
    raw[:, rng.integers(0, V, 64)] = F16(-0.0)
    raw[:, rng.integers(0, V, 8)] = F16(-np.inf)
    hot = rng.integers(0, V, 40)                  # a small pool: repeats, prompt / output overlaps
    slots = []
    for s in range(nseq):
        prompt = list(rng.choice(hot, int(rng.integers(1, 30)))) + list(rng.integers(0, V, int(rng.integers(0, 50))))
        outs = list(rng.choice(hot, int(rng.integers(0, 400)))) + list(rng.integers(0, V, int(rng.integers(0, 20))))
        p = Params(repetition=float(rng.choice([1.0, 1.2, 0.8, 2.5, 1.05])), frequency=float(rng.choice([0.0, 0.1, -0.3, 1.5])),
                   presence=float(rng.choice([0.0, 0.5, -0.25, 2.0])), min_tokens=int(rng.choice([0, 0, len(outs) + 1, len(outs) + 3])),
                   stop_ids=tuple(int(t) for t in rng.integers(0, V, int(rng.integers(1, 17)))))
        if s == 0:
            p = Params()
        slots.append(dict(prompt=[int(t) for t in prompt], outputs=[int(t) for t in outs], params=p, active=True))
    if nseq >= 3:
        slots[-1]["active"] = False
    drafts = rng.choice(hot, (max(n_draft, 1), nseq)).astype(np.int64)[:n_draft] if n_draft else np.zeros((0, nseq), np.int64)
    return dict(raw=raw, slots=slots, drafts=drafts, j_base=j_base, rows_per_seq=rows_per_seq, n_draft=n_draft)


def expected_prepass(case) -> np.ndarray:
    raw, rps = case["raw"], case["rows_per_seq"]
    out = np.empty_like(raw)
    for t in range(raw.shape[0]):
        s, j = t // rps, case["j_base"] + t % rps
        sl = case["slots"][s]
        if not sl["active"]:
            out[t] = raw[t]
            continue
        out[t] = process_row(raw[t], sl["prompt"], sl["outputs"], [int(d) for d in case["drafts"][:j, s]], sl["params"])
    return out
