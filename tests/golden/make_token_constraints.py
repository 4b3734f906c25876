"""Writes tests/golden/token_constraints.npz: inputs and outputs of the reference's OWN token-constraint processors run on CPU.

  * vllm/entrypoints/openai/logits_processors.py   logit_bias_logits_processor (:43-50) and AllowedTokenIdsLogitsProcessor
    (:10-27);
  * vllm/logits_process.py                         NoBadWordsLogitsProcessor (:48-119) -- the module imports the tokenizer
    package, so the class definition is compiled FROM THE REFERENCE FILE, the way make_golden.py's _ref_function takes functions.
They are applied to one fp16 row the way _apply_logits_processors does (vllm/model_executor/layers/logits_processor.py:134-170):
`row = logits[i]`, every processor in the engine's order (bias, allowed, bad words; llm_engine.py:1950-2009) with the sequence's
OUTPUT tokens, `logits[i] = row`.  Behind them the min_tokens mask and the reference's apply_penalties exactly as
make_logit_processors.py runs them, which pins the ORDER: constraints first.

Under speculation the row with in-cycle index j is processed as the non-speculative path would process that position: the
processors get outputs + the in-flight d_1 .. d_j.

Only recorded inputs and outputs are written.  Needs the reference checkout (present only in the build container).
Run: python tests/golden/make_token_constraints.py
"""
import ast
import functools
import os
import sys
from typing import Dict, Iterable, List, Optional, Tuple, Union

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF  # noqa: E402
from make_logit_processors import _load_utils  # noqa: E402

V = 320
F16 = torch.float16
INF = float("inf")


def _ref_def(path, name):
    """A top-level class or function of a reference module that cannot be imported as a whole (both modules pull in the
    tokenizer package), compiled from the reference file and executed here.  Nothing is copied; the reference's own code runs."""
    tree = ast.parse(open(path).read(), filename=path)
    ns = {"torch": torch, "List": List, "Tuple": Tuple, "Union": Union, "Dict": Dict, "Optional": Optional, "Iterable": Iterable}
    for node in tree.body:
        if isinstance(node, (ast.ClassDef, ast.FunctionDef)) and node.name == name:
            exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), ns)
    return ns[name]


def cases():
    """(name, prompt, outputs, in flight, bias, allowed, bad words, rep, freq, pres, min_tokens, stop ids, share)
    share: the name of an earlier case whose AllowedTokenIdsLogitsProcessor OBJECT this case reuses (it has only `mask` then)."""
    N = (1.0, 0.0, 0.0)
    every = tuple(range(V))
    w8 = tuple(range(80, 88))
    rows = [
        # bias on +0.0 / -0.0 / -inf, by zeros of both signs and by ordinary values
        ("bias_zero_inf_a", [1], [2], [], {10: -0.0, 11: -0.0, 12: 5.0, 18: 0.0, 19: 0.0}, None, (), *N, 0, ()),
        ("bias_zero_inf_b", [1], [2], [], {10: 0.25, 11: -0.25, 12: -100.0, 18: 1e-8, 19: -1e-8}, None, (), *N, 0, ()),
        # bias, then a penalty on the same token: the repetition rule looks at the sign the bias left
        ("bias_then_penalty", [16, 17, 3], [16, 4, 4], [], {16: -3.0, 17: 2.5, 4: -9.0, 3: 0.0}, None, (), 1.5, 0.1, 0.5, 0, ()),
        ("bias_then_penalty_inflight", [16, 17, 3], [16, 4], [4, 17], {16: -3.0, 17: 2.5, 4: -9.0}, None, (), 2.0, -0.3, 0.25, 0, ()),
        # +-100 near the fp16 ceiling: rounding at spacing 32, overflow to +-inf
        ("bias_ceiling", [1], [], [], {13: 100.0, 14: -100.0, 15: 100.0, 20: 100.0, 21: -100.0, 22: -100.0, 23: 16.0, 24: 15.9},
         None, (), *N, 0, ()),
        # a biased token outside the allowed set stays forbidden
        ("bias_outside_allowed", [1], [5], [], {50: 100.0, 5: 1.0, 12: 3.0}, (5, 6, 7) + tuple(range(30, 41)), (), *N, 0, ()),
        ("allowed_one", [1], [42], [], {}, (42,), (), 1.3, 0.2, 0.1, 0, ()),
        ("allowed_all_but_one", [1], [42], [], {41: -100.0}, tuple(t for t in every if t != 42), (), *N, 0, ()),
        ("allowed_shared_mask_only", [9], [6, 6], [], {6: 2.0}, (5, 6, 7) + tuple(range(30, 41)), (), 1.2, 0.0, 0.0, 0, (),
         "bias_outside_allowed"),
        # bad words: length 1, 2 and 8; the fp32 zero the processor adds turns every -0.0 into +0.0
        ("bad_single", [1], [2], [], {}, None, ((60,), (61,), (11,)), *N, 0, ()),
        ("bad_single_penalised_negzero", [11, 18], [2], [], {}, None, ((60,),), 1.7, 0.0, 0.0, 0, ()),
        ("bad_pair_match", [1], [3, 70], [], {}, None, ((70, 71),), *N, 0, ()),
        ("bad_pair_no_match", [1], [3, 69], [], {}, None, ((70, 71),), *N, 0, ()),
        ("bad_eight_match", [1], [5] + list(w8[:7]), [], {}, None, (w8,), *N, 0, ()),
        ("bad_eight_one_short", [1], list(w8[1:7]), [], {}, None, (w8,), *N, 0, ()),
        ("bad_eight_exact_outputs", [1], list(w8[:7]), [], {}, None, (w8,), *N, 0, ()),
        # a word longer than the outputs + 1 is skipped; one of exactly that length is not
        ("bad_longer_than_outputs", [1], [2, 3], [], {}, None, ((9, 2, 3, 4), (2, 3, 100)), *N, 0, ()),
        ("bad_no_outputs", [1], [], [], {}, None, ((9, 4), (101,)), *N, 0, ()),
        # a match that ends in in-flight tokens, one wholly inside them, one straddling
        ("bad_inflight_tail", [1], [3, 70], [71], {}, None, ((70, 71, 72),), *N, 0, ()),
        ("bad_inflight_whole", [1], [3], [70, 71, 73], {}, None, ((70, 71, 73, 74), (71, 73, 75), (70, 71, 76)), *N, 0, ()),
        # two words ban the same last token (the reference adds -inf twice)
        ("bad_same_last", [1], [71, 70], [], {}, None, ((70, 75), (71, 70, 75), (75, 76)), *N, 0, ()),
        # prefixes that would match only if prompt tokens were counted
        ("bad_prompt_boundary_a", [7, 90], [], [], {}, None, ((90, 91),), *N, 0, ()),
        ("bad_prompt_boundary_b", [7, 90], [91], [], {}, None, ((90, 91, 92), (91, 93)), *N, 0, ()),
        ("bad_prompt_boundary_c", [7, 90, 91], [], [92], {}, None, ((90, 91, 92, 94), (91, 92, 95), (92, 96)), *N, 0, ()),
        # everything at once, min_tokens and penalties behind: the ORDER
        ("all_order", [16, 17, 30], [31, 70, 31], [71], {16: -3.0, 17: 2.5, 31: 4.0, 33: 100.0, 50: 100.0, 35: -2.0, 11: 0.0},
         tuple(range(8, 40)) + (72, 73), ((34,), (70, 71, 72), (71, 36), (31, 71, 37)), 1.5, 0.1, 0.5, 9, (33, 35, 12)),
        ("all_order_after_min_tokens", [16, 17, 30], [31, 70, 31], [71], {16: -3.0, 17: 2.5, 31: 4.0, 33: 100.0, 35: -2.0},
         tuple(range(8, 40)) + (72, 73), ((34,), (70, 71, 72)), 1.5, 0.1, 0.5, 4, (33, 35, 12)),
    ]
    return [r if len(r) == 13 else r + (None,) for r in rows]


def main():
    assert os.path.isdir(REF), "the reference checkout is only present in the build container"
    bias_fn = _ref_def(f"{REF}/vllm/entrypoints/openai/logits_processors.py", "logit_bias_logits_processor")
    Allowed = _ref_def(f"{REF}/vllm/entrypoints/openai/logits_processors.py", "AllowedTokenIdsLogitsProcessor")
    NoBadWords = _ref_def(f"{REF}/vllm/logits_process.py", "NoBadWordsLogitsProcessor")
    apply_penalties = _load_utils().apply_penalties
    g = torch.Generator().manual_seed(37)
    rows = cases()
    n = len(rows)
    raw = (torch.randn(n, V, generator=g) * 4).to(F16)
    for t, val in ((10, 0.0), (11, -0.0), (12, -INF), (13, 65000.0), (14, -65000.0), (15, 65504.0), (16, 2.0), (17, -1.0),
                   (18, 0.0), (19, -0.0), (20, 65400.0), (21, -65504.0), (22, -65480.0), (23, 65504.0), (24, 65504.0),
                   (3, -0.0), (4, 6.0)):
        raw[:, t] = torch.tensor(val, dtype=F16)
    P, O, Fl, NB, NW = 8, 16, 4, 8, 4
    prompt = torch.full((n, P), V, dtype=torch.long)
    outs = torch.full((n, O), V, dtype=torch.long)
    infl = torch.full((n, Fl), V, dtype=torch.long)
    both = torch.full((n, O + Fl), V, dtype=torch.long)
    stop = torch.full((n, 16), -1, dtype=torch.long)
    bias_ids = np.full((n, NB), -1, np.int64)
    bias_vals = np.zeros((n, NB), np.float64)
    has_allowed = np.zeros(n, np.int32)
    allowed = np.zeros((n, V), np.bool_)
    words = np.full((n, NW, 8), -1, np.int64)
    word_lens = np.zeros((n, NW), np.int32)
    mask_only = np.zeros(n, np.int32)
    constrained = raw.clone()            # what the three processors leave
    shared = {}
    for i, (name, pr, ou, fl, bias, al, bw, rep, f, p, mt, st, share) in enumerate(rows):
        prompt[i, :len(pr)] = torch.tensor(pr, dtype=torch.long)
        if ou:
            outs[i, :len(ou)] = torch.tensor(ou)
        if fl:
            infl[i, :len(fl)] = torch.tensor(fl)
        if ou or fl:
            both[i, :len(ou) + len(fl)] = torch.tensor(ou + fl)
        if st:
            stop[i, :len(st)] = torch.tensor(st)
        procs = []
        if bias:
            procs.append(functools.partial(bias_fn, dict(bias)))
            bias_ids[i, :len(bias)] = list(bias)
            bias_vals[i, :len(bias)] = list(bias.values())
        if al is not None:
            if share is not None:
                proc = shared[share]
                assert proc.allowed_ids is None and proc.mask is not None      # the state a cached processor is in
                mask_only[i] = 1
            else:
                proc = Allowed(al)
            shared[name] = proc
            procs.append(proc)
            has_allowed[i] = 1
            allowed[i, list(al)] = True
        if bw:
            procs.append(NoBadWords([list(w) for w in bw]))
            for j, w in enumerate(bw):
                words[i, j, :len(w)] = w
                word_lens[i, j] = len(w)
        row = constrained[i]
        for proc in procs:
            row = proc(list(ou) + list(fl), row)
        constrained[i] = row
    assert constrained.dtype == F16
    masked = constrained.clone()
    for i, r in enumerate(rows):
        if len(r[2]) + len(r[3]) < r[10]:
            masked[i, list(r[11])] = -INF
    rep = torch.tensor([r[7] for r in rows], dtype=F16)
    freq = torch.tensor([r[8] for r in rows], dtype=F16)
    pres = torch.tensor([r[9] for r in rows], dtype=F16)
    expected = apply_penalties(masked.clone(), prompt, both, pres.clone(), freq.clone(), rep.clone())
    assert expected.dtype == F16
    res = dict(tc_names=np.array([r[0] for r in rows]), tc_raw=raw.numpy(), tc_prompt=prompt.numpy(), tc_outputs=outs.numpy(),
               tc_inflight=infl.numpy(), tc_bias_ids=bias_ids, tc_bias_vals=bias_vals, tc_has_allowed=has_allowed,
               tc_allowed=allowed, tc_words=words, tc_word_lens=word_lens, tc_mask_only=mask_only, tc_stop=stop.numpy(),
               tc_min_tokens=np.array([r[10] for r in rows], np.int32), tc_rep=rep.numpy(), tc_freq=freq.numpy(),
               tc_pres=pres.numpy(), tc_constrained=constrained.numpy(), tc_expected=expected.numpy())
    np.savez_compressed(os.path.join(HERE, "token_constraints.npz"), **res)
    print({k: v.shape for k, v in res.items()})


if __name__ == "__main__":
    main()
