"""Writes tests/golden/logit_processors.npz: inputs and outputs of the reference's OWN logit processors run on CPU.

  * vllm/model_executor/layers/utils.py     apply_penalties (:24-57), imported from the reference file (plain torch), run in fp16
    as Sampler.forward runs it (sampler.py:262-266), one row per "sequence" -- where it is well defined;
  * vllm/model_executor/layers/sampler.py   _apply_min_p (:416-430), compiled from the reference file the way make_golden.py takes
    _apply_top_k_top_p and _multinomial, behind the reference's own _apply_top_k_top_p, temperature and softmax as :266-287.
The min_tokens mask (_apply_min_tokens_penalty, :338-384, needs SamplingMetadata objects) is its one effect -- the stop ids of a
row that has generated fewer than min_tokens tokens set to -inf -- applied here in front of apply_penalties, as Sampler.forward
orders them.

Only recorded inputs and outputs are written.  Needs the reference checkout (present only in the build container).
Run: python tests/golden/make_logit_processors.py
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, _ref_function  # noqa: E402

V = 1000
F16 = torch.float16


def _load_utils():
    spec = importlib.util.spec_from_file_location("ref_layers_utils", f"{REF}/vllm/model_executor/layers/utils.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def gen_penalties(out):
    apply_penalties = _load_utils().apply_penalties
    g = torch.Generator().manual_seed(29)
    rows = []   # (prompt, committed outputs, in flight, rep, freq, pres, min_tokens, stop ids)
    A, B, C, D1, D2, D7, D300 = 11, 22, 33, 44, 55, 66, 77          # prompt only / outputs only / both / counts 1, 2, 7, 300
    base_prompt = [A, C, 101, 102, 103, 999, 0]
    base_out = [B, C, D1] + [D2] * 2 + [D7] * 7 + [D300] * 300
    combos = [(1.2, 0.0, 0.0), (1.0, 0.1, 0.0), (1.0, 0.0, 0.5), (1.2, 0.1, 0.5), (0.8, 0.0, 0.0), (2.5, 1.5, 2.0),
              (1.0, -0.3, 0.0), (1.0, 0.0, -0.25), (1.3, -0.3, -0.25), (1.0, 0.0, 0.0), (1.05, 0.02, 0.01), (1.7, 0.7, 0.0)]
    for rep, f, p in combos:
        rows.append((base_prompt, base_out, [], rep, f, p, 0, []))
    # in-flight tokens (rows j = 1..3 of a cycle), min_tokens before and after the threshold, empty outputs, empty-ish prompt
    rows.append((base_prompt, base_out, [D1], 1.2, 0.1, 0.5, 0, []))
    rows.append((base_prompt, base_out, [D1, 500, 500], 1.2, 0.1, 0.5, 0, []))
    rows.append((base_prompt, [B, C], [], 1.2, 0.1, 0.5, 3, [5, 6, 7, C]))            # 2 < 3: masked, C is penalised too
    rows.append((base_prompt, [B, C], [D1], 1.2, 0.1, 0.5, 3, [5, 6, 7, C]))          # 2 + 1 = 3: no longer masked
    rows.append((base_prompt, [], [], 1.5, 0.4, 0.4, 1, list(range(16))))             # sixteen stop ids, nothing generated
    rows.append(([3], [], [], 1.0, 0.0, 0.0, 5, [3]))                                 # neutral penalties, mask only
    rows.append(([A], [A, A, A], [A], 0.5, -1.0, 1.0, 0, []))
    N = len(rows)
    raw = (torch.randn(N, V, generator=g) * 4).to(F16)
    # the special values on tokens the penalties touch and on tokens they do not
    for t, val in ((A, 0.0), (B, -0.0), (101, 3.5), (102, -3.5), (D300, 2.0), (D7, -1.0), (400, 0.0), (401, -0.0),
                   (D2, float("-inf")), (402, float("-inf")), (C, 6.1e-5), (D1, -6.0e-8)):
        raw[:, t] = torch.tensor(val, dtype=F16)
    raw[3, D300] = 60000.0
    P = max(len(r[0]) for r in rows)
    O = max(len(r[1]) for r in rows)
    Fl = max(len(r[2]) for r in rows)
    S = 16
    prompt = torch.full((N, P), V, dtype=torch.long)
    outs = torch.full((N, O), V, dtype=torch.long)
    infl = torch.full((N, max(Fl, 1)), V, dtype=torch.long)
    both = torch.full((N, O + Fl), V, dtype=torch.long)      # what the sampler of a NON-speculative run would be handed
    stop = torch.full((N, S), -1, dtype=torch.long)
    masked = raw.clone()
    for i, (pr, ou, fl, rep, f, p, mt, st) in enumerate(rows):
        prompt[i, :len(pr)] = torch.tensor(pr, dtype=torch.long)
        if ou:
            outs[i, :len(ou)] = torch.tensor(ou)
        if fl:
            infl[i, :len(fl)] = torch.tensor(fl)
        if ou or fl:
            both[i, :len(ou) + len(fl)] = torch.tensor(ou + fl)
        if st:
            stop[i, :len(st)] = torch.tensor(st)
        if len(ou) + len(fl) < mt:
            masked[i, st] = float("-inf")
    rep = torch.tensor([r[3] for r in rows], dtype=F16)
    freq = torch.tensor([r[4] for r in rows], dtype=F16)
    pres = torch.tensor([r[5] for r in rows], dtype=F16)
    expected = apply_penalties(masked.clone(), prompt, both, pres.clone(), freq.clone(), rep.clone())
    assert expected.dtype == F16
    out.update(pen_raw=raw.numpy(), pen_prompt=prompt.numpy(), pen_outputs=outs.numpy(), pen_inflight=infl.numpy(),
               pen_stop=stop.numpy(), pen_min_tokens=np.array([r[6] for r in rows], np.int32), pen_rep=rep.numpy(),
               pen_freq=freq.numpy(), pen_pres=pres.numpy(), pen_expected=expected.numpy())


def gen_min_p(out):
    sampler = f"{REF}/vllm/model_executor/layers/sampler.py"
    apply_tk_tp, apply_min_p, multinomial = _ref_function(sampler, "_apply_top_k_top_p", "_apply_min_p", "_multinomial")
    g = torch.Generator().manual_seed(31)
    allh = torch.arange(-2 ** 15, 2 ** 15, dtype=torch.int32).to(torch.int16).view(F16)
    pool = torch.unique(allh[torch.isfinite(allh) & (allh.abs() < 10) & (allh.abs() > 1e-3)])
    cases = [(t, -1, 1.0, mp) for mp in (0.02, 0.1, 0.5, 1.0) for t in (0.7, 1.0, 1.5)]
    cases += [(0.7, 50, 1.0, 0.1), (1.0, -1, 0.9, 0.02), (1.5, 40, 0.95, 0.1), (1.0, 5, 0.5, 0.5), (1.0, -1, 1.0, 1.0)]
    T = len(cases)
    logits = torch.stack([pool[torch.randperm(pool.numel(), generator=g)[:V]] for _ in range(T)])    # distinct per row
    top = logits[-1].max()
    logits[-1, [17, 400, 999]] = top                                       # the last row: several tokens tied at the maximum
    temperature = torch.tensor([c[0] for c in cases], dtype=torch.float32)
    top_k = torch.tensor([V if c[1] == -1 else c[1] for c in cases], dtype=torch.int32)
    top_p = torch.tensor([c[2] for c in cases], dtype=torch.float32)
    min_p = torch.tensor([c[3] for c in cases], dtype=torch.float32)
    lf = logits.to(torch.float)
    lf.div_(temperature.unsqueeze(dim=1))
    masked = apply_tk_tp(lf.clone(), top_p, top_k)
    # the reference compares p < min_p * p_max in fp32: a token within rounding of the threshold is undecidable.  Every token
    # must be a relative 1e-4 away from it -- or have the row maximum's own logit (its probability IS p_max, bit for bit: the
    # comparison is exact) -- so that NO token is exempted from the kept-set check
    pr = torch.softmax(masked.double(), dim=-1)
    ratio = pr / pr.max(dim=-1, keepdim=True).values
    at_max = masked == masked.max(dim=-1, keepdim=True).values
    rel = ((ratio / min_p.double().unsqueeze(1)) - 1).abs()
    assert bool((at_max | (rel >= 1e-4)).all()), float(rel[~at_max].min())
    print("min_p: closest relative distance to the threshold", float(rel[~at_max].min()))
    masked = apply_min_p(masked, min_p.clone())
    probs = torch.softmax(masked, dim=-1, dtype=torch.float)
    E = torch.empty(T, V).exponential_(1.0, generator=g)
    orig = torch.Tensor.exponential_
    try:
        torch.Tensor.exponential_ = lambda self, *a, **kw: self.copy_(E)
        tok = multinomial(probs.clone(), 1).view(-1)
    finally:
        torch.Tensor.exponential_ = orig
    keep = torch.isfinite(masked)
    assert int(keep[-1].sum()) == 4 and all(int(keep[i].sum()) >= 1 for i in range(T))
    out.update(mp_logits=logits.numpy(), mp_temperature=temperature.numpy(), mp_top_k=top_k.numpy(), mp_top_p=top_p.numpy(),
               mp_min_p=min_p.numpy(), mp_E=E.numpy(), mp_keep=keep.numpy(), mp_probs=probs.numpy(), mp_token=tok.numpy())


if __name__ == "__main__":
    assert os.path.isdir(REF), "the reference checkout is only present in the build container"
    res = {}
    gen_penalties(res)
    gen_min_p(res)
    np.savez_compressed(os.path.join(HERE, "logit_processors.npz"), **res)
    print({k: v.shape for k, v in res.items()})
