"""Cost of the token constraints: the plain pre-pass entry (must not move), the constrained entry with (a) one slot constrained
and (b) every slot carrying a deny mask, 512 biases and 32 bad words, at T = 4 / 16 / 192 (V = 128256); and the processed cycle
with and without a constrained request (Llama-3-8B synthetic weights, bs = 4, k = 3).
Medians of 15 rounds of 20 launches, one JSON line.  Usage: python scripts/bench_token_constraints.py [--no-cycle] [--plain-only]
(--plain-only: what a build without the constrained entry can run, for the before / after comparison)"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qspec_amd import ops  # noqa: E402

DEV, V = "cuda:0", 128256


def med_us(fn, rounds=15, inner=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1000.0 / inner)
    return round(float(np.median(out)), 2)


def main():
    res = {}
    plain_only = "--plain-only" in sys.argv
    g = torch.Generator(device=DEV).manual_seed(1)
    rs = np.random.default_rng(0)
    for T in (4, 16, 192):
        B = max(1, T // 4)
        lg = (torch.randn(T, V, device=DEV, generator=g) * 3).half()
        out = torch.empty_like(lg)
        table, counted = ops.new_logit_table(B, V, DEV)
        table.random_(0, 3)
        i32 = dict(dtype=torch.int32, device=DEV)
        a = dict(tok_table=table, repetition=torch.full((B,), 1.2, dtype=torch.float16, device=DEV),
                 frequency=torch.full((B,), 0.1, dtype=torch.float16, device=DEV),
                 presence=torch.full((B,), 0.5, dtype=torch.float16, device=DEV), min_tokens=torch.zeros(B, **i32),
                 gen_base=torch.zeros(B, **i32), gen_lens=torch.full((B,), 40, **i32), stop_ids=torch.zeros(B, 16, **i32),
                 num_stop_ids=torch.zeros(B, **i32), draft_ids=torch.zeros(3, B, dtype=torch.int64, device=DEV))
        res[f"prepass_T{T}_us"] = med_us(lambda: ops.process_logits(lg, out, rows_per_seq=4, j_base=0, **a))
        if plain_only:
            continue
        gen = torch.randint(0, V, (B, 64), dtype=torch.int64, device=DEV)
        heavy = dict(logit_bias={int(t): 1.5 for t in rs.choice(V, 512, replace=False)},
                     allowed_token_ids=[int(t) for t in np.nonzero(rs.random(V) < 0.5)[0]],
                     bad_words_token_ids=[[int(t) for t in rs.integers(0, V, 8)] for _ in range(32)] + [[7], [9]])
        for name, slots in (("none", []), ("one", [0]), ("all", list(range(B)))):
            tc = ops.TokenConstraints(B, V, DEV)
            for s in slots:
                ops.token_constraints_set(tc, s, **heavy)
            res[f"prepass_constrained_{name}_T{T}_us"] = med_us(lambda: ops.process_logits_constrained(
                lg, out, deny=tc.deny, meta=tc.meta, bias_ids=tc.bias_ids, bias_vals=tc.bias_vals, words=tc.words,
                word_lens=tc.word_lens, tail=tc.tail, gen_tokens=gen, rows_per_seq=4, j_base=0, **a))
    if "--no-cycle" not in sys.argv:
        from qspec_amd.model import CONFIGS, QuarotLlamaForCausalLM
        from qspec_amd.spec_decode import QSpecEngine
        model = QuarotLlamaForCausalLM(CONFIGS["llama-3-8b"], DEV).init_synthetic(seed=0)
        pen = dict(temperature=0.8, repetition_penalty=1.2, min_p=0.05)
        cons = dict(logit_bias={t: 0.5 for t in range(1000, 1512)}, allowed_token_ids=list(range(0, V, 2)),
                    bad_words_token_ids=[[int(t) for t in rs.integers(0, V, 4)] for _ in range(32)])
        variants = [("processed", [pen] * 4)]
        if not plain_only:
            variants += [("constrained_one", [dict(pen, **cons)] + [pen] * 3), ("constrained_all", [dict(pen, **cons)] * 4)]
        for name, kws in variants:
            eng = QSpecEngine(model, 3, 4, max_model_len=1024, block_size=16, max_new_tokens=900, use_graph=True)
            for b in range(4):
                eng.set_sampling_params(b, **kws[b])
            eng.add_sequences_to([0, 1, 2, 3], [rs.integers(0, V, 512).tolist() for _ in range(4)])
            eng.step()
            res[f"cycle_{name}_ms"] = round(med_us(eng.step, rounds=15, inner=5) / 1000.0, 4)
            del eng
    print(json.dumps(res))


if __name__ == "__main__":
    main()
