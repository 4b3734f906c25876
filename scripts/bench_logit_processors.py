"""Cost of the logit processors: the pre-pass at T = 4 / 16 / 192 (V = 128256), the min_p entry against the plain one, and the
processed cycle against the sampling cycle (tiny model shapes are not the point: Llama-3-8B synthetic weights, bs = 4, k = 3).
Medians of 15 rounds of 20 launches, one JSON line.  Usage: python scripts/bench_logit_processors.py [--no-cycle]"""
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
    g = torch.Generator(device=DEV).manual_seed(1)
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
                 gen_base=torch.zeros(B, **i32), gen_lens=torch.zeros(B, **i32), stop_ids=torch.zeros(B, 16, **i32),
                 num_stop_ids=torch.zeros(B, **i32), draft_ids=torch.zeros(3, B, dtype=torch.int64, device=DEV))
        rps = 4 if T >= 4 else 1
        res[f"prepass_T{T}_us"] = med_us(lambda: ops.process_logits(lg, out, rows_per_seq=rps, j_base=0, **a))
        probs = torch.empty(T, V, dtype=torch.float32, device=DEV)
        tok = torch.empty(T, dtype=torch.int64, device=DEV)
        temp = torch.full((T,), 0.8, device=DEV)
        rng = torch.tensor([1, 0], dtype=torch.int64, device=DEV)
        mp = torch.full((T,), 0.05, device=DEV)
        res[f"sample_T{T}_us"] = med_us(lambda: ops.sample_top_k_top_p(lg, probs, tok, temp, rng_state=rng))
        res[f"sample_min_p_T{T}_us"] = med_us(lambda: ops.sample_top_k_top_p(lg, probs, tok, temp, rng_state=rng, min_p=mp))
    if "--no-cycle" not in sys.argv:
        from qspec_amd.model import CONFIGS, QuarotLlamaForCausalLM
        from qspec_amd.spec_decode import QSpecEngine
        model = QuarotLlamaForCausalLM(CONFIGS["llama-3-8b"], DEV).init_synthetic(seed=0)
        rs = np.random.default_rng(0)
        for name, kw in (("sampling", dict(temperature=0.8)), ("processed", dict(temperature=0.8, repetition_penalty=1.2, min_p=0.05))):
            eng = QSpecEngine(model, 3, 4, max_model_len=1024, block_size=16, max_new_tokens=900, use_graph=True)
            for b in range(4):
                eng.set_sampling_params(b, **kw)
            eng.add_sequences_to([0, 1, 2, 3], [rs.integers(0, V, 512).tolist() for _ in range(4)])
            eng.step()
            res[f"cycle_{name}_ms"] = round(med_us(eng.step, rounds=15, inner=5) / 1000.0, 4)
            del eng
    print(json.dumps(res))


if __name__ == "__main__":
    main()
