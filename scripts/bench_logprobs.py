"""Cost of the logprobs kernel (V = 128256): the cycle form -- ops.token_logprobs_from_probs at rows = 16 (bs 4, k 3) and 192
(bs 32, k 5), num_top 0 / 5 / 20, against the torch expression the worker used before, on the same tensor, both INCLUDING the
device-to-host read of their results -- and the prompt form: ops.token_logprobs_from_logits at rows = 256, num_top 5, and a
2048-token prompt pass (Llama-3-8B synthetic weights) with and without prompt_logprobs=5.
Medians of 15 rounds, one JSON line.  Usage: python scripts/bench_logprobs.py [--no-prompt-pass]"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qspec_amd import ops  # noqa: E402

DEV, V = "cuda:0", 128256


def med_wall_us(fn, rounds=15, inner=5):
    """Host wall time per call of a fn that ends with its own host read (medians of `rounds` rounds of `inner` calls)."""
    for _ in range(3):
        fn()
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        out.append((time.perf_counter() - t0) * 1e6 / inner)
    return round(float(np.median(out)), 1)


def torch_path(probs, ids, num_top):
    """SpecDecodeWorker._create_logprob_lists_from_tensors as it was before the kernel: [k+1, B, V] logs, gather, a boolean
    compare for the ranks, topk, four host reads."""
    logp = torch.log(probs.clamp_min(torch.finfo(torch.float32).tiny)).transpose(0, 1)
    sel = logp.gather(-1, ids.unsqueeze(-1)).squeeze(-1)
    ranks = (logp > sel.unsqueeze(-1)).sum(-1) + 1
    out = [ranks.tolist(), sel.tolist()]
    if num_top:
        top_lp, top_id = logp.topk(num_top, dim=-1)
        out += [top_lp.tolist(), top_id.tolist()]
    return out


def main():
    res = {}
    g = torch.Generator(device=DEV).manual_seed(1)
    for B, k in ((4, 3), (32, 5)):
        rows = B * (k + 1)
        probs = torch.softmax(torch.randn(B, k + 1, V, device=DEV, generator=g) * 3, dim=-1)
        ids = torch.randint(0, V, (k + 1, B), device=DEV, generator=g)
        flat, flat_ids = probs.view(rows, V), ids.transpose(0, 1).contiguous().view(-1)
        for n in (0, 5, 20):
            buf = torch.empty(rows * (2 + 2 * n), dtype=torch.int32, device=DEV)
            host = torch.empty(rows * (2 + 2 * n), dtype=torch.int32, pin_memory=True)
            lp, rank = buf[:rows].view(torch.float32), buf[rows:2 * rows]
            top = buf[2 * rows:2 * rows + rows * n] if n else None
            tlp = buf[2 * rows + rows * n:].view(torch.float32) if n else None

            def kernel_path():
                ops.token_logprobs_from_probs(flat, flat_ids, n, lp, rank, top, tlp)
                host.copy_(buf, non_blocking=True)
                torch.cuda.current_stream().synchronize()
                return host.tolist()
            res[f"cycle_rows{rows}_top{n}_kernel_us"] = med_wall_us(kernel_path)
            res[f"cycle_rows{rows}_top{n}_torch_us"] = med_wall_us(lambda: torch_path(probs, ids, n))
    rows, n = 256, 5
    logits = (torch.randn(rows, V, device=DEV, generator=g) * 3).half()
    ids = torch.randint(0, V, (rows,), device=DEV, generator=g)
    buf = torch.empty(rows * (2 + 2 * n), dtype=torch.int32, device=DEV)
    host = torch.empty(rows * (2 + 2 * n), dtype=torch.int32, pin_memory=True)

    def prompt_form():
        ops.token_logprobs_from_logits(logits, ids, n, buf[:rows].view(torch.float32), buf[rows:2 * rows],
                                       buf[2 * rows:2 * rows + rows * n], buf[2 * rows + rows * n:].view(torch.float32))
        host.copy_(buf, non_blocking=True)
        torch.cuda.current_stream().synchronize()
    res["prompt_rows256_top5_kernel_us"] = med_wall_us(prompt_form)
    if "--no-prompt-pass" not in sys.argv:
        from qspec_amd.model import CONFIGS, QuarotLlamaForCausalLM
        from qspec_amd.spec_decode import QSpecEngine
        model = QuarotLlamaForCausalLM(CONFIGS["llama-3-8b"], DEV).init_synthetic(seed=0)
        eng = QSpecEngine(model, 3, 1, max_model_len=4096, block_size=16, max_new_tokens=16, use_graph=False)
        prompt = np.random.default_rng(0).integers(0, V, 2048).tolist()
        for name, kw in (("plain", {}), ("prompt_logprobs5", dict(prompt_logprobs=5))):
            def admit():
                eng.add_sequence(0, prompt, **kw)
                eng.free_slot(0)
            res[f"prompt_pass_2048_{name}_ms"] = round(med_wall_us(admit, rounds=15, inner=1) / 1000.0, 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
