"""Seeded vs unseeded sampling entries (dev tool): ops.sample_top_k_top_p at T = 4, 16, 192 and ops.rejection_sample at
(B, k) = (4, 3), (32, 5), vocabulary 128256.  The two forms are timed alternately with device events, each from a captured
graph of REPS calls; prints the median and the spread (min..max) per form over ROUNDS rounds, one JSON line per shape."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from qspec_amd import ops

DEV = "cuda:0"
V = 128256
REPS, ROUNDS = 20, 15


def _graph(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(REPS):
            fn()
    torch.cuda.synchronize()
    return g


def _time(g):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    g.replay()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / REPS


def _ab(name, plain, seeded):
    graphs = {"unseeded": _graph(plain), "seeded": _graph(seeded)}
    for g in graphs.values():
        g.replay()
    torch.cuda.synchronize()
    ts = {k: [] for k in graphs}
    for _ in range(ROUNDS):
        for k, g in graphs.items():
            ts[k].append(_time(g))
    res = {"shape": name}
    for k, v in ts.items():
        v = sorted(v)
        res[k] = {"median_us": round(v[len(v) // 2], 2), "min_us": round(v[0], 2), "max_us": round(v[-1], 2)}
    print(json.dumps(res), flush=True)


def main():
    torch.manual_seed(0)
    for T in (4, 16, 192):
        logits = (torch.randn(T, V, device=DEV) * 3).half()
        probs = torch.empty(T, V, dtype=torch.float32, device=DEV)
        tok = torch.empty(T, dtype=torch.int64, device=DEV)
        temp = torch.full((T,), 0.8, device=DEV)
        topk = torch.full((T,), 50, dtype=torch.int32, device=DEV)
        topp = torch.full((T,), 0.9, device=DEV)
        rs = torch.tensor([1, 0], dtype=torch.int64, device=DEV)
        ws = ops.new_sample_workspace(T, DEV)
        seeds = torch.arange(T, dtype=torch.int64, device=DEV) + 1000
        seeded = torch.ones(T, dtype=torch.int32, device=DEV)
        base = torch.full((T,), 77, dtype=torch.int32, device=DEV)
        _ab(f"sample_top_k_top_p T={T}",
            lambda: ops.sample_top_k_top_p(logits, probs, tok, temp, topk, topp, rng_state=rs, workspace=ws),
            lambda: ops.sample_top_k_top_p(logits, probs, tok, temp, topk, topp, rng_state=rs, workspace=ws, seq_seeds=seeds,
                                           seq_seeded=seeded, base_pos=base, draw_stream=2))
    for B, k in ((4, 3), (32, 5)):
        tq = torch.softmax(torch.randn(B, k + 1, V, device=DEV), -1)
        dp = torch.softmax(torch.randn(B, k, V, device=DEV), -1)
        ids = torch.randint(0, V, (B, k), device=DEV)
        bonus = torch.randint(0, V, (B,), device=DEV)
        out = torch.empty(B, k + 1, dtype=torch.int64, device=DEV)
        acc = torch.empty(B, k, dtype=torch.uint8, device=DEV)
        rec = torch.empty(B, k, dtype=torch.int64, device=DEV)
        rs = torch.tensor([1, 0], dtype=torch.int64, device=DEV)
        seeds = torch.arange(B, dtype=torch.int64, device=DEV) + 1000
        seeded = torch.ones(B, dtype=torch.int32, device=DEV)
        base = torch.full((B,), 77, dtype=torch.int32, device=DEV)
        _ab(f"rejection_sample B={B} k={k}",
            lambda: ops.rejection_sample(tq, bonus, dp, ids, out, acc, rec, rng_state=rs),
            lambda: ops.rejection_sample(tq, bonus, dp, ids, out, acc, rec, rng_state=rs, seq_seeds=seeds, seq_seeded=seeded,
                                         base_pos=base))


if __name__ == "__main__":
    main()
