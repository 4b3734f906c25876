"""Graph-replay micro-benchmark of the paged attention launch over an fp16 and an fp8 (e4m3) KV cache (dev tool).

Decode / verify shapes: bs in {4, 32}, q_len in {1, 4, 6}, ctx in {512, 2048, 8192}, partials only (the form the engine
launches), the engine's split count; the prompt pass at 512 and 4096 tokens (one sequence, one split).  One line per
shape: us per launch for both caches, alternating fp16 / fp8 measurements (PAIRS pairs, the median of each).
  CYCLE=1 also times the whole captured cycle of the headline (Llama-3-8B, bs 4, k 3) and config-3 (bs 32, k 5) shapes in
  both modes and prints the acceptance rate of the synthetic weights under each cache.
  PMC=fp16|fp8 (with PMC_SHAPE="bs,q_len,ctx", default 32,1,2048) launches that one decode shape eagerly a few times over
  that cache and nothing else: the workload of a counter pass of its own,
      rocprofv3 --pmc FETCH_SIZE --output-format csv -d DIR -- python3 scripts/bench_kv_fp8.py
  (no tracing flag beside --pmc), whose counter_collection.csv scripts/pmc_traffic.py turns into bytes per launch.
The fp8 caches are quantised at scale 1 and the launches pass the default scales (1, 1): the folded softmax scale and the
v_scale multiply at the store are timed in their trivial form (one fp32 multiply per stored element either way).
Llama-3-8B head layout: 32 query heads, 8 kv heads of 128, block size 16."""
import os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from qspec_amd import ops
dev = "cuda:0"
nq, nkv, d, bs = 32, 8, 128, 16
PAIRS = int(os.environ.get("PAIRS", 3))


def timed(f, inner=20, reps=5):
    f(); torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(inner): f()
    g.replay(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps): g.replay()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / (inner * reps) * 1e3


def shape(B, q_len, ctx0, n_splits, partial, pmc=None):
    max_blocks = (ctx0 + bs - 1) // bs + 1
    nb = B * max_blocks
    k16 = (torch.randn(nb, bs, nkv, d, device=dev) * 0.5).half(); v16 = (torch.randn_like(k16.float()) * 0.5).half()
    k8 = k16.float().clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8); v8 = v16.float().clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
    bt = torch.arange(nb, dtype=torch.int32, device=dev).view(B, -1).contiguous()
    T = B * q_len
    row = (nq + 2 * nkv) * d
    qkv = (torch.randn(T, row, device=dev) * 0.5).half()
    ctx = torch.full((B,), ctx0, dtype=torch.int32, device=dev)
    qs = (torch.arange(B + 1, dtype=torch.int32, device=dev) * q_len).contiguous()
    ws = torch.zeros(ops.paged_attention_workspace_bytes(T, nq, d, n_splits), dtype=torch.uint8, device=dev)
    out = None if partial else torch.empty(T, nq * d, dtype=torch.float16, device=dev)
    mk = lambda kc, vc: (lambda: ops.paged_attention(qkv, row, kc, vc, bt, ctx, qs, T, q_len, nq, d ** -0.5, n_splits, ws, out))
    f16, f8 = mk(k16, v16), mk(k8, v8)
    if pmc:   # counter pass: four eager launches over one cache, a host sync behind each
        for _ in range(4):
            (f8 if pmc == "fp8" else f16)(); torch.cuda.synchronize()
        return
    t16, t8 = [], []
    for _ in range(PAIRS):
        t16.append(timed(f16)); t8.append(timed(f8))
    kv_mb = 2 * B * ctx0 * nkv * d * 2 / 1e6
    return statistics.median(t16), statistics.median(t8), kv_mb


if os.environ.get("PMC"):
    from qspec_amd.spec_decode.engine import n_splits_for
    mode = os.environ["PMC"]
    assert mode in ("fp16", "fp8"), mode
    B, q_len, ctx0 = (int(x) for x in os.environ.get("PMC_SHAPE", "32,1,2048").split(","))
    shape(B, q_len, ctx0, n_splits_for(ctx0 + bs, B * nkv), True, pmc=mode)
    print(f"pmc workload: decode bs={B} q_len={q_len} ctx={ctx0} cache={mode}: K + V of the context = "
          f"{2 * B * ctx0 * nkv * d * (1 if mode == 'fp8' else 2) / 1e6:.1f} MB per launch", flush=True)
elif os.environ.get("CYCLE", "0") != "1":
    from qspec_amd.spec_decode.engine import n_splits_for
    for B in (4, 32):
        for q_len in (1, 4, 6):
            for ctx0 in (512, 2048, 8192):
                S = n_splits_for(ctx0 + bs, B * nkv)
                a, b, mb = shape(B, q_len, ctx0, S, True)
                print(f"decode bs={B} q_len={q_len} ctx={ctx0} n_splits={S} kv_fp16={mb:.1f}MB: fp16 {a:.2f} us, fp8 {b:.2f} us, fp8/fp16 {b / a:.3f}", flush=True)
    for n in (512, 4096):
        a, b, mb = shape(1, n, n, 1, False)
        print(f"prompt tokens={n}: fp16 {a:.1f} us, fp8 {b:.1f} us, fp8/fp16 {b / a:.3f}", flush=True)
else:
    from qspec_amd.model import CONFIGS, QuarotLlamaForCausalLM
    from qspec_amd.spec_decode import QSpecEngine
    import dataclasses
    cfg = dataclasses.replace(CONFIGS["llama-3-8b"], num_hidden_layers=int(os.environ.get("LAYERS", 4)))
    model = QuarotLlamaForCausalLM(cfg, dev).init_synthetic(seed=1)
    for name, B, k, plen in (("headline", 4, 3, 512), ("config-3", 32, 5, 512)):
        for mode in ("auto", "fp8") * PAIRS:
            eng = QSpecEngine(model, k, B, max_model_len=1024, block_size=bs, max_new_tokens=256, use_graph=True, seed=0,
                              kv_cache_dtype=mode)
            g = torch.Generator().manual_seed(0)
            eng.add_sequences([torch.randint(0, cfg.vocab_size, (plen,), generator=g).tolist() for _ in range(B)])
            for _ in range(3): eng.step()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(20): eng.step()
            b.record(); torch.cuda.synchronize()
            m = eng.metrics()
            print(f"cycle {name} layers={cfg.num_hidden_layers} kv={mode}: {a.elapsed_time(b) / 20:.3f} ms/cycle, acceptance {m.draft_acceptance_rate:.3f}", flush=True)
            del eng
