"""Cost of the KV block operations at Llama-3-8B cache geometry (32 layers, 8 KV heads, head size 128, block size 16), fp16 and
fp8 caches: QSpecEngine.copy_blocks at 1 / 32 / 256 pairs and swap_out + swap_in at 32 / 256 blocks, against the torch
expressions a user would otherwise write -- per layer `cache[dst] = cache[src]` for K and V (64 indexed copies), and per block
and per layer a `copy_` of K and V to / from a pinned tensor.  Both sides include the upload of their indices and end with a
stream synchronisation.  Beside the times: bytes moved per second (read + written for the device copy, one way for the
swap), and the host-link rate of the box (one 512 MiB pinned copy each way).
Medians of 15 rounds, one JSON line.  Usage: python scripts/bench_block_ops.py"""
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qspec_amd.spec_decode import QSpecEngine  # noqa: E402

DEV = "cuda:0"
LAYERS, NKV, D, BS = 32, 8, 128, 16
GPU_BLOCKS, CPU_BLOCKS = 1024, 256


def med_us(fn, rounds=15, inner=3):
    for _ in range(2):
        fn()
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e6 / inner)
    return round(float(np.median(out)), 1)


def cache_engine(dtype):
    """An engine shell holding nothing but the caches: the block operations read the cache tensors, the device and the two
    block counts, so no model is loaded for this measurement."""
    eng = QSpecEngine.__new__(QSpecEngine)
    eng.device, eng.num_blocks = torch.device(DEV), GPU_BLOCKS
    raw = (GPU_BLOCKS, BS, NKV, D * torch.empty(0, dtype=dtype).element_size())     # random bytes, viewed as the cache dtype
    eng.kv_caches = [tuple(torch.randint(0, 256, raw, dtype=torch.uint8, device=DEV).view(dtype) for _ in range(2))
                     for _ in range(LAYERS)]
    eng.allocate_cpu_cache(CPU_BLOCKS)
    return eng


def main():
    res = {}
    for name, dtype in (("fp16", torch.float16), ("fp8", torch.uint8)):
        eng = cache_engine(dtype)
        block_bytes = BS * NKV * D * eng.kv_caches[0][0].element_size()
        record = 2 * LAYERS * block_bytes
        res[f"{name}_record_bytes"] = record
        for n in (1, 32, 256):
            pairs = [(i, 512 + i) for i in range(n)]

            def torch_copy():
                src = torch.tensor([s for s, _ in pairs]).to(DEV)
                dst = torch.tensor([d for _, d in pairs]).to(DEV)
                for k, v in eng.kv_caches:
                    k[dst] = k[src]
                    v[dst] = v[src]
            us = med_us(lambda: eng.copy_blocks(pairs))
            res[f"{name}_copy{n}_kernel_us"], res[f"{name}_copy{n}_torch_us"] = us, med_us(torch_copy)
            res[f"{name}_copy{n}_kernel_GBps"] = round(2 * n * record / us / 1e3, 1)      # read + written
        # the torch swap: pinned per-layer K and V host tensors, one copy_ per block, layer and K / V
        host = [(torch.empty((CPU_BLOCKS, BS, NKV, D), dtype=dtype, pin_memory=True),
                 torch.empty((CPU_BLOCKS, BS, NKV, D), dtype=dtype, pin_memory=True)) for _ in range(LAYERS)]
        for n in (32, 256):
            out_pairs = [(2 * i, i) for i in range(n)]
            in_pairs = [(i, 600 + i) for i in range(n)]

            def kernel_swap():
                eng.swap_out(out_pairs)
                eng.swap_in(in_pairs)

            def torch_swap():
                for g, c in out_pairs:
                    for (k, v), (hk, hv) in zip(eng.kv_caches, host):
                        hk[c].copy_(k[g], non_blocking=True)
                        hv[c].copy_(v[g], non_blocking=True)
                for c, g in in_pairs:
                    for (k, v), (hk, hv) in zip(eng.kv_caches, host):
                        k[g].copy_(hk[c], non_blocking=True)
                        v[g].copy_(hv[c], non_blocking=True)
            us = med_us(kernel_swap, inner=1)
            res[f"{name}_swap{n}_kernel_us"], res[f"{name}_swap{n}_torch_us"] = us, med_us(torch_swap, rounds=5, inner=1)
            res[f"{name}_swap{n}_kernel_GBps"] = round(2 * n * record / us / 1e3, 1)      # out + in, one way each
        del eng, host
        torch.cuda.empty_cache()
    nbytes = 512 << 20
    pinned, dev = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True), torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    res["host_link_d2h_GBps"] = round(nbytes / med_us(lambda: pinned.copy_(dev, non_blocking=True), inner=1) / 1e3, 1)
    res["host_link_h2d_GBps"] = round(nbytes / med_us(lambda: dev.copy_(pinned, non_blocking=True), inner=1) / 1e3, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
