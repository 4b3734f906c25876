"""Dev tool: the prompt attention behind a cached prefix, unsplit against context splits (needs a GPU).

Llama-3-8B head layout (32 / 8 / 128), block size 16, fp16 and fp8 caches; suffix q x cached prefix x sequences.  Per point,
in one process and alternating per round: S = 1 three times (their medians' range is the spread), the S that
engine.prefill_splits picks, S in {2, 4, 8, 16}, and -- with --parent-lib, a build of the parent commit
(scripts/build_dev.sh there) -- that library at S = 1.  Every variant is the call with `out` given, so a split variant pays for
its merge launch.  Device events, 15 rounds of 5 back-to-back launches, medians in microseconds per launch.  The outputs of
the rule's variant and of the baseline are compared within 1e-3 x max(1, |ref|).

    python scripts/bench_prefix_attn.py [--parent-lib build_dev/libqspec_hip_parent.so] [--out profiles/prefix_attention.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from qspec_amd import _lib, ops
from qspec_amd.spec_decode.engine import PREFILL_SPLIT_MIN_KEYS, prefill_splits

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--out", default=None)
ap.add_argument("--rounds", type=int, default=15)
args = ap.parse_args()
assert torch.cuda.is_available(), "bench_prefix_attn.py needs a GPU"
dev = "cuda:0"
NQ, NKV, D, BS, REP = 32, 8, 128, 16, 5
parent = None
if args.parent_lib:
    ops.paged_attention_workspace_bytes(1, NQ, D, 1)   # the product library (and torch's HIP runtime) first
    parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
    for name in ("qspec_paged_attention", "qspec_paged_attention_kv8"):
        getattr(parent, name).restype, getattr(parent, name).argtypes = _lib.SIGNATURES[name]

lines = []


def say(text):
    print(text, flush=True)
    lines.append(text)


say(f"# prompt attention behind a cached prefix: us per launch (out given; median of {args.rounds} rounds x {REP} launches)")
say(f"# Kmin in engine.prefill_splits while this ran: {PREFILL_SPLIT_MIN_KEYS} keys")
say("# cache n_seqs prefix    q | rule |  S=1 (x3: spread) | rule S |    S=2    S=4    S=8   S=16 | parent S=1 | verdict")
bad = 0
for fp8 in (False, True):
    for n in (1, 4):
        for prefix in (512, 2048, 8192):
            for q in (32, 128, 512):
                ctx_len, T = prefix + q, n * q
                width = -(-ctx_len // BS)
                g = torch.Generator(device=dev).manual_seed(prefix + q + n)
                kc = (torch.randn(n * width, BS, NKV, D, device=dev, generator=g) * 0.5).half()
                vc = (torch.randn(n * width, BS, NKV, D, device=dev, generator=g) * 0.5).half()
                if fp8:
                    kc, vc = kc.to(torch.float8_e4m3fn).view(torch.uint8), vc.to(torch.float8_e4m3fn).view(torch.uint8)
                bt = torch.arange(n * width, dtype=torch.int32, device=dev).view(n, width).contiguous()
                row = (NQ + 2 * NKV) * D
                qkv = (torch.randn(T, row, device=dev, generator=g) * 0.5).half()
                ctx = torch.full((n,), ctx_len, dtype=torch.int32, device=dev)
                qs = (torch.arange(n + 1, dtype=torch.int32, device=dev) * q).contiguous()
                rule = prefill_splits([q] * n, [ctx_len] * n, NKV, NQ // NKV)

                def variant(S, lib=None, T=T, q=q, n=n, width=width, kc=kc, vc=vc, bt=bt, qkv=qkv, ctx=ctx, qs=qs, fp8=fp8):
                    ws = torch.zeros(ops.paged_attention_workspace_bytes(T, NQ, D, S), dtype=torch.uint8, device=dev)
                    out = torch.empty(T, NQ * D, dtype=torch.float16, device=dev)
                    lib = lib or _lib.load()   # both libraries through the same bare call: equal host cost per launch
                    scales = (1.0, 1.0) if fp8 else ()
                    fn = lib.qspec_paged_attention_kv8 if fp8 else lib.qspec_paged_attention
                    st = torch.cuda.current_stream().cuda_stream
                    return out, lambda: _lib.check(fn(qkv.data_ptr(), row, kc.data_ptr(), vc.data_ptr(), *scales, bt.data_ptr(), width,
                                                      ctx.data_ptr(), qs.data_ptr(), n, T, q, NQ, NKV, D, BS, D ** -0.5, S,
                                                      ws.data_ptr(), out.data_ptr(), st))
                names = ["S1a", "S1b", "S1c", "rule", "S2", "S4", "S8", "S16"] + (["parent"] if parent else [])
                made = [variant(1), variant(1), variant(1), variant(rule), variant(2), variant(4), variant(8), variant(16)]
                if parent:
                    made.append(variant(1, parent))
                times = {k: [] for k in names}
                for _, f in made:
                    f()
                torch.cuda.synchronize()
                for r in range(args.rounds):
                    order = list(range(len(names)))
                    order = order[r % len(order):] + order[:r % len(order)]   # alternate who goes first
                    for i in order:
                        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        a.record()
                        for _ in range(REP):
                            made[i][1]()
                        b.record()
                        torch.cuda.synchronize()
                        times[names[i]].append(a.elapsed_time(b) / REP * 1e3)
                med = {k: statistics.median(v) for k, v in times.items()}
                s1 = [med["S1a"], med["S1b"], med["S1c"]]
                spread, base = max(s1) - min(s1), med.get("parent", statistics.median(s1))
                ref, got = made[-1][0].float() if parent else made[0][0].float(), made[3][0].float()
                agree = bool(((got - ref).abs() <= 1e-3 * ref.abs().clamp(min=1.0)).all())
                best = min(("S2", "S4", "S8", "S16"), key=lambda k: med[k])
                if rule > 1:
                    ok = med["rule"] < base - spread
                    verdict = "rule wins" if ok else "RULE LOSES"
                else:
                    ok = med[best] >= statistics.median(s1) - spread
                    verdict = "1 is right" if ok else f"RULE MISSES {best}"
                bad += (not ok) + (not agree)
                say(f"{'fp8 ' if fp8 else 'fp16'} {n:6d} {prefix:6d} {q:4d} | {rule:4d} | {s1[0]:7.1f} {s1[1]:7.1f} {s1[2]:7.1f} ({spread:5.1f}) | "
                    f"{med['rule']:7.1f} | {med['S2']:7.1f} {med['S4']:7.1f} {med['S8']:7.1f} {med['S16']:7.1f} | "
                    f"{med.get('parent', float('nan')):10.1f} | {verdict}{'' if agree else ' OUTPUTS DIFFER'}")
say(f"# points where the rule loses, misses or the outputs differ: {bad}")
if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
sys.exit(1 if bad else 0)
