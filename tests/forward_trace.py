"""Launch traces of QuarotLlamaForCausalLM.forward for tests/test_forward_launches_gpu.py: one forward per case with
ops._call wrapped (and still called), every launch written down as `entry(arg, ...)` -- scalars as they are (floats by
repr), a pointer as the name of the tensor that contains it plus the byte offset, the trailing stream dropped.  The cases
are the smallest shapes that reach every launch form of forward(): 2-layer models (the hand-over between layers needs two)
at the layer widths of three families and of test_model_gpu.tiny_cfg(), with the paged inputs of test_model_gpu.make_inputs.

tests/golden/forward_launches.json holds the traces of the commit BEFORE forward() was split into a launch plan and stage
methods; this file uses only names that commit has too, so `python tests/forward_trace.py` on that commit rewrites it."""
import functools
import json
import os
from types import SimpleNamespace

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forward_launches.json")
DEV = "cuda:0"
WIDTHS = {   # hidden, intermediate, heads, kv heads, rope theta
    "8b": (4096, 14336, 32, 8, 500000.0),
    "13b": (5120, 13824, 40, 40, 10000.0),     # 40 heads: a table factor on the head axis
    "tl": (2048, 5632, 32, 4, 10000.0),        # head size 64
    "tiny": None,                              # test_model_gpu.tiny_cfg(): 8 heads, the generic head transform
}
KV8_SCALES = [(0.5, 0.25), (2.0, 0.75)]


def _case(width, draft, T, knobs=None, kv8=False, tp=False):
    name = f"{width}-{'draft' if draft else 'verify'}-T{T}"
    name += "".join(f"-{k}={int(v)}" for k, v in (knobs or {}).items()) + ("-kv8" if kv8 else "") + ("-tp" if tp else "")
    return name, SimpleNamespace(width=width, draft=draft, T=T, knobs=knobs or {}, kv8=kv8, tp=tp)


CASES = dict([
    _case("8b", True, 4), _case("8b", True, 4, {"HADAMARD_QUANT_IN_OPROJ": False}), _case("8b", True, 8),
    _case("8b", True, 32), _case("8b", False, 16), _case("8b", False, 32), _case("8b", False, 32, {"XP32_DOWN_SLICES": False}),
    _case("8b", False, 48), _case("8b", False, 16, {"ACT_FRAGMENT_MAJOR": False}),
    _case("8b", False, 32, {"ACT_FRAGMENT_MAJOR": False}), _case("8b", False, 16, {"VERIFY_O_SLICES": 2}),
    _case("8b", True, 4, kv8=True), _case("8b", False, 16, kv8=True), _case("8b", False, 8, tp=True),
    _case("13b", True, 4), _case("13b", False, 16), _case("13b", False, 24),
    _case("tl", True, 4), _case("tl", True, 40), _case("tl", False, 8), _case("tl", False, 40),
    _case("tiny", True, 4), _case("tiny", False, 16),
])


class _HalfTP:
    """Stands in for parallel.TensorParallel: rank 0 of 2, collectives that do nothing (only the launches are looked at)."""
    world = 2

    def k_range(self, K):
        return 0, K // 2

    channel_range = k_range

    def all_reduce(self, t):
        return t

    def all_gather_channels(self, t, n):
        return t


@functools.lru_cache(maxsize=None)
def _model(width):
    from qspec_amd.model import QuarotLlamaConfig, QuarotLlamaForCausalLM
    if WIDTHS[width] is None:
        from test_model_gpu import tiny_cfg
        cfg = tiny_cfg()
    else:
        H, I, nh, nkv, theta = WIDTHS[width]
        cfg = QuarotLlamaConfig(H, I, nh, nkv, 2, 1024, 1e-5, theta, 512, width + "-2layer")
    return QuarotLlamaForCausalLM(cfg, DEV).init_synthetic(seed=4, lm_head_std=0.05)


def _named(model, s, inp, kv):
    md = inp["md"]
    named = {k: v for k, v in vars(s).items() if isinstance(v, torch.Tensor)}
    named.update(cos_sin_cache=model.cos_sin_cache, embed_tokens=model.embed_tokens, had_rem_dim=model.had_rem_dim,
                 head_had=model.head_had, input_ids=inp["ids_t"], positions=inp["pos_t"], slot_mapping=md.slot_mapping,
                 block_tables=md.block_tables, ctx_lens=md.ctx_lens, q_start=md.q_start)
    for i, layer in enumerate(model.layers):
        for proj in ("qkv_proj", "o_proj", "gate_up", "down_proj"):
            lin = getattr(layer, proj)
            named[f"layers[{i}].{proj}.weight"], named[f"layers[{i}].{proj}.scales"] = lin.weight, lin.weight_scales
        named[f"kv[{i}].k"], named[f"kv[{i}].v"] = kv[i]
    return [(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size(), name) for name, t in named.items() if t is not None]


def _label(ptr, named):
    from qspec_amd import ops
    spans = named + [(w.data_ptr(), w.data_ptr() + w.numel() * w.element_size(), "ws." + key[0])
                     for key, w in ops._workspaces.items()]
    return next((f"{name}+{ptr - lo}" for lo, hi, name in spans if lo <= ptr < hi), "?")


def trace(name):
    """(last_forward_form, [launch, ...]) of the case's one forward call."""
    from qspec_amd import ops
    from qspec_amd.model import Scratch
    from test_model_gpu import make_inputs
    c = CASES[name]
    model = _model(c.width)
    q_len = 1 if c.draft else 4
    B = c.T // q_len
    ctx_lens = [33 + (37 * i) % 240 for i in range(B)]        # below max_position_embeddings, three context splits from B = 3
    inp = make_inputs(model, np.random.default_rng(7), ctx_lens, q_len)
    kv = inp["kv_t"]
    if c.kv8:   # bytes below 0x78: finite e4m3 values
        kv = [tuple(torch.randint(0, 120, k.shape, dtype=torch.uint8, device=DEV) for k in pair) for pair in kv]
    s = Scratch(model.config, c.T, B, q_len, inp["n_splits"], DEV)
    named, launches, call = _named(model, s, inp, kv), [], ops._call

    def recorder(entry, *args):   # (an int from 2^32 up is a pointer: no scalar of these shapes comes near, no device address is below)
        shown = [repr(a) if isinstance(a, float) else _label(a, named) if isinstance(a, int) and a >= 1 << 32 else str(a)
                 for a in args[:-1]]
        launches.append(f"{entry}({','.join(shown)})")
        call(entry, *args)
    try:   # the knobs are class attributes: shadow them on the (cached) model for this call only
        for k, v in c.knobs.items():
            setattr(model, k, v)
        model.tp = _HalfTP() if c.tp else None
        ops._call = recorder
        model.forward(inp["ids_t"], inp["pos_t"], kv, inp["md"], s, w4a4=c.draft, kv_scales=KV8_SCALES if c.kv8 else None)
        torch.cuda.synchronize()
    finally:
        ops._call, model.tp = call, None
        for k in c.knobs:
            vars(model).pop(k, None)
    return model.last_forward_form, launches


if __name__ == "__main__":   # python tests/forward_trace.py [FILE]: write the traces of this tree
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    out = {name: dict(zip(("form", "launches"), trace(name))) for name in CASES}
    with open(sys.argv[1] if len(sys.argv) > 1 else GOLDEN, "w") as f:   # one case per line: a changed launch is one changed line
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in out.items()) + "\n}\n")
    print({name: (rec["form"], len(rec["launches"])) for name, rec in out.items()})
    sys.exit([l for rec in out.values() for l in rec["launches"] if "?" in l] or 0)
