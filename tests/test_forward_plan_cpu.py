"""QuarotLlamaForCausalLM._plan on the host (no GPU): the launch-form decision table of forward().  The library is a stub
whose `*_supported` / `*_slices` answers come from a table the test controls (everything "yes" unless a test says otherwise),
Scratch lives on the CPU.  tiny_cfg() has 8 heads, which no tile form takes (they need 32 / 64 heads or a table factor), so
the fragment-major and two-tile rows use a 32-head layer and a 40-head one beside it."""
import functools
from types import SimpleNamespace

import pytest
import torch

from qspec_amd import _lib, ops
from qspec_amd.model import AttentionMetadata, QuarotLlamaConfig, QuarotLlamaForCausalLM, Scratch
from test_model_gpu import tiny_cfg

SUPPORTED = ("qkv_rope_linear", "heads_hadamard_mix_merged_spread", "heads_hadamard_merged_spread", "ln_linear_s4s4",
             "rowwise_scaled_linear_s4s4_residual", "rowwise_scaled_linear_s4s4_residual_hq", "w4a16_act_layout",
             "w4a16_act_layout32", "mlp_hadamard_act_layout")
SLICES = {"rowwise_scaled_linear_s4s4_partial_slices": 2, "w4a16_linear_partial_slices": 4, "w4a16_linear_partial_slices_xp32": 4}
SIZES = {"paged_attention_workspace_bytes": 64, "xwg_workspace_bytes": 256, "ln_linear_workspace_bytes": 192,
         "w4a16_workspace_bytes": 96}
KNOBS = ("BIG_M", "VERIFY_FUSE_MAX_M", "FUSE_LN_MAX_M", "VERIFY_O_SLICES", "FUSE_LN", "HADAMARD_QUANT_IN_OPROJ",
         "ACT_FRAGMENT_MAJOR", "XP32_DOWN_SLICES", "TILED_PARTIAL_IN_NORM", "MERGE_IN_HADAMARD", "DOWN_K_SLICES")
DEFAULTS = dict(zip(KNOBS, (64, 16, 4, 0, True, True, True, True, True, True, True)))


@pytest.fixture
def lib(monkeypatch):
    """The stub library: lib.table[name] is the answer of query `name` (a value, or a function of the query's arguments),
    lib.asked the names of the queries made so far.  The knobs are pinned to their defaults, whatever the environment says."""
    table = {**{q + "_supported": True for q in SUPPORTED}, **SLICES}
    asked = []

    def query(name):
        def f(*args):
            asked.append(name)
            v = table[name]
            return v(*args) if callable(v) else v
        return f
    fns = {"qspec_" + name: query(name) for name in table}
    fns.update({"qspec_" + name: (lambda *a, v=v: v) for name, v in SIZES.items()})
    stub = SimpleNamespace(**fns)
    monkeypatch.setattr(_lib, "load", lambda: stub)
    for k, v in DEFAULTS.items():
        monkeypatch.setattr(QuarotLlamaForCausalLM, k, v)
    return SimpleNamespace(table=table, asked=asked)


@functools.lru_cache(maxsize=None)
def _model(kind):
    cfg = {"tiny": tiny_cfg,                                                                          # 8 heads: generic transform
           "h32": lambda: QuarotLlamaConfig(4096, 3584, 32, 8, 2, 1024, 1e-5, 10000.0, 512, "h32"),   # 32 heads of 128
           "h40": lambda: QuarotLlamaConfig(5120, 3584, 40, 40, 2, 1024, 1e-5, 10000.0, 512, "h40"),  # table factor (had40)
           "d64": lambda: QuarotLlamaConfig(2048, 3584, 32, 4, 2, 1024, 1e-5, 10000.0, 512, "d64")}[kind]()   # head size 64
    return QuarotLlamaForCausalLM(cfg, "cpu")


class _HalfTP:
    world = 2

    def k_range(self, K):
        return 0, K // 2

    channel_range = k_range

    def all_reduce(self, t):
        return t

    def all_gather_channels(self, t, n):
        return t


def plan(kind, T, w4a4, n_splits=3, scratch_T=None, tp=False, **knobs):
    model = _model(kind)
    s = Scratch(model.config, scratch_T or T, 4, 4, n_splits, "cpu")
    old = dict(model.__dict__)
    try:
        model.__dict__.update(knobs, tp=_HalfTP() if tp else None)
        return model._plan(T, w4a4, n_splits, s)
    finally:
        model.__dict__.clear()
        model.__dict__.update(old)


def flags(p):
    return {k for k in ("fuse", "ln_fused", "hq", "xp", "xp32", "tp_on") if getattr(p, k)}


def slices(p):
    return p.S_down, p.S_mlp, p.S_o, p.S32


# ------------------------------------------------------------------ every form, all queries "yes"

@pytest.mark.parametrize("kind,heads", [("h32", "merged"), ("h40", "mix_merged")])
def test_every_form_is_chosen_when_its_queries_say_yes(lib, kind, heads):
    cases = {   # (w4a4, T): form, flags, (S_down, S_mlp, S_o, S32)
        (True, 4): ("fused", {"fuse", "ln_fused", "hq"}, (0, 0, 0, 0)),
        (True, 8): ("fused", {"fuse"}, (0, 0, 0, 0)),              # above FUSE_LN_MAX_M: separate norms
        (True, 32): ("fused", {"fuse"}, (2, 0, 0, 0)),             # int32 K slices (Scratch has down_ipart at 17..32 tokens)
        (True, 100): ("fused", {"fuse"}, (0, 0, 0, 0)),
        (False, 16): ("fragment-major", {"fuse", "xp"}, (0, 4, 0, 0)),
        (False, 32): ("two-tile", {"xp32"}, (0, 4, 0, 4)),
        (False, 48): ("unfused", set(), (0, 4, 4, 0)),             # M-tiled kernel, partials finished in the norms
        (False, 300): ("unfused", set(), (0, 0, 0, 0)),            # no down_part above 256 tokens
    }
    for (w4a4, T), (form, on, S) in cases.items():
        p = plan(kind, T, w4a4)
        assert (p.form, flags(p), slices(p), p.heads, p.w4a4) == (form, on, S, heads, w4a4), (w4a4, T)


def test_eight_heads_take_the_generic_transform_and_no_tile_form(lib):
    for T, form in ((16, "fused"), (32, "unfused")):
        p = plan("tiny", T, False)
        assert (p.form, p.heads, p.xp, p.xp32) == (form, "generic", False, False)
    p = plan("tiny", 4, True)   # the spread transform of the draft pass is the library's to refuse, not the plan's
    assert (p.form, flags(p), p.heads) == ("fused", {"fuse", "ln_fused", "hq"}, "generic")


def test_head_size_64_fuses_on_the_streaming_shapes_only(lib):
    assert [plan("d64", T, True).form for T in (4, 32, 33, 40)] == ["fused", "fused", "unfused", "unfused"]
    assert [plan("d64", T, False).form for T in (8, 16, 17, 40)] == ["fused", "fused", "unfused", "unfused"]
    assert plan("d64", 8, False).heads == "merged" and not plan("d64", 16, False).xp   # tiles are for head size 128
    lib.table["qkv_rope_linear_supported"] = False
    assert plan("d64", 4, True).form == plan("d64", 8, False).form == "unfused"
    assert flags(plan("d64", 4, True)) == set()   # and with it the LN-fused form, which needs the fused epilogues


def test_neither_pass_picks_a_form_of_the_other(lib):
    for kind in ("tiny", "h32", "h40", "d64"):
        for T in (1, 4, 8, 16, 17, 32, 33, 48, 64, 65, 256, 300):
            d, v = plan(kind, T, True), plan(kind, T, False)
            assert not (d.xp or d.xp32 or d.tp_on) and d.form in ("fused", "unfused") and slices(d)[1:] == (0, 0, 0), (kind, T)
            assert not (v.ln_fused or v.hq) and v.S_down == 0, (kind, T)
            assert plan(kind, T, True, tp=True) == d, (kind, T)   # tensor parallelism is the verify pass's


# ------------------------------------------------------------------ one "no" at a time

NO_TILE = [dict(query="w4a16_act_layout_supported"), dict(query="mlp_hadamard_act_layout_supported"),
           dict(ACT_FRAGMENT_MAJOR=False), dict(MERGE_IN_HADAMARD=False), dict(n_splits=65), dict(VERIFY_O_SLICES=2),
           dict(scratch_T=40), dict(query="w4a16_linear_partial_slices", answer=8)]


def _one_no(lib, kind, T, w4a4, query=None, answer=False, **kw):
    if query is not None:
        lib.table[query] = answer
    return plan(kind, T, w4a4, **kw)


@pytest.mark.parametrize("no", NO_TILE, ids=str)
def test_fragment_major_falls_back_to_fused(lib, no):
    p = _one_no(lib, "h32", 16, False, **no)
    assert (p.form, flags(p), p.S32) == ("fused", {"fuse"}, 0)
    if no == dict(VERIFY_O_SLICES=2):
        assert p.S_o == 2
    else:
        assert p.S_o == 0 and p.S_mlp == (0 if no.get("answer") == 8 else 4)


def test_fragment_major_needs_the_layout_at_each_gemm_width(lib):
    H, I, seen = 4096, 3584, []
    lib.table["w4a16_act_layout_supported"] = lambda M, K: seen.append(K) or True
    assert plan("h32", 16, False).xp and seen == [H, H, I // 4]        # hidden, q_size, one K slice of down_proj
    lib.table["w4a16_linear_partial_slices"] = 0
    del seen[:]
    assert plan("h32", 16, False).xp and seen == [H, H, I]
    for width in (H, I):
        lib.table["w4a16_act_layout_supported"] = lambda M, K, width=width: K != width
        assert plan("h32", 16, False).form == "fused"
    lib.table.update(w4a16_act_layout_supported=True, heads_hadamard_mix_merged_spread_supported=False)
    assert plan("h32", 16, False).xp and plan("h40", 16, False).form == "fused"   # a table factor needs the spread transform


@pytest.mark.parametrize("no", [dict(query="w4a16_act_layout32_supported"), dict(ACT_FRAGMENT_MAJOR=False), dict(n_splits=65),
                                dict(MERGE_IN_HADAMARD=False), dict(scratch_T=40)], ids=str)
def test_two_tile_falls_back_to_unfused(lib, no):
    p = _one_no(lib, "h32", 32, False, **no)
    assert (p.form, flags(p), slices(p)) == ("unfused", set(), (0, 4, 4, 0))   # the M-tiled kernel's own K slices


@pytest.mark.parametrize("no", [dict(XP32_DOWN_SLICES=False), dict(query="mlp_hadamard_act_layout_supported"),
                                dict(query="w4a16_linear_partial_slices_xp32", answer=0),
                                dict(query="w4a16_linear_partial_slices_xp32", answer=1),
                                dict(query="w4a16_linear_partial_slices_xp32", answer=9)], ids=str)
def test_two_tile_down_proj_without_its_slices_is_the_m_tiled_launch(lib, no):
    p = _one_no(lib, "h32", 32, False, **no)
    assert (p.form, flags(p), slices(p)) == ("two-tile", {"xp32"}, (0, 4, 0, 0))


@pytest.mark.parametrize("no", [dict(query="ln_linear_s4s4_supported"), dict(query="rowwise_scaled_linear_s4s4_residual_supported"),
                                dict(FUSE_LN=False), dict(FUSE_LN_MAX_M=0)], ids=str)
def test_ln_fused_falls_back_to_fused_with_separate_norms(lib, no):
    p = _one_no(lib, "h32", 4, True, **no)
    assert (p.form, flags(p), slices(p)) == ("fused", {"fuse"}, (0, 0, 0, 0))


@pytest.mark.parametrize("kind,no", [("h32", dict(HADAMARD_QUANT_IN_OPROJ=False)), ("h32", dict(MERGE_IN_HADAMARD=False)),
                                     ("h32", dict(n_splits=65)), ("h32", dict(query="heads_hadamard_merged_spread_supported")),
                                     ("h40", dict(query="heads_hadamard_mix_merged_spread_supported")),
                                     ("h32", dict(query="rowwise_scaled_linear_s4s4_residual_hq_supported"))], ids=str)
def test_hq_falls_back_to_the_quantising_head_transform(lib, kind, no):
    p = _one_no(lib, kind, 4, True, **no)
    assert (p.form, flags(p)) == ("fused", {"fuse", "ln_fused"})
    merges = not ({"MERGE_IN_HADAMARD", "n_splits"} & set(no)) and no.get("query") != "heads_hadamard_mix_merged_spread_supported"
    assert p.heads == (("merged" if kind == "h32" else "mix_merged") if merges else "generic")


def test_slice_counts_that_mean_the_plain_launch(lib):
    """0 or 1 slices, a count the buffer has no room for, or the knob off: S = 0.  (One fp32 slice of the verify down_proj
    is a sliced launch, as it has been: ops.w4a16_linear_partial_slices answers 0 for "use w4a16_linear".)"""
    for answer, want in ((0, 0), (1, 0), (2, 2), (3, 3)):
        lib.table["rowwise_scaled_linear_s4s4_partial_slices"] = answer
        assert plan("h32", 32, True).S_down == want
    assert plan("h32", 32, True, DOWN_K_SLICES=False).S_down == 0 and plan("h32", 16, True).S_down == 0
    for answer, at16, at48, o48 in ((0, 0, 0, 0), (1, 1, 1, 0), (4, 4, 4, 4), (8, 0, 8, 8), (9, 0, 0, 0)):
        lib.table["w4a16_linear_partial_slices"] = answer
        assert plan("tiny", 16, False).S_mlp == at16 and slices(plan("tiny", 48, False)) == (0, at48, o48, 0)
    lib.table["w4a16_linear_partial_slices"] = 4
    assert slices(plan("tiny", 48, False, TILED_PARTIAL_IN_NORM=False)) == (0, 0, 0, 0)
    assert slices(plan("tiny", 16, False, TILED_PARTIAL_IN_NORM=False)) == (0, 4, 0, 0)
    assert [plan("tiny", 16, False, VERIFY_O_SLICES=n).S_o for n in (0, 1, 2, 4)] == [0, 0, 2, 4]
    assert plan("tiny", 48, False, VERIFY_O_SLICES=2).S_o == 4   # the knob is for <= 16 tokens


def test_tensor_parallel_verify_never_takes_a_tile_form(lib):
    for T, form, on in ((8, "fused", {"fuse", "tp_on"}), (16, "fused", {"fuse", "tp_on"}), (32, "fused", {"fuse", "tp_on"}),
                        (48, "unfused", set())):
        p = plan("h32", T, False, tp=True)
        assert (p.form, flags(p), p.S32) == (form, on, 0), T
        assert (p.S_mlp, p.S_o) == ((0, 0) if p.tp_on else (4, 4))   # the shards hand over one fp32 partial of their own
    model = _model("h32")
    model.tp = SimpleNamespace(world=2, shard_layers=False)   # replicated layers (vocab-parallel lm_head only)
    try:
        assert model._plan(16, False, 3, Scratch(model.config, 16, 4, 4, 3, "cpu")).form == "fragment-major"
    finally:
        model.tp = None


# ------------------------------------------------------------------ the layer loop asks nothing

@pytest.mark.parametrize("kind,w4a4,T,form", [("tiny", True, 4, "fused"), ("tiny", False, 16, "fused"), ("h32", True, 32, "fused"),
                                              ("h32", False, 16, "fragment-major"), ("h32", False, 32, "two-tile"),
                                              ("h40", False, 48, "unfused"), ("d64", False, 40, "unfused")])
def test_forward_asks_what_one_plan_asks_and_nothing_in_the_layer_loop(lib, monkeypatch, kind, w4a4, T, form):
    """A whole forward() over launches that do nothing: the queries it makes are those of ONE _plan() call, all of them
    before the first launch."""
    model = _model(kind)
    launches = []
    monkeypatch.setattr(ops, "_call", lambda name, *args: launches.append((name, len(lib.asked))))
    monkeypatch.setattr(ops, "_chk", lambda t, name, dtype=None: t.data_ptr())
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(ops, "_stream_id", lambda device: 7)
    monkeypatch.setattr(ops, "_device_index", lambda device: 0)
    monkeypatch.setattr(ops, "_workspaces", {})
    q_len = 1 if w4a4 else 4
    B = T // q_len
    s = Scratch(model.config, T, B, q_len, 3, "cpu")
    model._plan(T, w4a4, 3, s)
    one_plan = list(lib.asked)
    del lib.asked[:]
    i32, i64 = torch.int32, torch.int64
    md = AttentionMetadata(torch.zeros(T, dtype=i64), torch.zeros(B, 4, dtype=i32), torch.full((B,), 40, dtype=i32),
                           torch.arange(B + 1, dtype=i32) * q_len, q_len, 3)
    cfg = model.config
    kv = [(torch.zeros(4, 16, cfg.num_key_value_heads, cfg.head_dim, dtype=torch.float16),) * 2 for _ in model.layers]
    out = model.forward(torch.zeros(T, dtype=i64), torch.zeros(T, dtype=i64), kv, md, s, w4a4=w4a4)
    assert out.data_ptr() == s.normed.data_ptr() and model.last_forward_form == form
    assert lib.asked == one_plan and one_plan
    assert len(launches) > 2 * 7 and all(asked == len(one_plan) for _, asked in launches)
