"""FP8 (e4m3) KV cache on the GPU (include/qspec_hip.h, "FP8 KV cache").

1. Writers: every `_kv8` write form against the reference quantiser applied to what the fp16 form stores, byte for byte.
2. Readers: ops.paged_attention over quantised caches against the float64 reference on the DEQUANTISED caches (the exact e4m3
   values times the scale), over the whole case matrix of tests/attn_cases.py, at the fp16 tests' own bar.
3. Engine and worker with kv_cache_dtype = "fp8".

The oracle engine (oracle/) models the fp16 cache only, so section 3 checks the discrete logic of a cycle exactly (as
test_model_gpu._engine_cycle_check does) and the relations between this project's own paths, not distributions against it."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import attn_cases as A
from test_kernels_gpu import assert_close_1e3, rand_hidden, rand_w4

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CNT_SLOTS = 4096   # attention_common.cuh: QS_ATT_CNT_SLOTS
SENTINEL = 0x5A
SCALES = [(1.0, 1.0), (0.75, 1.5)]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    from qspec_amd import ops as o
    return o


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def quantise(x, scale):
    """The reference quantiser: fp16 values (numpy or CPU tensor) -> torch.float8_e4m3fn on the CPU."""
    x = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x.cpu()
    return torch.clamp(x.float() * np.float32(1) / np.float32(scale), -448, 448).to(torch.float8_e4m3fn)


def dequantise_f64(q8, scale):
    return q8.float().double().numpy() * float(np.float32(scale))


# ------------------------------------------------------------------ 1. writers

def _inputs(oracle, rng, M, nq, nkv, d, K, bs, n_slots, skip):
    N = (nq + 2 * nkv) * d
    slots_np = rng.permutation(n_slots)[:M].astype(np.int64)
    if M > 1:
        slots_np[skip % M] = -1
    return SimpleNamespace(
        M=M, N=N, K=K, nq=nq, nkv=nkv, d=d, bs=bs, n_slots=n_slots, slots_np=slots_np, slots=dev(slots_np),
        wq=dev(oracle.pack_i4(rand_w4(rng, N, K))), ws=dev((rng.random(N) * 0.01 + 0.001).astype(np.float16)),
        cs=dev(oracle.make_cos_sin_cache(d, 2048, 10000.0)), pos=dev(rng.integers(0, 2048, M).astype(np.int64)))


def _form_rope_kv_write(ops, oracle, rng, nq, nkv, d, bs):
    i = _inputs(oracle, rng, 6, nq, nkv, d, 128, bs, 128, 3)
    qkv = rng.standard_normal((6, i.N)).astype(np.float16)

    def run(kc, vc, **kw):
        t = dev(qkv)
        ops.rope_kv_write(i.pos, t, i.cs, kc, vc, i.slots, nq, nkv, d, **kw)
        return t
    return i, run


def _form_reshape_and_cache(ops, oracle, rng, nq, nkv, d, bs):
    i = _inputs(oracle, rng, 6, nq, nkv, d, 128, bs, 128, 3)
    qkv = dev(rng.standard_normal((6, i.N)).astype(np.float16))

    def run(kc, vc, **kw):
        ops.reshape_and_cache_flash(qkv[:, nq * d:(nq + nkv) * d].view(6, nkv, d), qkv[:, (nq + nkv) * d:].view(6, nkv, d), kc, vc,
                                    i.slots, **kw)
        return qkv
    return i, run


def _form_qkv_rope_linear(ops, oracle, rng, M, w4a4, nq, nkv, d, K, bs, xp=False):
    i = _inputs(oracle, rng, M, nq, nkv, d, K, bs, 1024, 0)
    if w4a4:
        x, xs = dev(oracle.pack_i4(rand_w4(rng, M, K))), dev((rng.random(M) * 0.1 + 0.01).astype(np.float16))
    elif xp:
        from test_act_layout_gpu import to_tile
        x, xs = to_tile(rand_hidden(rng, M, K)), None
    else:
        x, xs = dev(rand_hidden(rng, M, K)), None
    assert ops.qkv_rope_linear_supported(w4a4, M, i.N, K, d)

    def run(kc, vc, **kw):
        out = torch.empty(M, i.N, dtype=torch.float16, device=DEV)
        ops.qkv_rope_linear(x, xs, i.wq, i.ws, out, i.pos, i.cs, kc, vc, i.slots, nq, nkv, d, xp=xp, tokens=M, **kw)
        return out
    return i, run


def _form_xp32(ops, oracle, rng, M, nq, nkv, K):
    from test_act_layout_gpu import to_tiles32
    i = _inputs(oracle, rng, M, nq, nkv, 128, K, 16, 1024, 1)
    x = to_tiles32(rand_hidden(rng, M, K))
    assert ops.w4a16_act_layout32_supported(M, i.N, K)

    def run(kc, vc, **kw):
        out = torch.empty(M, i.N, dtype=torch.float16, device=DEV)
        ops.qkv_rope_linear_xp32(x, i.wq, i.ws, out, i.pos, i.cs, kc, vc, i.slots, nq, nkv, 128, M, **kw)
        return out
    return i, run


def _form_ln_qkv(ops, oracle, rng, M, nq, nkv, K):
    i = _inputs(oracle, rng, M, nq, nkv, 128, K, 16, 1024, 1)
    hidden, delta = dev(rand_hidden(rng, M, K)), dev(rand_hidden(rng, M, K, 0.3))
    assert ops.ln_linear_s4s4_supported(M, i.N, K)

    def run(kc, vc, **kw):
        out = torch.empty(M, i.N, dtype=torch.float16, device=DEV)
        h1 = torch.empty_like(hidden)
        ops.ln_qkv_rope_linear(hidden, delta, h1, 1e-5, i.wq, i.ws, out, i.pos, i.cs, kc, vc, i.slots, nq, nkv, 128, **kw)
        return torch.cat([out, h1], dim=1)   # the residual stream is an output of the launch too
    return i, run


L8B, TINY, TL = (32, 8, 128, 4096), (8, 2, 128, 1024), (32, 4, 64, 2048)   # (nq, nkv, d, K): Llama-3-8B width, the tests' tiny, TinyLlama
WRITER_FORMS = {
    "rope_kv_write-8b-bs16": lambda o, orc, r: _form_rope_kv_write(o, orc, r, 32, 8, 128, 16),
    "rope_kv_write-8b-bs8": lambda o, orc, r: _form_rope_kv_write(o, orc, r, 32, 8, 128, 8),
    "rope_kv_write-d64-bs32": lambda o, orc, r: _form_rope_kv_write(o, orc, r, 32, 4, 64, 32),
    "reshape_and_cache_flash-8b-bs16": lambda o, orc, r: _form_reshape_and_cache(o, orc, r, 32, 8, 128, 16),
    "reshape_and_cache_flash-d64-bs8": lambda o, orc, r: _form_reshape_and_cache(o, orc, r, 32, 4, 64, 8),
    # QKV_ROPE_SHAPES of test_kernels_gpu (streaming kernels up to 16 / 32 rows, the first-generation kernels of gemm.hip above)
    "s4s4-M4-tiny": lambda o, orc, r: _form_qkv_rope_linear(o, orc, r, 4, True, *TINY, 16),
    "s4s4-M16-tiny-bs8": lambda o, orc, r: _form_qkv_rope_linear(o, orc, r, 16, True, *TINY, 8),
    "s4s4-M33-tiny": lambda o, orc, r: _form_qkv_rope_linear(o, orc, r, 33, True, *TINY, 16),
    "s4s4-M4-8b": lambda o, orc, r: _form_qkv_rope_linear(o, orc, r, 4, True, *L8B, 16),
    "s4s4-M32-8b": lambda o, orc, r: _form_qkv_rope_linear(o, orc, r, 32, True, *L8B, 16),
    "s4s4-M4-d64": lambda o, orc, r: _form_qkv_rope_linear(o, orc, r, 4, True, *TL, 32),
    "w4a16-M16-tiny": lambda o, orc, r: _form_qkv_rope_linear(o, orc, r, 16, False, *TINY, 16),
    "w4a16-M24-tiny": lambda o, orc, r: _form_qkv_rope_linear(o, orc, r, 24, False, *TINY, 16),
    "w4a16-M16-8b": lambda o, orc, r: _form_qkv_rope_linear(o, orc, r, 16, False, *L8B, 16),
    "w4a16-M16-d64": lambda o, orc, r: _form_qkv_rope_linear(o, orc, r, 16, False, *TL, 16),
    "w4a16_xp-M8-8b": lambda o, orc, r: _form_qkv_rope_linear(o, orc, r, 8, False, *L8B, 16, xp=True),
    "w4a16_xp-M16-8b": lambda o, orc, r: _form_qkv_rope_linear(o, orc, r, 16, False, *L8B, 16, xp=True),
    "w4a16_xp32-M32-8b": lambda o, orc, r: _form_xp32(o, orc, r, 32, 32, 8, 4096),
    "w4a16_xp32-M19": lambda o, orc, r: _form_xp32(o, orc, r, 19, 16, 2, 8192),
    "ln_s4s4-M4-8b": lambda o, orc, r: _form_ln_qkv(o, orc, r, 4, 32, 8, 4096),
    "ln_s4s4-M16-small": lambda o, orc, r: _form_ln_qkv(o, orc, r, 16, 4, 2, 2048),
}


@pytest.mark.parametrize("scales", SCALES, ids=lambda s: f"k{s[0]}-v{s[1]}")
@pytest.mark.parametrize("form", list(WRITER_FORMS))
def test_kv8_writers_store_the_reference_quantisers_bytes(ops, oracle, form, scales):
    rng = np.random.default_rng(sum(map(ord, form)))
    i, run = WRITER_FORMS[form](ops, oracle, rng)
    shape = (i.n_slots // i.bs, i.bs, i.nkv, i.d)
    kc16 = torch.zeros(shape, dtype=torch.float16, device=DEV); vc16 = torch.zeros_like(kc16)
    out16 = run(kc16, vc16).clone()
    kc8 = torch.full(shape, SENTINEL, dtype=torch.uint8, device=DEV); vc8 = torch.full_like(kc8, SENTINEL)
    out8 = run(kc8, vc8, k_scale=scales[0], v_scale=scales[1])
    torch.cuda.synchronize()
    assert torch.equal(out8.view(torch.int16), out16.view(torch.int16))     # the fp16 outputs: bit-identical
    written = np.zeros(i.n_slots, bool)
    written[i.slots_np[i.slots_np >= 0]] = True
    assert written.sum() == (i.slots_np >= 0).sum() >= 1
    for c16, c8, s in ((kc16, kc8, scales[0]), (vc16, vc8, scales[1])):
        got = host(c8).reshape(i.n_slots, -1)
        ref = quantise(host(c16), s).view(torch.uint8).numpy().reshape(i.n_slots, -1)
        assert np.abs(host(c16).reshape(i.n_slots, -1)[written].astype(np.float32)).max() > 0   # the fp16 form did write there
        assert np.array_equal(got[written], ref[written])                   # no tolerance
        assert (got[~written] == SENTINEL).all()                            # slot -1 and every other slot: untouched


def test_kv8_accepts_float8_tensors_and_refuses_scales_on_fp16(ops, oracle):
    rng = np.random.default_rng(5)
    i, run = _form_rope_kv_write(ops, oracle, rng, 8, 2, 128, 16)
    shape = (i.n_slots // i.bs, i.bs, i.nkv, i.d)
    a = torch.zeros(shape, dtype=torch.uint8, device=DEV); b = torch.zeros_like(a)
    run(a, b, k_scale=0.5, v_scale=2.0)
    a8 = torch.zeros(shape, dtype=torch.uint8, device=DEV).view(torch.float8_e4m3fn); b8 = torch.zeros_like(a8)
    run(a8, b8, k_scale=0.5, v_scale=2.0)
    torch.cuda.synchronize()
    assert torch.equal(a8.view(torch.uint8), a) and torch.equal(b8.view(torch.uint8), b)
    h = torch.zeros(shape, dtype=torch.float16, device=DEV)
    with pytest.raises(ValueError):
        run(h, torch.zeros_like(h), k_scale=0.5, v_scale=1.0)


# ------------------------------------------------------------------ 2. readers

def _launch(ops, case, d, kc8, vc8, scales, out):
    T = case.T
    ws = torch.zeros(ops.paged_attention_workspace_bytes(T, case.nq, case.d, case.n_splits), dtype=torch.uint8, device=DEV)
    ops.paged_attention(dev(d["qkv"]), d["row"], kc8.view(torch.uint8).to(DEV), vc8.view(torch.uint8).to(DEV), dev(d["bt"]),
                        dev(d["ctx"]), dev(d["q_start"]), T, case.q_len, case.nq, d["scale"], case.n_splits, ws, out,
                        k_scale=scales[0], v_scale=scales[1])
    return ws


def _partials(case, ws):
    T, nq, hd = case.T, case.nq, case.d
    S = A.generic_splits(case.n_splits) if hd != 128 else case.n_splits
    f = host(ws.view(torch.float32))
    o = f[CNT_SLOTS:CNT_SLOTS + T * nq * S * hd].reshape(T, nq, S, hd)
    ml = f[CNT_SLOTS + T * nq * S * hd:CNT_SLOTS + T * nq * S * (hd + 2)].reshape(T, nq, S, 2)
    return o, ml


def _quantised_case(case, scales):
    """The case's data with K / V quantised.  Scales (1, 1): the fp16 values themselves.  Other scales: x / scale is
    quantised, so the dequantised data keep the magnitude of the fp16 cases.  Poison saturates to +-448, NaN stays NaN."""
    d = A.build(case)
    kc8, vc8 = quantise(d["kc"], scales[0]), quantise(d["vc"], scales[1])
    assert torch.isnan(kc8.float()[torch.from_numpy(d["nan_blocks"]).long()]).all()
    pk = np.abs(kc8.float().numpy())[d["poisoned"]]
    assert pk.size == 0 or (pk == 448.0).all()
    ref = A.ref_attention_f64(d["q"], dequantise_f64(kc8, scales[0]), dequantise_f64(vc8, scales[1]), d["bt"], d["ctx"],
                              d["q_start"], d["scale"])
    return d, kc8, vc8, ref


def _one_case_per_required_row():
    chosen, seen = [], set()
    for c in A.GPU_CASES:
        new = (A.path_rows(c) & A.REQUIRED_ROWS) - seen - {"generic"}
        if new:
            chosen.append(c)
            seen |= new
    assert seen == A.REQUIRED_ROWS - {"generic"}
    return chosen


READER_CASES = [(c, SCALES[0]) for c in A.GPU_CASES] + [(c, SCALES[1]) for c in _one_case_per_required_row()]


def test_fp8_reader_cases_reach_every_instantiation():
    rows = set()
    for c, _ in READER_CASES:
        if A.kernel_path(c) != "generic":
            rows |= A.path_rows(c)
    assert rows >= A.REQUIRED_ROWS - {"generic"}, sorted((A.REQUIRED_ROWS - {"generic"}) - rows)
    rows_scaled = set().union(*(A.path_rows(c) for c, s in READER_CASES if s != SCALES[0]))
    assert rows_scaled >= A.REQUIRED_ROWS - {"generic"}


@pytest.mark.parametrize("case,scales", READER_CASES, ids=[f"{c.id}-k{s[0]}v{s[1]}" for c, s in READER_CASES])
def test_paged_attention_fp8_matches_float64_on_the_dequantised_cache(ops, case, scales):
    d, kc8, vc8, ref = _quantised_case(case, scales)
    T = case.T
    if A.kernel_path(case) == "generic":   # odd head sizes: the scalar kernel has no fp8 form and says so
        out = torch.empty(T, case.nq * case.d, dtype=torch.float16, device=DEV)
        with pytest.raises(RuntimeError):
            _launch(ops, case, d, kc8, vc8, scales, out)
        return
    if case.merged:
        out = torch.full((T + 1, case.nq * case.d), 7.0, dtype=torch.float16, device=DEV)
        _launch(ops, case, d, kc8, vc8, scales, out[:T])
        assert_close_1e3(host(out[:T]), ref)
        assert torch.all(out[T] == 7.0)   # guard row
    else:
        o, ml = _partials(case, _launch(ops, case, d, kc8, vc8, scales, None))
        assert np.isfinite(o).all() and not np.isnan(ml).any()
        assert_close_1e3(A.merge_partials_f64(o, ml).reshape(T, -1), ref)


CONSUMER_CASES = [
    ("merged", A.make_case((300, 1100, 5, 2049), 4, A.H32, 16, "sink", 8, False, 6000, sink_last=True), SCALES[1]),
    ("merged", A.make_case((17, 8191), 1, A.H64, 16, "peaked", 16, False, 6005), SCALES[0]),
    ("spread", A.make_case((37, 600, 1500, 9), 1, A.H32, 16, "sink", 8, False, 6100, sink_last=True), SCALES[1]),
    ("mix", A.make_case((300, 77, 1200), 1, A.H40, 16, "sink", 3, False, 6200, sink_last=True), SCALES[1]),
]


@pytest.mark.parametrize("form,case,scales", CONSUMER_CASES, ids=[f"{f}-{c.id}-k{s[0]}" for f, c, s in CONSUMER_CASES])
def test_fp8_partials_through_the_head_transform_match_float64(ops, oracle, form, case, scales):
    """The partials carry v_scale: the unchanged consumers give the head transform of the float64 attention."""
    from qspec_amd import hadamard_tables
    d, kc8, vc8, ref = _quantised_case(case, scales)
    had_scale = oracle.rsqrt_scale(case.nq)
    hadK, K = hadamard_tables.get_hadK(case.nq)
    r16 = ref.astype(np.float16)
    ref_h = (oracle.heads_hadamard(r16, case.nq, had_scale) if K == 1
             else oracle.heads_hadamard(r16, case.nq, had_scale, hadK.numpy().astype(np.float16), K))
    ws = _launch(ops, case, d, kc8, vc8, scales, None)
    T, nq, hd, S = case.T, case.nq, case.d, case.n_splits
    out = torch.full((T + 1, nq * hd), 7.0, dtype=torch.float16, device=DEV)
    if form == "merged":
        ops.heads_hadamard_merged(ws, T, S, T, nq, hd, had_scale, out_f16=out[:T])
    elif form == "spread":
        assert ops.heads_hadamard_merged_spread_supported(T, nq, hd)
        pam = torch.full((T, 8), -1.0, dtype=torch.float32, device=DEV)
        ops.heads_hadamard_merged_spread(ws, T, S, T, nq, hd, had_scale, out[:T], pam)
    else:
        assert K > 1 and ops.heads_hadamard_mix_merged_spread_supported(T, nq, hd, K)
        ops.heads_hadamard_mix_merged_spread(ws, T, S, T, nq, hd, hadK.to(torch.float16).to(DEV), K, had_scale, out[:T])
    assert_close_1e3(host(out[:T]), ref_h)
    assert torch.all(out[T] == 7.0)


# ------------------------------------------------------------------ 3. engine and worker

def tiny_cfg():
    from qspec_amd.model import QuarotLlamaConfig
    return QuarotLlamaConfig(1024, 3584, 8, 2, 2, 2048, 1e-5, 10000.0, 512, "tiny")


def wide_cfg():
    """Llama-3-8B width (32 x 128 heads, 8 kv heads, H 4096, I 14336), two layers."""
    from qspec_amd.model import QuarotLlamaConfig
    return QuarotLlamaConfig(4096, 14336, 32, 8, 2, 2048, 1e-5, 500000.0, 512, "8b-width")


@pytest.fixture(scope="module")
def models():
    from qspec_amd.model import QuarotLlamaForCausalLM
    built = {}

    def get(name):
        if name not in built:
            cfg = tiny_cfg() if name == "tiny" else wide_cfg()
            built[name] = QuarotLlamaForCausalLM(cfg, DEV).init_synthetic(seed=1, lm_head_std=0.05)
        return built[name]
    return get


KV_SCALES = [(0.75, 1.5), (1.0, 2.0)]


@pytest.mark.parametrize("width", ["tiny", "8b"])
def test_fp8_graph_replay_equals_eager(models, width):
    from qspec_amd.spec_decode import QSpecEngine
    model = models(width)
    rng = np.random.default_rng(3)
    prompts = [rng.integers(0, model.config.vocab_size, n).tolist() for n in (20, 31, 8, 50)]
    outs = []
    for use_graph in (False, True):
        eng = QSpecEngine(model, 3, 4, max_model_len=256, block_size=16, max_new_tokens=64, use_graph=use_graph, seed=5,
                          kv_cache_dtype="fp8", kv_scales=KV_SCALES)
        assert model.kv_scales is None and eng.kv_scales == KV_SCALES   # the scales live on the engine, not the shared model
        assert all(k.dtype == torch.uint8 and v.dtype == torch.uint8 for k, v in eng.kv_caches)
        eng.add_sequences(prompts)
        for _ in range(6):
            eng.step()
        outs.append((eng.generated(), eng.metrics(), [(k.clone(), v.clone()) for k, v in eng.kv_caches]))
    assert outs[0][0] == outs[1][0] and outs[0][1] == outs[1][1]
    assert all(len(g) >= 7 for g in outs[0][0])
    for (ka, va), (kb, vb) in zip(outs[0][2], outs[1][2]):
        assert torch.equal(ka, kb) and torch.equal(va, vb)
    assert any(int(k.max()) > 0 for k, _ in outs[0][2])   # the byte caches were written


@pytest.mark.parametrize("width,k,B,block_size", [("tiny", 3, 4, 16), ("tiny", 3, 4, 8), ("8b", 5, 4, 16)])
def test_fp8_engine_cycle_invariants(models, oracle, width, k, B, block_size):
    """The discrete part of test_model_gpu._engine_cycle_check with an fp8 cache: given the GPU's own distributions and the
    injected draws, accept mask, recovered ids, output layout, counters, sequence state and the verify pass's tokens,
    positions and slots are exact."""
    from qspec_amd.spec_decode import QSpecEngine
    model = models(width)
    rng = np.random.default_rng(11)
    V, bs = model.config.vocab_size, block_size
    prompts = [rng.integers(0, V, n).tolist() for n in (20, 31, 8, 50)[:B]]
    eng = QSpecEngine(model, k, B, max_model_len=256, block_size=bs, max_new_tokens=64, use_graph=False, seed=0,
                      kv_cache_dtype="fp8")
    eng.add_sequences(prompts)
    gen = [[int(t)] for t in eng.last_token.tolist()]
    counters = np.zeros(3, np.int64)
    for cyc in range(3):
        U = rng.random((B, k)).astype(np.float32)
        E = rng.exponential(1.0, (B, k, V)).astype(np.float32)
        eng.inject_uniform, eng.inject_exponential = torch.from_numpy(U).to(DEV), torch.from_numpy(E).to(DEV)
        L0 = eng.seq_lens.cpu().numpy().copy()
        eng.step()
        torch.cuda.synchronize()
        d_ids = eng.draft_ids_kb.t().cpu().numpy()
        d_probs = eng.draft_probs_kbv.transpose(0, 1).cpu().numpy()
        t_probs, t_toks = eng.target_probs.cpu().numpy(), eng.target_tokens.cpu().numpy()
        assert np.isfinite(d_probs).all() and np.isfinite(t_probs).all()
        out = eng.out_tokens.cpu().numpy()
        o_out, o_acc, o_rec, c = oracle.rejection_sample(t_probs, t_toks[:, k], d_probs, d_ids, U, E)
        assert np.array_equal(out, o_out), cyc
        assert np.array_equal(eng.accepted.cpu().numpy().astype(bool), o_acc), cyc
        assert np.array_equal(eng.recovered.cpu().numpy()[~o_acc], o_rec[~o_acc]), cyc
        counters += np.array(c)
        n_emit = (out != -1).sum(1)
        assert (n_emit >= 1).all() and np.array_equal(eng.seq_lens.cpu().numpy(), L0 + n_emit)
        for b in range(B):
            em = [int(t) for t in out[b] if t != -1]
            assert out[b, :len(em)].tolist() == em
            gen[b].extend(em)
            assert int(eng.last_token[b]) == em[-1]
        vt = eng.v_tokens.view(B, k + 1).cpu().numpy()
        assert np.array_equal(vt[:, 1:], d_ids)
        pos = eng.v_pos.view(B, k + 1).cpu().numpy()
        assert np.array_equal(pos, (L0 - 1)[:, None] + np.arange(k + 1)[None])
        bt = eng.block_tables.cpu().numpy()
        exp_slots = np.take_along_axis(bt, (pos // bs).astype(np.int64), 1).astype(np.int64) * bs + pos % bs
        assert np.array_equal(eng.v_slots.view(B, k + 1).cpu().numpy(), exp_slots)
    assert eng.generated() == gen
    m = eng.metrics()
    assert [m.accepted_tokens, m.emitted_tokens, m.draft_tokens] == counters.tolist()


@pytest.mark.parametrize("w4a4,ctx_lens,q_len", [(True, [40, 130, 7, 260], 1), (False, [40, 130, 9, 260], 4)])
def test_fp8_fused_forward_equals_modulewise(models, w4a4, ctx_lens, q_len):
    """The relation test_model_gpu.test_fused_forward_equals_modulewise asserts for the fp16 cache: bit for bit, outputs
    and caches (both paths quantise the same fp16 K / V values and read the same bytes)."""
    from test_model_gpu import make_inputs
    from qspec_amd.model import Scratch
    tiny = models("tiny")
    rng = np.random.default_rng(0)
    inp = make_inputs(tiny, rng, ctx_lens, q_len)
    s = Scratch(tiny.config, inp["T"], len(ctx_lens), q_len, inp["n_splits"], DEV)
    kv8 = [(quantise(k, ks).view(torch.uint8).to(DEV), quantise(v, vs).view(torch.uint8).to(DEV))
           for (k, v), (ks, vs) in zip(inp["kv_np"], KV_SCALES)]
    kv_a = [(k.clone(), v.clone()) for k, v in kv8]
    kv_b = [(k.clone(), v.clone()) for k, v in kv8]
    a = tiny.forward(inp["ids_t"], inp["pos_t"], kv_a, inp["md"], s, w4a4=w4a4, kv_scales=KV_SCALES).clone()
    b = tiny.forward_modulewise(inp["ids_t"], inp["pos_t"], kv_b, inp["md"], w4a4=w4a4, kv_scales=KV_SCALES)
    torch.cuda.synchronize()
    assert torch.isfinite(a.float()).all()
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    for (ka, va), (kb, vb), (k0, _) in zip(kv_a, kv_b, kv8):
        assert torch.equal(ka, kb) and torch.equal(va, vb)
        assert not torch.equal(ka, k0)   # the new tokens' slots were written


def _vllm_config(cache_dtype):
    hf = SimpleNamespace(model_type="llama_quarot", hidden_size=1024, intermediate_size=3584, num_attention_heads=8,
                         num_key_value_heads=2, num_hidden_layers=2, vocab_size=2048, rms_norm_eps=1e-5,
                         rope_theta=10000.0, max_position_embeddings=512)
    return SimpleNamespace(
        model_config=SimpleNamespace(hf_config=hf, max_model_len=256, model="/nonexistent", seed=0, max_logprobs=5),
        cache_config=SimpleNamespace(block_size=16, gpu_memory_utilization=0.5, swap_space_bytes=1 << 30, cache_dtype=cache_dtype),
        scheduler_config=SimpleNamespace(max_num_seqs=4, max_num_batched_tokens=1024),
        parallel_config=SimpleNamespace(tensor_parallel_size=1, pipeline_parallel_size=1),
        load_config=SimpleNamespace(load_format="dummy"),
        speculative_config=SimpleNamespace(num_speculative_tokens=3, speculative_disable_by_batch_size=None,
                                           disable_log_stats=True, disable_logprobs=True,
                                           draft_token_acceptance_method="rejection_sampler",
                                           speculative_disable_mqa_scorer=False))


def test_fp8_worker_from_vllm_config(models):
    from qspec_amd.spec_decode import ExecuteModelRequest, SequenceGroupMetadata, create_spec_worker
    from qspec_amd.spec_decode.worker import SequenceData
    tiny = models("tiny")
    rng = np.random.default_rng(4)
    probe_vals = {}

    def worker(cache_dtype):
        w = create_spec_worker(vllm_config=_vllm_config(cache_dtype), local_rank=0, rank=0, is_driver_worker=True, device=DEV,
                               model=tiny)
        w.init_device()
        if not probe_vals:                       # one profiled run; both workers size their cache from the same figures
            probe_vals["v"] = w._profile_memory()
        w._memory_probe = lambda: probe_vals["v"]
        return w
    w16, w = worker("auto"), worker("fp8")
    nb16, ncpu16 = w16.determine_num_available_blocks()
    nb, ncpu = w.determine_num_available_blocks()
    assert nb16 > 64 and nb in (2 * nb16, 2 * nb16 + 1) and ncpu == 2 * ncpu16
    w.initialize_cache(64, 0)
    eng = w.engine
    assert eng.kv_cache_dtype == "fp8" and all(k.dtype == torch.uint8 and v.dtype == torch.uint8 for k, v in eng.kv_caches)
    assert eng.kv_caches[0][0].shape == (64, 16, 2, 128)
    # prompts, then speculative steps: r1's context (14 tokens) crosses the block boundary at 16 during them
    sg = [SequenceGroupMetadata(f"r{i}", True, {i: SequenceData(rng.integers(0, 2048, 13 + i).tolist())}) for i in range(4)]
    out = w.execute_model(ExecuteModelRequest(sg, num_lookahead_slots=0))
    assert len(out) == 1 and len(out[0].outputs) == 4 and all(0 <= t < 2048 for t in out[0].token_ids())
    for s in sg:
        s.is_prompt = False
    total = np.zeros(4, np.int64)
    for _ in range(3):
        outs = w.execute_model(ExecuteModelRequest(sg, num_lookahead_slots=3))
        assert 1 <= len(outs) <= 4
        toks = np.array([o.token_ids() for o in outs]).T            # [B, steps]
        assert (toks[:, 0] >= 0).all() and (toks < 2048).all()
        for row in toks.tolist():                                    # -1 only as a suffix
            seen = False
            for t in row:
                assert not (seen and t != -1)
                seen = seen or t == -1
        total += (toks >= 0).sum(1)
    assert (eng.seq_lens.cpu().numpy() > 16).all()                   # every context crossed its first block boundary
    # r0 finishes, its slot is freed and reused by a new request
    outs = w.execute_model(ExecuteModelRequest(sg[1:], num_lookahead_slots=3, finished_requests_ids=["r0"]))
    assert "r0" not in w._slots and 1 <= len(outs) <= 4
    new = SequenceGroupMetadata("r9", True, {9: SequenceData(rng.integers(0, 2048, 21).tolist())})
    out = w.execute_model(ExecuteModelRequest([new], num_lookahead_slots=0))
    assert len(out) == 1 and 0 <= out[0].token_ids()[0] < 2048
    assert w._slots["r9"] == 0
    new.is_prompt = False
    outs = w.execute_model(ExecuteModelRequest([new] + sg[1:], num_lookahead_slots=3))
    assert 1 <= len(outs) <= 4 and all(0 <= t < 2048 for t in outs[0].token_ids())
    torch.cuda.synchronize()
    assert eng._len_ub == eng.seq_lens.tolist()
    assert w.execute_model(None) == []
