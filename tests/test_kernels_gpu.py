"""Parity of every HIP kernel (through the C ABI) against the CPU oracle on the same seeded inputs.

Bar: bit-exact for every integer / byte / index output and for fp16 outputs whose arithmetic is fully
specified (norm, quant, Hadamard, RoPE, W4A4 epilogue); tolerance 1e-3 (north_star) for outputs that
contain an fp32 accumulation whose order the hardware fixes (W4A16 / fp16 GEMM through MFMA, attention).
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


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


def bits(a):
    return np.ascontiguousarray(a).view(np.uint16)


def rand_hidden(rng, T, H, scale=1.0):
    x = rng.standard_normal((T, H)) * scale
    x[:, rng.integers(0, H, 8)] *= 20.0  # a few outlier channels, as in real LLM activations
    return x.astype(np.float16)


# ------------------------------------------------------------------ norm / quant

@pytest.mark.parametrize("T,H", [(1, 4096), (4, 4096), (16, 4096), (192, 4096), (3, 2048), (2, 5120), (5, 8192)])
def test_ln_quant_i4_bit_exact(ops, oracle, T, H):
    rng = np.random.default_rng(T * 131 + H)
    x = rand_hidden(rng, T, H)
    q0, s0, sum0 = oracle.ln_quant_i4(x, 1e-5)
    q = torch.empty(T, H // 2, dtype=torch.int8, device=DEV)
    s = torch.empty(T, dtype=torch.float16, device=DEV)
    isum = torch.empty(T, dtype=torch.float16, device=DEV)
    ops.rms_norm_general_fuse_sum_i4(q, dev(x), isum, s, 1e-5, True)
    assert np.array_equal(host(q), q0)
    assert np.array_equal(bits(host(s)), bits(s0))
    assert np.array_equal(bits(host(isum)), bits(sum0))


def test_ln_quant_edge_rows(ops, oracle):
    H = 4096
    x = np.zeros((5, H), np.float16)
    x[1] = 3.0
    x[2, ::2], x[2, 1::2] = 1.0, -1.0
    x[3, 0] = 100.0
    x[4] = np.float16(6e-8)  # subnormals
    q0, s0, _ = oracle.ln_quant_i4(x, 1e-5)
    q = torch.empty(5, H // 2, dtype=torch.int8, device=DEV)
    s = torch.empty(5, dtype=torch.float16, device=DEV)
    ops.rms_norm_general_fuse_sum_i4(q, dev(x), None, s, 1e-5)
    assert np.array_equal(host(q), q0) and np.array_equal(bits(host(s)), bits(s0))


@pytest.mark.parametrize("T,H", [(4, 4096), (16, 4096), (3, 2048)])
def test_ln_fp16_and_fused_residual_bit_exact(ops, oracle, T, H):
    rng = np.random.default_rng(7)
    x, d = rand_hidden(rng, T, H), rand_hidden(rng, T, H, 0.3)
    out = torch.empty(T, H, dtype=torch.float16, device=DEV)
    ops.rms_norm_general_fuse_sum_fp16(out, dev(x), 1e-5)
    assert np.array_equal(bits(host(out)), bits(oracle.ln_fp16(x, 1e-5)))
    hid = oracle.add_f16(x, d)
    hidden_out = torch.empty_like(out)
    ops.add_rms_norm_fp16(out, hidden_out, dev(x), dev(d), 1e-5)
    assert np.array_equal(bits(host(hidden_out)), bits(hid))
    assert np.array_equal(bits(host(out)), bits(oracle.ln_fp16(hid, 1e-5)))
    q = torch.empty(T, H // 2, dtype=torch.int8, device=DEV)
    s = torch.empty(T, dtype=torch.float16, device=DEV)
    ops.add_rms_norm_i4(q, s, hidden_out, dev(x), dev(d), 1e-5)
    q0, s0, _ = oracle.ln_quant_i4(hid, 1e-5)
    assert np.array_equal(host(q), q0) and np.array_equal(bits(host(s)), bits(s0))


@pytest.mark.parametrize("T,K", [(4, 4096), (4, 14336), (16, 14336), (3, 250), (2, 5632)])
def test_fuse_sym_quant_bit_exact(ops, oracle, T, K):
    rng = np.random.default_rng(K)
    x = rand_hidden(rng, T, K)
    x[0] = 0  # all-zero row: 0/0 -> NaN -> 0
    q0, s0 = oracle.rowabsmax_quant_i4(x, 1.0)
    q = torch.empty(T, K // 2, dtype=torch.int8, device=DEV)
    s = torch.empty(T, dtype=torch.float16, device=DEV)
    ops.fuse_sym_quant(dev(x), s, q, 1.0)
    assert np.array_equal(host(q), q0) and np.array_equal(bits(host(s)), bits(s0))
    q0, s0 = oracle.rowabsmax_quant_i4(x, 0.9)
    ops.fuse_sym_quant(dev(x), s, q, 0.9)
    assert np.array_equal(host(q), q0) and np.array_equal(bits(host(s)), bits(s0))


def test_fuse_sym_quant_reference_fixture_bit_exact(ops, golden_dir):
    """a3 on the GPU against the REFERENCE's Python statement (sym_quant + pack_i4 run on CPU by tests/golden/make_golden.py:
    sym_quant_w4a16.npz), not against the oracle: packed bytes and scales bit for bit."""
    g = np.load(os.path.join(golden_dir, "sym_quant_w4a16.npz"))
    for idx in range(int(g["sq_cases"])):
        x, clip = g[f"sq{idx}_x"], float(g[f"sq{idx}_clip"])
        T, K = x.shape
        q = torch.empty(T, K // 2, dtype=torch.int8, device=DEV)
        s = torch.empty(T, dtype=torch.float16, device=DEV)
        ops.fuse_sym_quant(dev(x), s, q, clip)
        assert np.array_equal(bits(host(s)), bits(g[f"sq{idx}_scale"])), idx
        assert np.array_equal(host(q).view(np.uint8), g[f"sq{idx}_q"].view(np.uint8)), idx


def test_w4a16_reference_fixture(ops, golden_dir):
    """a6 on the GPU against the reference's Python statement of forward_w4a16 (unpack_i4 * scales -> fp16 weight, fp32-
    accumulate matmul; sym_quant_w4a16.npz).  Same bars as the oracle holds against that fixture (test_oracle_golden.py): the
    reference form rounds s * w to fp16, the kernels (like the oracle) scale the sum -- >= 97 % within 1e-3, max 2.5e-3; and
    the kernels are within 1e-3 of the exact sum_k x (s w)."""
    g = np.load(os.path.join(golden_dir, "sym_quant_w4a16.npz"))
    for idx in range(int(g["wa_cases"])):
        x, wq, ws = g[f"wa{idx}_x"], g[f"wa{idx}_wq"], g[f"wa{idx}_ws"]
        M, N = x.shape[0], wq.shape[0]
        out = torch.empty(M, N, dtype=torch.float16, device=DEV)
        ops.w4a16_linear(dev(x), dev(wq), dev(ws), out)
        got = host(out).astype(np.float64)
        ref = g[f"wa{idx}_ref_f32"].astype(np.float64)
        r = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
        assert (r <= 1e-3).mean() >= 0.97 and r.max() <= 2.5e-3, (idx, r.max(), (r > 1e-3).mean())
        w = ((wq.view(np.uint8)[:, :, None] >> np.array([0, 4], np.uint8)) & 0xF).astype(np.int8).reshape(N, -1)
        w = np.where(w >= 8, w - 16, w).astype(np.float64)
        exact = x.astype(np.float64) @ (w * ws.astype(np.float64)[:, None]).T
        assert (np.abs(got - exact) <= 1e-3 * np.maximum(1.0, np.abs(exact))).all(), idx


# ------------------------------------------------------------------ hadamard

@pytest.mark.parametrize("rows,N", [(512, 32), (112, 512), (5, 1024), (3, 8), (2, 4096)])
def test_fwht_bit_exact(ops, oracle, rows, N):
    rng = np.random.default_rng(N)
    x = (rng.standard_normal((rows, N)) * 3).astype(np.float16)
    sc = oracle.rsqrt_scale(N)
    out = ops.fast_hadamard_transform(dev(x), sc)
    assert np.array_equal(bits(host(out)), bits(oracle.fwht(x, sc)))


def test_fwht_golden(ops, golden_dir):
    g = np.load(os.path.join(golden_dir, "hadamard.npz"))
    for n in (32, 512):
        out = ops.fast_hadamard_transform(dev(g[f"x_{n}"].astype(np.float16)), float(np.float32(1) / np.sqrt(np.float32(n))))
        assert np.allclose(host(out).astype(np.float64), g[f"y_{n}"], atol=5e-3, rtol=0)


def test_hadamard_mix_bit_exact(ops, oracle, golden_dir):
    g = np.load(os.path.join(golden_dir, "hadamard.npz"))
    rng = np.random.default_rng(3)
    for K, M in ((28, 512), (108, 128), (12, 64)):
        had = g[f"had{K}"].astype(np.float16)
        y = rng.standard_normal((3, K, M)).astype(np.float16)
        out = torch.empty(3, K, M, dtype=torch.float16, device=DEV)
        ops.hadamard_mix(dev(y), dev(had), out)
        assert np.array_equal(bits(host(out)), bits(oracle.hadk_mix(y, had)))


@pytest.mark.parametrize("T,heads,d", [(4, 32, 128), (16, 32, 128), (3, 64, 128), (2, 32, 64)])
def test_heads_hadamard_bit_exact(ops, oracle, T, heads, d):
    rng = np.random.default_rng(heads + d)
    x = rand_hidden(rng, T, heads * d)
    sc = oracle.rsqrt_scale(heads)
    y0 = oracle.heads_hadamard(x, heads, sc)
    out = torch.empty(T, heads * d, dtype=torch.float16, device=DEV)
    ops.heads_hadamard(dev(x), sc, out_f16=out, heads=heads)
    assert np.array_equal(bits(host(out)), bits(y0))
    q0, s0 = oracle.rowabsmax_quant_i4(y0, 1.0)
    q = torch.empty(T, heads * d // 2, dtype=torch.int8, device=DEV)
    s = torch.empty(T, dtype=torch.float16, device=DEV)
    ops.heads_hadamard(dev(x), sc, q=q, scale=s, heads=heads)
    assert np.array_equal(host(q), q0) and np.array_equal(bits(host(s)), bits(s0))


@pytest.mark.parametrize("T,I,K", [(4, 14336, 28), (16, 14336, 28), (2, 28672, 28), (2, 13824, 108), (3, 1024, 1),
                                   (2, 1536, 12)])
def test_silu_mul_hadamard_bit_exact(ops, oracle, golden_dir, T, I, K):
    g = np.load(os.path.join(golden_dir, "hadamard.npz"))
    rng = np.random.default_rng(I + K)
    gu = rand_hidden(rng, T, 2 * I, 2.0)
    had = g[f"had{K}"].astype(np.float16) if K > 1 else None
    sc = oracle.rsqrt_scale(I)
    z0 = oracle.mlp_hadamard(oracle.silu_mul(gu, I), had, K, sc)
    out = torch.empty(T, I, dtype=torch.float16, device=DEV)
    hd = dev(had) if had is not None else None
    ops.silu_mul_hadamard(dev(gu), hd, K, sc, out_f16=out)
    assert np.array_equal(bits(host(out)), bits(z0))
    q0, s0 = oracle.rowabsmax_quant_i4(z0, 1.0)
    q = torch.empty(T, I // 2, dtype=torch.int8, device=DEV)
    s = torch.empty(T, dtype=torch.float16, device=DEV)
    ops.silu_mul_hadamard(dev(gu), hd, K, sc, q=q, scale=s)
    assert np.array_equal(host(q), q0) and np.array_equal(bits(host(s)), bits(s0))


# ------------------------------------------------------------------ GEMMs

def rand_w4(rng, N, K):
    return rng.integers(-8, 8, (N, K)).astype(np.int8)


@pytest.mark.parametrize("M,N,K", [(1, 64, 128), (4, 6144, 4096), (4, 4096, 14336), (16, 4096, 4096), (32, 512, 4096),
                                   (33, 256, 1408), (67, 64, 1408), (192, 128, 4096), (4, 28672, 4096),
                                   (4, 5120, 13824), (16, 512, 13824), (32, 640, 13824), (32, 5120, 13824), (3, 6144, 14336), (1, 2048, 5632), (4, 2048, 5632)])
def test_w4a4_gemm_bit_exact(ops, oracle, M, N, K):
    rng = np.random.default_rng(M * 7 + N + K)
    xq = oracle.pack_i4(rand_w4(rng, M, K))
    wq = oracle.pack_i4(rand_w4(rng, N, K))
    xs = (rng.random(M) * 0.1 + 0.01).astype(np.float16)
    ws = (rng.random(N) * 0.01 + 0.001).astype(np.float16)
    out = torch.empty(M, N, dtype=torch.float16, device=DEV)
    ops.rowwise_scaled_linear_cutlass_s4s4_unified(dev(xq), dev(xs), dev(wq), dev(ws), None, out)
    assert np.array_equal(bits(host(out)), bits(oracle.gemm_w4a4(xq, xs, wq, ws)))
    if N <= 4096:
        bias = rng.random(N).astype(np.float16)
        ops.rowwise_scaled_linear_cutlass_s4s4_unified(dev(xq), dev(xs), dev(wq), dev(ws), dev(bias), out)
        assert np.array_equal(bits(host(out)), bits(oracle.gemm_w4a4(xq, xs, wq, ws, bias)))


def test_w4a4_gemm_extreme_values(ops, oracle):
    """all -8 x -8 at the longest K: the int32 accumulator (x256 from the nibble widening) must not overflow."""
    M, N, K = 4, 32, 14336
    xq = oracle.pack_i4(np.full((M, K), -8, np.int8))
    wq = oracle.pack_i4(np.full((N, K), -8, np.int8))
    wq[1::2] = oracle.pack_i4(np.full((N // 2, K), 7, np.int8))
    xs = np.full(M, 0.01, np.float16)
    ws = np.full(N, 0.001, np.float16)
    out = torch.empty(M, N, dtype=torch.float16, device=DEV)
    ops.rowwise_scaled_linear_cutlass_s4s4_unified(dev(xq), dev(xs), dev(wq), dev(ws), None, out)
    assert np.array_equal(bits(host(out)), bits(oracle.gemm_w4a4(xq, xs, wq, ws)))


def test_w4a4_gemm_golden(ops, golden_dir):
    """The reference test's formula on its own (M, K) shapes -- committed fixture."""
    g = np.load(os.path.join(golden_dir, "w4a4_gemm.npz"))
    for idx in range(6):
        xq, wq, xs, ws = (g[f"c{idx}_{k}"] for k in ("xq", "wq", "xs", "ws"))
        M, N = xq.shape[0], wq.shape[0]
        out = torch.empty(M, N, dtype=torch.float16, device=DEV)
        ops.rowwise_scaled_linear_cutlass_s4s4_unified(dev(xq), dev(xs), dev(wq), dev(ws), None, out)
        assert np.array_equal(bits(host(out)), bits(g[f"c{idx}_ref_n"])), idx
        ops.rowwise_scaled_linear_cutlass_s4s4_unified(dev(xq), dev(xs), dev(wq), dev(ws), dev(g[f"c{idx}_bias"]), out)
        assert np.array_equal(bits(host(out)), bits(g[f"c{idx}_ref_b"])), idx


def assert_close_1e3(got, ref):
    got, ref = got.astype(np.float64), ref.astype(np.float64)
    tol = 1e-3 * np.maximum(1.0, np.abs(ref))
    bad = ~(np.abs(got - ref) <= tol)   # NaN / inf in either fails (a plain `> tol` lets NaN through)
    assert not bad.any(), (np.abs(got - ref).max(), int(bad.sum()))


@pytest.mark.parametrize("M,N,K", [(1, 64, 128), (16, 6144, 4096), (16, 4096, 14336), (4, 4096, 4096), (24, 512, 4096),
                                   (40, 128, 4096), (4, 2048, 5632), (16, 2048, 5632)])
def test_w4a16_gemm_within_1e3(ops, oracle, M, N, K):
    rng = np.random.default_rng(M + N + K)
    x = rand_hidden(rng, M, K)
    wq = oracle.pack_i4(rand_w4(rng, N, K))
    ws = (rng.random(N) * 0.002 + 0.0005).astype(np.float16)
    out = torch.empty(M, N, dtype=torch.float16, device=DEV)
    ops.w4a16_linear(dev(x), dev(wq), dev(ws), out)
    assert_close_1e3(host(out), oracle.gemm_w4a16(x, wq, ws))


def test_w4a16_exact_on_integer_data(ops, oracle):
    """Small-integer activations make every fp32 partial sum exact, so any k-permutation or lane-map
    error in the MFMA path shows up as a bit mismatch (asymmetric data on purpose)."""
    rng = np.random.default_rng(5)
    M, N, K = 16, 64, 512
    x = rng.integers(-4, 5, (M, K)).astype(np.float16)
    wq = oracle.pack_i4(rand_w4(rng, N, K))
    ws = np.ones(N, np.float16)
    out = torch.empty(M, N, dtype=torch.float16, device=DEV)
    ops.w4a16_linear(dev(x), dev(wq), dev(ws), out)
    assert np.array_equal(bits(host(out)), bits(oracle.gemm_w4a16(x, wq, ws)))


def test_both_views_read_the_same_buffer(ops, oracle):
    """Draft and verify GEMMs take the identical device pointer; neither modifies it."""
    rng = np.random.default_rng(9)
    M, N, K = 4, 256, 4096
    w = dev(oracle.pack_i4(rand_w4(rng, N, K)))
    before = w.clone()
    ws = dev((rng.random(N) * 0.01 + 0.001).astype(np.float16))
    out = torch.empty(M, N, dtype=torch.float16, device=DEV)
    ops.rowwise_scaled_linear_cutlass_s4s4_unified(dev(oracle.pack_i4(rand_w4(rng, M, K))), dev(np.ones(M, np.float16)), w, ws, None, out)
    ops.w4a16_linear(dev(rand_hidden(rng, M, K)), w, ws, out)
    torch.cuda.synchronize()
    assert torch.equal(w, before)


QKV_ROPE_SHAPES = [(4, True, 128), (16, True, 128), (33, True, 128), (16, False, 128), (24, False, 128),
                   (1, True, 64), (4, True, 64), (16, True, 64), (24, True, 64), (4, False, 64), (16, False, 64)]


@pytest.mark.parametrize("M,w4a4,d", QKV_ROPE_SHAPES)
def test_qkv_rope_linear_equals_gemm_then_rope_then_cache(ops, oracle, M, w4a4, d):
    _qkv_rope_linear_check(ops, oracle, M, w4a4, d, 16)


@pytest.mark.parametrize("bs", [8, 32])
@pytest.mark.parametrize("M,w4a4,d", QKV_ROPE_SHAPES)
def test_qkv_rope_linear_equals_gemm_then_rope_then_cache_block_sizes(ops, oracle, M, w4a4, d, bs):
    """The same at vLLM's other common KV block sizes (the same data: 1024 cache slots at every block size)."""
    _qkv_rope_linear_check(ops, oracle, M, w4a4, d, bs)


def _qkv_rope_linear_check(ops, oracle, M, w4a4, d, bs):
    """Fused epilogue == the three reference ops one after the other, bit for bit (same kernels' arithmetic).  Head size 64
    (TinyLlama: 32 + 2 x 4 heads, K = 2048) runs on the streaming kernels only (RoPE pairs (i, i + 32), four tiles per head)."""
    rng = np.random.default_rng(M)
    nq, nkv, K = (8, 2, 1024) if d == 128 else (32, 4, 2048)
    N = (nq + 2 * nkv) * d
    if not ops.qkv_rope_linear_supported(w4a4, M, N, K, d):   # head size 64 beyond the streaming shapes: refused, not mis-computed
        assert d == 64 and M > 16
        with pytest.raises(RuntimeError):
            ops.qkv_rope_linear(dev(oracle.pack_i4(rand_w4(rng, M, K))), dev(np.ones(M, np.float16)), dev(oracle.pack_i4(rand_w4(rng, N, K))),
                                dev(np.ones(N, np.float16)), torch.empty(M, N, dtype=torch.float16, device=DEV),
                                dev(np.zeros(M, np.int64)), dev(oracle.make_cos_sin_cache(d, 64, 10000.0)),
                                torch.zeros(8, bs, nkv, d, dtype=torch.float16, device=DEV), torch.zeros(8, bs, nkv, d, dtype=torch.float16, device=DEV),
                                dev(np.zeros(M, np.int64)), nq, nkv, d)
        return
    wq = dev(oracle.pack_i4(rand_w4(rng, N, K)))
    ws = dev((rng.random(N) * 0.01 + 0.001).astype(np.float16))
    cs = dev(oracle.make_cos_sin_cache(d, 2048, 10000.0))
    pos = dev(rng.integers(0, 2048, M).astype(np.int64))
    slots_np = rng.permutation(1024)[:M].astype(np.int64)   # 1024 slots (and the same data) at every block size
    slots_np[0] = -1
    slots = dev(slots_np)
    if w4a4:
        x, xs = dev(oracle.pack_i4(rand_w4(rng, M, K))), dev((rng.random(M) * 0.1 + 0.01).astype(np.float16))
    else:
        x, xs = dev(rand_hidden(rng, M, K)), None
    ref = torch.empty(M, N, dtype=torch.float16, device=DEV)
    if w4a4:
        ops.rowwise_scaled_linear_cutlass_s4s4_unified(x, xs, wq, ws, None, ref)
    else:
        ops.w4a16_linear(x, wq, ws, ref)
    kc0 = torch.zeros(1024 // bs, bs, nkv, d, dtype=torch.float16, device=DEV); vc0 = torch.zeros_like(kc0)
    ops.rope_kv_write(pos, ref, cs, kc0, vc0, slots, nq, nkv, d)
    out = torch.empty_like(ref)
    kc1 = torch.zeros_like(kc0); vc1 = torch.zeros_like(kc0)
    ops.qkv_rope_linear(x, xs, wq, ws, out, pos, cs, kc1, vc1, slots, nq, nkv, d)
    torch.cuda.synchronize()
    if not w4a4 and M > 16:
        # W4A16 above 16 rows: w4a16_linear is the M-tiled kernel since round 4, the fused-epilogue entry the 2-D kernel of
        # gemm.hip (the engine no longer calls it there): two fp32 summation orders, each within 1e-3 of the oracle
        assert_close_1e3(host(out), host(ref))
        assert_close_1e3(host(kc1), host(kc0))
        assert_close_1e3(host(vc1), host(vc0))
        return
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))
    assert torch.equal(kc1, kc0) and torch.equal(vc1, vc0)


@pytest.mark.parametrize("M,w4a4", [(4, True), (16, True), (40, True), (16, False)])
def test_gate_up_silu_linear_and_mlp_hadamard_equal_unfused(ops, oracle, golden_dir, M, w4a4):
    rng = np.random.default_rng(M + 100)
    I, K = 3584, 1024
    g = np.load(os.path.join(golden_dir, "hadamard.npz"))
    had = dev(g["had28"].astype(np.float16))
    wq = dev(oracle.pack_i4(rand_w4(rng, 2 * I, K)))
    ws = dev((rng.random(2 * I) * 0.01 + 0.001).astype(np.float16))
    if w4a4:
        x, xs = dev(oracle.pack_i4(rand_w4(rng, M, K))), dev((rng.random(M) * 0.1 + 0.01).astype(np.float16))
    else:
        x, xs = dev(rand_hidden(rng, M, K)), None
    gu = torch.empty(M, 2 * I, dtype=torch.float16, device=DEV)
    if w4a4:
        ops.rowwise_scaled_linear_cutlass_s4s4_unified(x, xs, wq, ws, None, gu)
    else:
        ops.w4a16_linear(x, wq, ws, gu)
    ref_act = ops.silu_mul(gu, torch.empty(M, I, dtype=torch.float16, device=DEV))
    act = ops.gate_up_silu_linear(x, xs, wq, ws, torch.empty(M, I, dtype=torch.float16, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(act.view(torch.int16), ref_act.view(torch.int16))
    sc = oracle.rsqrt_scale(I)
    q0 = torch.empty(M, I // 2, dtype=torch.int8, device=DEV); s0 = torch.empty(M, dtype=torch.float16, device=DEV)
    q1 = torch.empty_like(q0); s1 = torch.empty_like(s0)
    ops.silu_mul_hadamard(gu, had, 28, sc, q=q0, scale=s0)
    ops.mlp_hadamard(act, had, 28, sc, q=q1, scale=s1)
    o0 = torch.empty(M, I, dtype=torch.float16, device=DEV); o1 = torch.empty_like(o0)
    ops.silu_mul_hadamard(gu, had, 28, sc, out_f16=o0)
    ops.mlp_hadamard(act, had, 28, sc, out_f16=o1)
    torch.cuda.synchronize()
    assert torch.equal(q0, q1) and torch.equal(s0.view(torch.int16), s1.view(torch.int16))
    assert torch.equal(o0.view(torch.int16), o1.view(torch.int16))


@pytest.mark.parametrize("M,K,with_delta", [(4, 4096, True), (1, 4096, False), (16, 4096, True), (3, 2048, True),
                                            (7, 5120, True), (4, 8192, True), (5, 1024, True)])
@pytest.mark.parametrize("handoff", [False, True])
def test_ln_prologue_gemms_equal_ln_then_gemm(ops, oracle, M, K, with_delta, handoff, monkeypatch):
    """The draft pass's fused launches (residual add + LN + int4 quant in the GEMM prologue) against the separate
    LN kernel (oracle-checked above) followed by the GEMM entry (oracle-checked above): bit for bit, including the
    residual stream written by workgroup 0 and the KV cache."""
    monkeypatch.setattr(ops, "LN_HANDOFF", handoff)   # norm recomputed per workgroup / by producers + hand-off
    monkeypatch.setattr(ops, "LN_HANDOFF_MIN_M", 1)
    rng = np.random.default_rng(M * 7 + K)
    nq, nkv, d, bs = 4, 2, 128, 16
    N = (nq + 2 * nkv) * d
    I = 1792
    hidden = dev(rand_hidden(rng, M, K))
    delta = dev(rand_hidden(rng, M, K, 0.3)) if with_delta else None
    wq = dev(oracle.pack_i4(rand_w4(rng, N, K)))
    ws = dev((rng.random(N) * 0.01 + 0.001).astype(np.float16))
    wg = dev(oracle.pack_i4(rand_w4(rng, 2 * I, K)))
    wgs = dev((rng.random(2 * I) * 0.01 + 0.001).astype(np.float16))
    cs = dev(oracle.make_cos_sin_cache(d, 2048, 10000.0))
    pos = dev(rng.integers(0, 2048, M).astype(np.int64))
    slots_np = rng.permutation(64 * bs)[:M].astype(np.int64)
    if M > 1:
        slots_np[1] = -1
    slots = dev(slots_np)
    # reference: LN kernel, then the GEMM entries on its (q, scale)
    q = torch.empty(M, K // 2, dtype=torch.int8, device=DEV)
    sc = torch.empty(M, dtype=torch.float16, device=DEV)
    h_ref = torch.empty_like(hidden)
    ops.add_rms_norm_i4(q, sc, h_ref, hidden, delta, 1e-5)
    if delta is None:
        h_ref.copy_(hidden)
    qkv_ref = torch.empty(M, N, dtype=torch.float16, device=DEV)
    kc0 = torch.zeros(64, bs, nkv, d, dtype=torch.float16, device=DEV); vc0 = torch.zeros_like(kc0)
    ops.qkv_rope_linear(q, sc, wq, ws, qkv_ref, pos, cs, kc0, vc0, slots, nq, nkv, d)
    act_ref = ops.gate_up_silu_linear(q, sc, wg, wgs, torch.empty(M, I, dtype=torch.float16, device=DEV))
    # fused
    assert ops.ln_linear_s4s4_supported(M, N, K)
    h1 = torch.full_like(hidden, float("nan")); h2 = torch.full_like(hidden, float("nan"))
    qkv = torch.empty_like(qkv_ref)
    kc1 = torch.zeros_like(kc0); vc1 = torch.zeros_like(kc0)
    ops.ln_qkv_rope_linear(hidden, delta, h1, 1e-5, wq, ws, qkv, pos, cs, kc1, vc1, slots, nq, nkv, d)
    act = ops.ln_gate_up_silu_linear(hidden, delta, h2, 1e-5, wg, wgs, torch.empty(M, I, dtype=torch.float16, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(h1.view(torch.int16), h_ref.view(torch.int16))
    assert torch.equal(h2.view(torch.int16), h_ref.view(torch.int16))
    assert torch.equal(qkv.view(torch.int16), qkv_ref.view(torch.int16))
    assert torch.equal(kc1, kc0) and torch.equal(vc1, vc0)
    assert torch.equal(act.view(torch.int16), act_ref.view(torch.int16))


@pytest.mark.parametrize("residual", [False, True], ids=["pure", "residual"])
@pytest.mark.parametrize("M,handoff", [(3, False), (6, False), (6, True)], ids=["split", "unsplit", "handoff"])
@pytest.mark.parametrize("K", [1024, 2048, 4096, 5120, 8192])
def test_ln_prologue_every_dispatch_row(ops, oracle, K, M, handoff, residual, monkeypatch):
    """Every row of the norm-prologue dispatch (gemm_stream_w4a4.hip: stream_form() x QS_LN_SHAPES), bit for bit against
    the separate LN kernel followed by the (q, scale) GEMM entries: each K as the split form (M = 3; K = 8192 has none
    and falls through to the unsplit one), as the unsplit form (M = 6) and with the producer hand-off (M = 6), each as
    the pure norm of hidden_in (no delta, nothing written back) and as the residual form (delta added, stream written
    by workgroup 0).  16 weight rows per tile: 64 qkv and 32 gate_up tiles per launch."""
    monkeypatch.setattr(ops, "LN_HANDOFF", handoff)
    monkeypatch.setattr(ops, "LN_HANDOFF_MIN_M", 1)
    rng = np.random.default_rng(K + 31 * M + 2 * handoff + residual)
    nq, nkv, d, bs, I = 4, 2, 128, 16, 256
    N = (nq + 2 * nkv) * d
    hidden = dev(rand_hidden(rng, M, K))
    delta = dev(rand_hidden(rng, M, K, 0.3)) if residual else None
    wq = dev(oracle.pack_i4(rand_w4(rng, N, K)))
    ws = dev((rng.random(N) * 0.01 + 0.001).astype(np.float16))
    wg = dev(oracle.pack_i4(rand_w4(rng, 2 * I, K)))
    wgs = dev((rng.random(2 * I) * 0.01 + 0.001).astype(np.float16))
    cs = dev(oracle.make_cos_sin_cache(d, 2048, 10000.0))
    pos = dev(rng.integers(0, 2048, M).astype(np.int64))
    slots_np = rng.permutation(64 * bs)[:M].astype(np.int64)
    slots_np[1] = -1
    slots = dev(slots_np)
    # reference: LN kernel, then the GEMM entries on its (q, scale)
    q = torch.empty(M, K // 2, dtype=torch.int8, device=DEV)
    sc = torch.empty(M, dtype=torch.float16, device=DEV)
    h_ref = torch.empty_like(hidden) if residual else None
    ops.add_rms_norm_i4(q, sc, h_ref, hidden, delta, 1e-5)
    qkv_ref = torch.empty(M, N, dtype=torch.float16, device=DEV)
    kc0 = torch.zeros(64, bs, nkv, d, dtype=torch.float16, device=DEV); vc0 = torch.zeros_like(kc0)
    ops.qkv_rope_linear(q, sc, wq, ws, qkv_ref, pos, cs, kc0, vc0, slots, nq, nkv, d)
    act_ref = ops.gate_up_silu_linear(q, sc, wg, wgs, torch.empty(M, I, dtype=torch.float16, device=DEV))
    # fused
    assert ops.ln_linear_s4s4_supported(M, N, K)
    h1 = torch.full_like(hidden, float("nan")) if residual else None
    h2 = torch.full_like(hidden, float("nan")) if residual else None
    qkv = torch.empty_like(qkv_ref)
    kc1 = torch.zeros_like(kc0); vc1 = torch.zeros_like(kc0)
    ops.ln_qkv_rope_linear(hidden, delta, h1, 1e-5, wq, ws, qkv, pos, cs, kc1, vc1, slots, nq, nkv, d)
    act = ops.ln_gate_up_silu_linear(hidden, delta, h2, 1e-5, wg, wgs, torch.empty(M, I, dtype=torch.float16, device=DEV))
    torch.cuda.synchronize()
    if residual:   # (pure norm: nothing is written back)
        assert torch.equal(h1.view(torch.int16), h_ref.view(torch.int16))
        assert torch.equal(h2.view(torch.int16), h_ref.view(torch.int16))
    assert torch.equal(qkv.view(torch.int16), qkv_ref.view(torch.int16))
    assert torch.equal(kc1, kc0) and torch.equal(vc1, vc0)
    assert torch.equal(act.view(torch.int16), act_ref.view(torch.int16))


@pytest.mark.parametrize("handoff", [False, True])
def test_ln_prologue_edge_rows(ops, oracle, handoff, monkeypatch):
    """Edge rows through the fused norm prologue: all-zero (amax floor 1e-6), constant, tiny, near-overflow, exact
    .5 ties, -0.0 -- same bytes as the standalone LN kernel (itself oracle-checked on such rows) + GEMM."""
    monkeypatch.setattr(ops, "LN_HANDOFF", handoff)
    monkeypatch.setattr(ops, "LN_HANDOFF_MIN_M", 1)
    K, I = 4096, 256
    rng = np.random.default_rng(5)
    x = np.zeros((8, K), np.float16)
    x[1] = 3.0
    x[2] = (rng.standard_normal(K) * 1e-4).astype(np.float16)
    x[3] = (rng.standard_normal(K) * 3e4).clip(-6e4, 6e4).astype(np.float16)
    x[4] = np.tile(np.array([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 3.5, -3.5], np.float16), K // 8)
    x[5] = -0.0
    x[6] = rand_hidden(rng, 1, K)[0]
    x[7, ::2] = 1.0
    for delta in (None, dev((rng.standard_normal((8, K)) * 0.01).astype(np.float16))):
        hid = dev(x)
        wg = dev(rng.integers(-128, 128, (2 * I, K // 2)).astype(np.int8)); wgs = dev((rng.random(2 * I) * 0.01 + 0.001).astype(np.float16))
        q = torch.empty(8, K // 2, dtype=torch.int8, device=DEV); sc = torch.empty(8, dtype=torch.float16, device=DEV)
        h0 = torch.empty_like(hid)
        ops.add_rms_norm_i4(q, sc, h0, hid, delta, 1e-5)
        a0 = ops.gate_up_silu_linear(q, sc, wg, wgs, torch.empty(8, I, dtype=torch.float16, device=DEV))
        h1 = torch.empty_like(hid) if delta is not None else None
        a1 = ops.ln_gate_up_silu_linear(hid, delta, h1, 1e-5, wg, wgs, torch.empty(8, I, dtype=torch.float16, device=DEV))
        torch.cuda.synchronize()
        assert torch.equal(a0.view(torch.int16), a1.view(torch.int16))
        if delta is not None:
            assert torch.equal(h0.view(torch.int16), h1.view(torch.int16))


@pytest.mark.parametrize("M", [4, 3, 16])
def test_ln_prologue_full_layer_shapes_with_lds_prefetch(ops, oracle, M, monkeypatch):
    """Llama-3-8B layer shapes: several tiles per workgroup, so the tiles behind the first one are brought into LDS
    by LDS-DMA underneath the norm (gemm_stream_w4a4.hip).  Against the separate LN kernel + the plain GEMM entries."""
    monkeypatch.setattr(ops, "LN_HANDOFF", False)
    rng = np.random.default_rng(M)
    K, nq, nkv, d, bs, I = 4096, 32, 8, 128, 16, 14336
    N = (nq + 2 * nkv) * d
    hidden = dev(rand_hidden(rng, M, K)); delta = dev(rand_hidden(rng, M, K, 0.3))
    wq = dev(rng.integers(-128, 128, (N, K // 2)).astype(np.int8)); ws = dev((rng.random(N) * 0.01 + 0.001).astype(np.float16))
    wg = dev(rng.integers(-128, 128, (2 * I, K // 2)).astype(np.int8)); wgs = dev((rng.random(2 * I) * 0.01 + 0.001).astype(np.float16))
    cs = dev(oracle.make_cos_sin_cache(d, 2048, 500000.0))
    pos = dev(rng.integers(0, 2048, M).astype(np.int64))
    slots = dev(rng.permutation(64 * bs)[:M].astype(np.int64))
    q = torch.empty(M, K // 2, dtype=torch.int8, device=DEV); sc = torch.empty(M, dtype=torch.float16, device=DEV)
    h_ref = torch.empty_like(hidden)
    ops.add_rms_norm_i4(q, sc, h_ref, hidden, delta, 1e-5)
    qkv_ref = torch.empty(M, N, dtype=torch.float16, device=DEV)
    kc0 = torch.zeros(64, bs, nkv, d, dtype=torch.float16, device=DEV); vc0 = torch.zeros_like(kc0)
    ops.qkv_rope_linear(q, sc, wq, ws, qkv_ref, pos, cs, kc0, vc0, slots, nq, nkv, d)
    act_ref = ops.gate_up_silu_linear(q, sc, wg, wgs, torch.empty(M, I, dtype=torch.float16, device=DEV))
    h1 = torch.empty_like(hidden); qkv = torch.empty_like(qkv_ref)
    kc1 = torch.zeros_like(kc0); vc1 = torch.zeros_like(kc0)
    ops.ln_qkv_rope_linear(hidden, delta, h1, 1e-5, wq, ws, qkv, pos, cs, kc1, vc1, slots, nq, nkv, d)
    act = ops.ln_gate_up_silu_linear(hidden, delta, h1, 1e-5, wg, wgs, torch.empty(M, I, dtype=torch.float16, device=DEV))
    torch.cuda.synchronize()
    assert torch.equal(h1.view(torch.int16), h_ref.view(torch.int16))
    assert torch.equal(qkv.view(torch.int16), qkv_ref.view(torch.int16))
    assert torch.equal(kc1, kc0) and torch.equal(vc1, vc0)
    assert torch.equal(act.view(torch.int16), act_ref.view(torch.int16))


@pytest.mark.parametrize("M,N,K", [(4, 4096, 4096), (4, 4096, 14336), (16, 1024, 2048), (3, 512, 1024), (4, 5120, 13824),
                                   (4, 5120, 5120), (1, 2048, 5632), (8, 8192, 28672), (3, 512, 28672)])
def test_s4s4_residual_epilogue_equals_linear_then_add(ops, oracle, M, N, K):
    """hidden = residual + proj_out in the GEMM epilogue == the GEMM entry followed by an fp16 tensor add; also in
    place (resid_out aliasing resid_in), and the delta-less norm prologue == the plain LN kernel + GEMM."""
    rng = np.random.default_rng(M + N + K)
    xq = dev(oracle.pack_i4(rand_w4(rng, M, K))); xs = dev((rng.random(M) * 0.1 + 0.01).astype(np.float16))
    wq = dev(rng.integers(-128, 128, (N, K // 2)).astype(np.int8)); ws = dev((rng.random(N) * 0.01 + 0.001).astype(np.float16))
    resid = dev(rand_hidden(rng, M, N))
    lin = torch.empty(M, N, dtype=torch.float16, device=DEV)
    ops.rowwise_scaled_linear_cutlass_s4s4_unified(xq, xs, wq, ws, None, lin)
    ref = resid + lin                                   # fp16 tensor add: one rounding per element
    out = torch.empty_like(resid)
    ops.rowwise_scaled_linear_s4s4_residual(xq, xs, wq, ws, resid, out)
    inplace = resid.clone()
    ops.rowwise_scaled_linear_s4s4_residual(xq, xs, wq, ws, inplace, inplace)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), ref.view(torch.int16))
    assert torch.equal(inplace.view(torch.int16), ref.view(torch.int16))
    if K in (1024, 2048, 4096):   # norm-only prologue (delta = None, nothing written back)
        I = 256
        hid = dev(rand_hidden(rng, M, K))
        wg = dev(rng.integers(-128, 128, (2 * I, K // 2)).astype(np.int8)); wgs = dev((rng.random(2 * I) * 0.01 + 0.001).astype(np.float16))
        q = torch.empty(M, K // 2, dtype=torch.int8, device=DEV); sc = torch.empty(M, dtype=torch.float16, device=DEV)
        ops.rms_norm_general_fuse_sum_i4(q, hid, None, sc, 1e-5)
        a0 = ops.gate_up_silu_linear(q, sc, wg, wgs, torch.empty(M, I, dtype=torch.float16, device=DEV))
        a1 = ops.ln_gate_up_silu_linear(hid, None, None, 1e-5, wg, wgs, torch.empty(M, I, dtype=torch.float16, device=DEV))
        torch.cuda.synchronize()
        assert torch.equal(a0.view(torch.int16), a1.view(torch.int16))


def test_ln_handoff_stress_back_to_back(ops, oracle, monkeypatch):
    """The fence-free producer -> consumer hand-off of the LN-prologue GEMMs under back-to-back launches with
    different inputs each time (a stale flag or a stale row would reuse the previous launch's activations), at the
    real layer shapes, eagerly and replayed from a hipGraph; every output word is checked."""
    rng = np.random.default_rng(11)
    M, K, I = 4, 4096, 14336
    nin = 6
    hid = [dev(rand_hidden(rng, M, K)) for _ in range(nin)]
    dlt = [dev(rand_hidden(rng, M, K, 0.3)) for _ in range(nin)]
    wg = dev(rng.integers(-128, 128, (2 * I, K // 2)).astype(np.int8))
    wgs = dev((rng.random(2 * I) * 0.01 + 0.001).astype(np.float16))
    hout = torch.empty_like(hid[0])
    monkeypatch.setattr(ops, "LN_HANDOFF_MIN_M", 1)
    ops.LN_HANDOFF = False
    try:
        ref = [ops.ln_gate_up_silu_linear(hid[i], dlt[i], hout, 1e-5, wg, wgs,
                                          torch.empty(M, I, dtype=torch.float16, device=DEV)).clone() for i in range(nin)]
    finally:
        ops.LN_HANDOFF = True
    n = 60
    outs = [torch.empty(M, I, dtype=torch.float16, device=DEV) for _ in range(n)]

    def body():
        for j in range(n):
            ops.ln_gate_up_silu_linear(hid[j % nin], dlt[j % nin], hout, 1e-5, wg, wgs, outs[j])
    body()
    torch.cuda.synchronize()
    for j in range(n):
        assert torch.equal(outs[j].view(torch.int16), ref[j % nin].view(torch.int16)), j
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        body()
    for rep in range(5):
        for o in outs:
            o.zero_()
        g.replay()
        torch.cuda.synchronize()
        for j in range(n):
            assert torch.equal(outs[j].view(torch.int16), ref[j % nin].view(torch.int16)), (rep, j)
    ws = ops.ln_linear_workspace(torch.device(DEV))
    assert int(ws[:128].view(torch.int32).abs().sum().item()) == 0   # flags and ticket counter left at zero


def test_ln_prologue_rejects_aliasing_and_big_m(ops, oracle):
    rng = np.random.default_rng(0)
    K, I = 4096, 64
    hidden = dev(rand_hidden(rng, 4, K))
    wg = dev(oracle.pack_i4(rand_w4(rng, 2 * I, K)))
    wgs = dev(np.ones(2 * I, np.float16))
    with pytest.raises(RuntimeError):
        ops.ln_gate_up_silu_linear(hidden, None, hidden, 1e-5, wg, wgs, torch.empty(4, I, dtype=torch.float16, device=DEV))
    assert not ops.ln_linear_s4s4_supported(17, 128, 4096)
    assert not ops.ln_linear_s4s4_supported(4, 128, 3072)


@pytest.mark.parametrize("M,N,K", [(4, 1000, 4096), (16, 128256, 256), (20, 2048, 2048), (8, 4096, 8192), (16, 1040, 8192), (1, 32, 8192)])
def test_linear_f16_within_1e3(ops, oracle, M, N, K):
    rng = np.random.default_rng(N)
    x = rand_hidden(rng, M, K)
    w = (rng.standard_normal((N, K)) * 0.02).astype(np.float16)
    out = torch.empty(M, N, dtype=torch.float16, device=DEV)
    ops.linear_f16(dev(x), dev(w), out)
    assert_close_1e3(host(out), oracle.gemm_f16(x, w))


def test_dequant_w4(ops, oracle):
    rng = np.random.default_rng(2)
    N, K = 48, 512
    w = rand_w4(rng, N, K)
    ws = (rng.random(N) * 0.01 + 0.001).astype(np.float16)
    out = torch.empty(N, K, dtype=torch.float16, device=DEV)
    ops.dequant_w4(dev(oracle.pack_i4(w)), dev(ws), out)
    ref = (w.astype(np.float32) * ws.astype(np.float32)[:, None]).astype(np.float16)
    assert np.array_equal(bits(host(out)), bits(ref))


# ------------------------------------------------------------------ attention side

def make_paged(rng, n_seqs, ctx_lens, nkv, d, block_size):
    max_blocks = max((c + block_size - 1) // block_size for c in ctx_lens) + 1
    nb = n_seqs * max_blocks + 3
    perm = rng.permutation(nb)[: n_seqs * max_blocks].reshape(n_seqs, max_blocks).astype(np.int32)
    kc = (rng.standard_normal((nb, block_size, nkv, d)) * 0.5).astype(np.float16)
    vc = (rng.standard_normal((nb, block_size, nkv, d)) * 0.5).astype(np.float16)
    return perm, kc, vc


def test_rope_and_cache_write_bit_exact(ops, oracle):
    _rope_and_cache_write_check(ops, oracle, 16)


@pytest.mark.parametrize("bs", [8, 32])
def test_rope_and_cache_write_bit_exact_block_sizes(ops, oracle, bs):
    _rope_and_cache_write_check(ops, oracle, bs)


def _rope_and_cache_write_check(ops, oracle, bs):
    rng = np.random.default_rng(11)
    T, nq, nkv, d = 6, 32, 8, 128
    cs = oracle.make_cos_sin_cache(d, 4096, 500000.0)
    pos = rng.integers(0, 4096, T).astype(np.int64)
    qkv = (rng.standard_normal((T, (nq + 2 * nkv) * d))).astype(np.float16)
    q0, k0 = oracle.rope_neox(pos, qkv[:, : nq * d], qkv[:, nq * d:(nq + nkv) * d], cs, d)
    # standalone ops on strided views of the fused buffer
    t = dev(qkv)
    ops.rotary_embedding(dev(pos), t[:, : nq * d], t[:, nq * d:(nq + nkv) * d], d, dev(cs))
    got = host(t)
    assert np.array_equal(bits(got[:, : nq * d]), bits(q0)) and np.array_equal(bits(got[:, nq * d:(nq + nkv) * d]), bits(k0))
    nb = 128 // bs   # 128 slots at every block size (the last one written below)
    kc = torch.zeros(nb, bs, nkv, d, dtype=torch.float16, device=DEV)
    vc = torch.zeros_like(kc)
    slots = np.array([5, 17, 18, -1, 100, 127], np.int64)
    ops.reshape_and_cache_flash(t[:, nq * d:(nq + nkv) * d].view(T, nkv, d), t[:, (nq + nkv) * d:].view(T, nkv, d), kc, vc, dev(slots))
    kc0 = np.zeros((nb, bs, nkv, d), np.float16)
    vc0 = np.zeros_like(kc0)
    oracle.reshape_and_cache_flash(k0.reshape(T, nkv, d), qkv[:, (nq + nkv) * d:].reshape(T, nkv, d), kc0, vc0, slots)
    assert np.array_equal(bits(host(kc)), bits(kc0)) and np.array_equal(bits(host(vc)), bits(vc0))
    # fused kernel
    t2 = dev(qkv)
    kc.zero_(); vc.zero_()
    ops.rope_kv_write(dev(pos), t2, dev(cs), kc, vc, dev(slots), nq, nkv, d)
    got2 = host(t2)
    assert np.array_equal(bits(got2[:, : (nq + nkv) * d]), bits(got[:, : (nq + nkv) * d]))
    assert np.array_equal(bits(host(kc)), bits(kc0)) and np.array_equal(bits(host(vc)), bits(vc0))


@pytest.mark.parametrize("ctx_lens,q_len", [([37, 128, 129, 500], 1), ([37, 130, 260, 515], 4), ([700], 6), ([5, 9], 4)])
@pytest.mark.parametrize("few_splits", [False, True])
def test_paged_attention_within_1e3(ops, oracle, ctx_lens, q_len, few_splits):
    rng = np.random.default_rng(sum(ctx_lens) + q_len)
    nq, nkv, d, bs = 32, 8, 128, 16
    n_seqs = len(ctx_lens)
    bt, kc, vc = make_paged(rng, n_seqs, ctx_lens, nkv, d, bs)
    T = n_seqs * q_len
    row = (nq + 2 * nkv) * d
    qkv = (rng.standard_normal((T, row)) * 0.5).astype(np.float16)
    q_start = (np.arange(n_seqs + 1) * q_len).astype(np.int32)
    ctx = np.array(ctx_lens, np.int32)
    scale = d ** -0.5
    ref = oracle.paged_attention(qkv[:, : nq * d], kc, vc, bt, ctx, q_start, scale)
    # few_splits: splits longer than 128 keys -> the kernel's inner chunk loop with the running softmax
    n_splits = (1 if max(ctx_lens) < 600 else 2) if few_splits else (max(ctx_lens) + 127) // 128 + 1
    ws = torch.zeros(ops.paged_attention_workspace_bytes(T, nq, d, n_splits), dtype=torch.uint8, device=DEV)
    out = torch.empty(T, nq * d, dtype=torch.float16, device=DEV)
    ops.paged_attention(dev(qkv), row, dev(kc), dev(vc), dev(bt), dev(ctx), dev(q_start), T, q_len, nq, scale,
                        n_splits, ws, out)
    assert_close_1e3(host(out), ref)


# ------------------------------------------------------------------ token side

@pytest.mark.parametrize("ctx_lens,q_len,d,nq,nkv", [([37, 200], 1, 64, 32, 4), ([70, 9, 300], 4, 64, 8, 8), ([50], 3, 96, 4, 2),
                                                     ([2, 600, 1300], 2, 64, 32, 4), ([2100], 1, 64, 8, 4), ([700, 3], 1, 256, 2, 1),
                                                     ([300], 4, 8, 4, 4)])
def test_paged_attention_generic_head_size_within_1e3(ops, oracle, ctx_lens, q_len, d, nq, nkv):
    """Head sizes other than 128 (TinyLlama: 64) take the generic kernel (no context split, no matrix cores): contexts inside
    and beyond the P.V pass's prefetch window (8 rows per thread), one-key rows, 1..32 pieces per row.  (A context holds at
    least q_len keys: a 1-key context under 2 query tokens put the first query at position -1, a row without keys whose
    0/0 NaN -- in the kernel and the oracle alike -- the old bar let through.)"""
    rng = np.random.default_rng(sum(ctx_lens) + d)
    bs = 16
    n_seqs = len(ctx_lens)
    bt, kc, vc = make_paged(rng, n_seqs, ctx_lens, nkv, d, bs)
    T = n_seqs * q_len
    row = (nq + 2 * nkv) * d
    qkv = (rng.standard_normal((T, row)) * 0.5).astype(np.float16)
    q_start = (np.arange(n_seqs + 1) * q_len).astype(np.int32)
    ctx = np.array(ctx_lens, np.int32)
    scale = d ** -0.5
    ref = oracle.paged_attention(qkv[:, : nq * d], kc, vc, bt, ctx, q_start, scale)
    ws = torch.zeros(ops.paged_attention_workspace_bytes(T, nq, d, 1), dtype=torch.uint8, device=DEV)
    out = torch.empty(T, nq * d, dtype=torch.float16, device=DEV)
    ops.paged_attention(dev(qkv), row, dev(kc), dev(vc), dev(bt), dev(ctx), dev(q_start), T, q_len, nq, scale, 1, ws, out)
    assert_close_1e3(host(out), ref)
    # context splits (min(n_splits, 4) of whole 16-key groups; some of them empty for the short sequences) + the merge launch
    for n_splits in (3, 16):
        ws = torch.zeros(ops.paged_attention_workspace_bytes(T, nq, d, n_splits), dtype=torch.uint8, device=DEV)
        out_s = torch.full((T + 1, nq * d), 7.0, dtype=torch.float16, device=DEV)
        ops.paged_attention(dev(qkv), row, dev(kc), dev(vc), dev(bt), dev(ctx), dev(q_start), T, q_len, nq, scale, n_splits, ws, out_s[:T])
        assert_close_1e3(host(out_s[:T]), ref)
        assert torch.all(out_s[T] == 7.0)
        if nq == 32 and d % 8 == 0:   # partials left to the head transform: the bits of merge launch -> heads_hadamard
            had_scale = oracle.rsqrt_scale(nq)
            o0 = torch.empty(T, nq * d, dtype=torch.float16, device=DEV); o1 = torch.empty_like(o0)
            q0 = torch.empty(T, nq * d // 2, dtype=torch.int8, device=DEV); s0 = torch.empty(T, dtype=torch.float16, device=DEV)
            q1 = torch.empty_like(q0); s1 = torch.empty_like(s0)
            ops.heads_hadamard(out_s[:T].contiguous(), had_scale, out_f16=o0, heads=nq)
            ops.heads_hadamard(out_s[:T].contiguous(), had_scale, q=q0, scale=s0, heads=nq)
            ws2 = torch.zeros_like(ws)
            ops.paged_attention(dev(qkv), row, dev(kc), dev(vc), dev(bt), dev(ctx), dev(q_start), T, q_len, nq, scale, n_splits, ws2, None)
            ops.heads_hadamard_merged(ws2, T, n_splits, T, nq, d, had_scale, out_f16=o1)
            ops.heads_hadamard_merged(ws2, T, n_splits, T, nq, d, had_scale, q=q1, scale=s1)
            torch.cuda.synchronize()
            assert torch.equal(o0.view(torch.int16), o1.view(torch.int16))
            assert torch.equal(q0, q1) and torch.equal(s0.view(torch.int16), s1.view(torch.int16))


@pytest.mark.parametrize("ctx_lens,q_len,n_splits", [([37, 128, 129, 500], 1, 8), ([37, 130, 260, 515], 4, 5),
                                                     ([1500], 2, 12), ([5, 9], 4, 3), ([1500, 3000], 1, 4)])
def test_heads_hadamard_merged_equals_attention_merge_then_hadamard(ops, oracle, ctx_lens, q_len, n_splits):
    """Split merge moved from the attention kernel into the head-Hadamard launch: bit-identical outputs (int4 bytes,
    scales, fp16 rows) to the attention kernel merging its own splits followed by the plain head Hadamard."""
    rng = np.random.default_rng(sum(ctx_lens) * 3 + q_len)
    nq, nkv, d, bs = 32, 8, 128, 16
    n_seqs = len(ctx_lens)
    bt, kc, vc = make_paged(rng, n_seqs, ctx_lens, nkv, d, bs)
    T = n_seqs * q_len
    row = (nq + 2 * nkv) * d
    qkv = dev((rng.standard_normal((T, row)) * 0.5).astype(np.float16))
    q_start = dev((np.arange(n_seqs + 1) * q_len).astype(np.int32))
    ctx = dev(np.array(ctx_lens, np.int32))
    sc = d ** -0.5
    had_scale = oracle.rsqrt_scale(nq)
    args = (qkv, row, dev(kc), dev(vc), dev(bt), ctx, q_start, T, q_len, nq, sc, n_splits)
    ws = torch.zeros(ops.paged_attention_workspace_bytes(T, nq, d, n_splits), dtype=torch.uint8, device=DEV)
    attn = torch.empty(T, nq * d, dtype=torch.float16, device=DEV)
    ops.paged_attention(*args, ws, attn)
    q0 = torch.empty(T, nq * d // 2, dtype=torch.int8, device=DEV); s0 = torch.empty(T, dtype=torch.float16, device=DEV)
    o0 = torch.empty(T, nq * d, dtype=torch.float16, device=DEV)
    ops.heads_hadamard(attn, had_scale, q=q0, scale=s0, heads=nq)
    ops.heads_hadamard(attn, had_scale, out_f16=o0, heads=nq)
    ws2 = torch.zeros_like(ws)
    ops.paged_attention(*args, ws2, None)
    q1 = torch.empty_like(q0); s1 = torch.empty_like(s0); o1 = torch.empty_like(o0)
    ops.heads_hadamard_merged(ws2, T, n_splits, T, nq, d, had_scale, q=q1, scale=s1)
    ops.heads_hadamard_merged(ws2, T, n_splits, T, nq, d, had_scale, out_f16=o1)
    torch.cuda.synchronize()
    if bt.shape[1] * bs > 128 * n_splits:
        # splits that may exceed one 128-key chunk: the partials come from the keys-over-waves kernel, whose summation
        # order differs from the chunk kernel that merges in place -- same rows within the attention tolerance
        assert_close_1e3(host(o1), host(o0))
        return
    assert torch.equal(q0, q1) and torch.equal(s0.view(torch.int16), s1.view(torch.int16))
    assert torch.equal(o0.view(torch.int16), o1.view(torch.int16))


@pytest.mark.parametrize("ctx_lens,q_len,n_splits", [([37, 128, 129, 500], 1, 8), ([600, 5, 77], 1, 8), ([600, 5, 20], 1, 8),
                                                     ([37, 130], 2, 5), ([77], 1, 8), ([300, 20], 1, 8), ([900], 3, 8)])
def test_spread_head_hadamard_and_quantiser_in_the_o_proj_prologue(ops, oracle, ctx_lens, q_len, n_splits):
    """Draft pass, T <= 4: merge + head Hadamard spread over 8 workgroups per token (fp16 rows + 8 partial row maxima) and the
    row-absmax quantiser in the prologue of the o_proj launch give the bits of heads_hadamard_merged(q) followed by
    rowwise_scaled_linear_s4s4_residual -- and of the CPU oracle's rowabsmax_quant_i4 -> gemm_w4a4 -> add_f16 on the same
    fp16 rows; an all-zero row included."""
    rng = np.random.default_rng(sum(ctx_lens) * 7 + q_len)
    nq, nkv, d, bs, N = 32, 8, 128, 16, 4096
    n_seqs = len(ctx_lens)
    bt, kc, vc = make_paged(rng, n_seqs, ctx_lens, nkv, d, bs)
    T = n_seqs * q_len
    row = (nq + 2 * nkv) * d
    qkv_h = (rng.standard_normal((T, row)) * 0.5).astype(np.float16)
    vc = np.array(vc)
    if ctx_lens[-1] <= bs * 2:          # the last sequence sees only zero values -> an all-zero attention row
        for b in bt[-1]:
            vc[b] = 0
    qkv = dev(qkv_h)
    q_start = dev((np.arange(n_seqs + 1) * q_len).astype(np.int32))
    ctx = dev(np.array(ctx_lens, np.int32))
    had_scale = oracle.rsqrt_scale(nq)
    ws = torch.zeros(ops.paged_attention_workspace_bytes(T, nq, d, n_splits), dtype=torch.uint8, device=DEV)
    ops.paged_attention(qkv, row, dev(kc), dev(vc), dev(bt), ctx, q_start, T, q_len, nq, d ** -0.5, n_splits, ws, None)
    wq, wsc = rng.integers(-128, 128, (N, nq * d // 2)).astype(np.int8), (rng.random(N) * 0.01 + 0.001).astype(np.float16)
    resid = (rng.standard_normal((T, N))).astype(np.float16)
    # the two-launch form
    q0 = torch.empty(T, nq * d // 2, dtype=torch.int8, device=DEV); s0 = torch.empty(T, dtype=torch.float16, device=DEV)
    o0 = torch.empty(T, nq * d, dtype=torch.float16, device=DEV)
    ops.heads_hadamard_merged(ws, T, n_splits, T, nq, d, had_scale, q=q0, scale=s0)
    ops.heads_hadamard_merged(ws, T, n_splits, T, nq, d, had_scale, out_f16=o0)
    h0 = dev(resid)
    ops.rowwise_scaled_linear_s4s4_residual(q0, s0, dev(wq), dev(wsc), h0, h0)
    # the spread form
    assert ops.heads_hadamard_merged_spread_supported(T, nq, d) and ops.rowwise_scaled_linear_s4s4_residual_hq_supported(T, N, nq * d)
    o1 = torch.empty_like(o0)
    pam = torch.full((T, 8), -1.0, dtype=torch.float32, device=DEV)
    ops.heads_hadamard_merged_spread(ws, T, n_splits, T, nq, d, had_scale, o1, pam)
    h1 = dev(resid)
    ops.rowwise_scaled_linear_s4s4_residual_hq(o1, pam, 1.0, dev(wq), dev(wsc), h1, h1)
    torch.cuda.synchronize()
    assert torch.equal(o0.view(torch.int16), o1.view(torch.int16))
    assert np.array_equal(host(pam).max(axis=1), np.abs(host(o1).astype(np.float32)).max(axis=1))
    assert torch.equal(h0.view(torch.int16), h1.view(torch.int16))
    # and against the oracle on the same fp16 rows
    qo, so = oracle.rowabsmax_quant_i4(host(o1), 1.0)
    ref = oracle.add_f16(resid, oracle.gemm_w4a4(qo, so, wq, wsc))
    assert np.array_equal(bits(host(h1)), bits(ref))


def _attn_partials_ws(ops, T, heads, d, S, o, m, l):
    """A paged_attention workspace holding the given per-split partials: [ticket counters | o [T, heads, S, d] | (m, l)
    [T, heads, S, 2]] fp32 (attention_common.cuh: attn_ws; paged_attention, out = NULL)."""
    total = ops.paged_attention_workspace_bytes(T, heads, d, S) // 4
    cnt = total - T * heads * S * (d + 2)
    ws = torch.zeros(total, dtype=torch.float32, device=DEV)
    ws[cnt:cnt + T * heads * S * d] = dev(np.ascontiguousarray(o, np.float32)).view(-1)
    ml = np.stack([m, l], axis=-1).astype(np.float32)
    ws[cnt + T * heads * S * d:] = dev(ml).view(-1)
    return ws.view(torch.uint8)


@pytest.mark.parametrize("T,heads", [(4, 40), (1, 40), (3, 24), (16, 40), (2, 48)])
def test_spread_table_factor_head_transform_bit_exact_on_given_partials(ops, oracle, T, heads):
    """Head counts with a table factor (Llama-2-13B: 40 heads = had40; 24 = had12 x 2; 48 = had12 x 4): the spread merge +
    FWHT over 2^p + scale + table mix on GIVEN partials.  One split with (m, l) = (0, 1) makes the merge the identity on fp16
    values, so the transform is compared bit for bit with heads_hadamard_mix and with the oracle's heads_hadamard; two splits
    with different maxima are compared with the merge formula in fp64 (the hardware 2^x is ~1 ulp: 1e-3)."""
    from qspec_amd import hadamard_tables
    rng = np.random.default_rng(T * 100 + heads)
    d = 128
    hadK, K = hadamard_tables.get_hadK(heads)
    assert K > 1 and ops.heads_hadamard_mix_merged_spread_supported(T, heads, d, K)
    hk = hadK.to(torch.float16).to(DEV)
    had_scale = oracle.rsqrt_scale(heads)
    attn = (rng.standard_normal((T, heads, d)) * 0.5).astype(np.float16)
    attn[0, :, 5] = 0
    ws = _attn_partials_ws(ops, T, heads, d, 1, attn.astype(np.float32)[:, :, None, :], np.zeros((T, heads, 1)), np.ones((T, heads, 1)))
    o0 = torch.empty(T, heads * d, dtype=torch.float16, device=DEV)
    ops.heads_hadamard_mix(dev(attn), hk, K, had_scale, o0)
    o1 = torch.empty_like(o0); o2 = torch.empty_like(o0)
    pam = torch.full((T, 8), -1.0, dtype=torch.float32, device=DEV)
    ops.heads_hadamard_mix_merged_spread(ws, T, 1, T, heads, d, hk, K, had_scale, o1)
    ops.heads_hadamard_mix_merged_spread(ws, T, 1, T, heads, d, hk, K, had_scale, o2, pam)
    torch.cuda.synchronize()
    assert torch.equal(o0.view(torch.int16), o1.view(torch.int16)) and torch.equal(o0.view(torch.int16), o2.view(torch.int16))
    assert np.array_equal(host(pam).max(axis=1), np.abs(host(o1).astype(np.float32)).max(axis=1))
    ref = oracle.heads_hadamard(attn.reshape(T, heads * d), heads, had_scale, hadK.numpy().astype(np.float16), K)
    assert np.array_equal(bits(host(o1)), bits(ref))
    # two splits: out = sum_s e^(m_s - M) o_s / sum_s e^(m_s - M) l_s
    o = rng.standard_normal((T, heads, 2, d)) * 2.0
    m = rng.standard_normal((T, heads, 2)) * 3.0
    l = rng.random((T, heads, 2)) * 5.0 + 0.5
    m[0, 0, 1] = -np.inf                        # an empty split (a sequence shorter than the split's first key)
    o[0, 0, 1], l[0, 0, 1] = 0.0, 0.0
    ws2 = _attn_partials_ws(ops, T, heads, d, 2, o, m, l)
    wgt = np.exp(m - m.max(axis=2, keepdims=True))
    merged = ((wgt[..., None] * o).sum(axis=2) / (wgt * l).sum(axis=2)[..., None]).astype(np.float16)
    ref2 = oracle.heads_hadamard(merged.reshape(T, heads * d), heads, had_scale, hadK.numpy().astype(np.float16), K)
    ops.heads_hadamard_mix_merged_spread(ws2, T, 2, T, heads, d, hk, K, had_scale, o1)
    assert np.abs(host(o1).astype(np.float64) - ref2.astype(np.float64)).max() <= 2e-3 * max(1.0, np.abs(ref2).max())
    if T <= 4 and ops.rowwise_scaled_linear_s4s4_residual_hq_supported(T, 256, heads * d):   # K = 5120: PRO_RQ, two chunks per thread
        Kd, N = heads * d, 1024
        wq, wsc = rng.integers(-128, 128, (N, Kd // 2)).astype(np.int8), (rng.random(N) * 0.01 + 0.001).astype(np.float16)
        resid = (rng.standard_normal((T, N))).astype(np.float16)
        q0 = torch.empty(T, Kd // 2, dtype=torch.int8, device=DEV); s0 = torch.empty(T, dtype=torch.float16, device=DEV)
        ops.fuse_sym_quant(o0, s0, q0)
        h0 = dev(resid)
        ops.rowwise_scaled_linear_s4s4_residual(q0, s0, dev(wq), dev(wsc), h0, h0)
        h1 = dev(resid)
        ops.rowwise_scaled_linear_s4s4_residual_hq(o2, pam, 1.0, dev(wq), dev(wsc), h1, h1)
        torch.cuda.synchronize()
        assert torch.equal(h0.view(torch.int16), h1.view(torch.int16))
        qo, so = oracle.rowabsmax_quant_i4(host(o2), 1.0)
        assert np.array_equal(bits(host(h1)), bits(oracle.add_f16(resid, oracle.gemm_w4a4(qo, so, wq, wsc))))


@pytest.mark.parametrize("ctx_lens,q_len,n_splits,heads,nkv", [([37, 128, 129, 500], 1, 2, 40, 40), ([600, 5, 20], 1, 8, 40, 40),
                                                                ([37, 130], 2, 2, 40, 40), ([300], 4, 8, 40, 40), ([90, 17], 1, 1, 24, 24)])
def test_spread_table_factor_head_transform_behind_the_attention_launch(ops, oracle, ctx_lens, q_len, n_splits, heads, nkv):
    """The same kernel behind a real attention launch that leaves its partials (out = NULL), against the oracle's head
    transform of the in-kernel-merged attention output (out != NULL): 1e-3 -- the two attention launches may be different
    kernels (per-wave form for partials: another summation order inside a split, include/qspec_hip.h)."""
    from qspec_amd import hadamard_tables
    rng = np.random.default_rng(sum(ctx_lens) * 3 + q_len + heads)
    d, bs = 128, 16
    n_seqs = len(ctx_lens)
    bt, kc, vc = make_paged(rng, n_seqs, ctx_lens, nkv, d, bs)
    T = n_seqs * q_len
    row = (heads + 2 * nkv) * d
    qkv = dev((rng.standard_normal((T, row)) * 0.5).astype(np.float16))
    q_start = dev((np.arange(n_seqs + 1) * q_len).astype(np.int32))
    ctx = dev(np.array(ctx_lens, np.int32))
    hadK, K = hadamard_tables.get_hadK(heads)
    hk = hadK.to(torch.float16).to(DEV)
    had_scale = oracle.rsqrt_scale(heads)
    ws = torch.zeros(ops.paged_attention_workspace_bytes(T, heads, d, n_splits), dtype=torch.uint8, device=DEV)
    attn = torch.empty(T, heads * d, dtype=torch.float16, device=DEV)
    ops.paged_attention(qkv, row, dev(kc), dev(vc), dev(bt), ctx, q_start, T, q_len, heads, d ** -0.5, n_splits, ws, attn)
    ws.zero_()
    ops.paged_attention(qkv, row, dev(kc), dev(vc), dev(bt), ctx, q_start, T, q_len, heads, d ** -0.5, n_splits, ws, None)
    o1 = torch.empty(T, heads * d, dtype=torch.float16, device=DEV)
    ops.heads_hadamard_mix_merged_spread(ws, T, n_splits, T, heads, d, hk, K, had_scale, o1)
    ref = oracle.heads_hadamard(host(attn), heads, had_scale, hadK.numpy().astype(np.float16), K)
    assert np.abs(host(o1).astype(np.float64) - ref.astype(np.float64)).max() <= 1e-3


def test_embedding(ops):
    rng = np.random.default_rng(0)
    V, H = 1000, 4096
    table = rng.standard_normal((V, H)).astype(np.float16)
    ids = np.array([0, 999, 5, 5], np.int64)
    out = torch.empty(4, H, dtype=torch.float16, device=DEV)
    ops.embedding(dev(ids), dev(table), out)
    assert np.array_equal(bits(host(out)), bits(table[ids]))


@pytest.mark.parametrize("T,V", [(4, 128256), (16, 32000), (3, 1000)])
def test_softmax_argmax(ops, oracle, T, V):
    rng = np.random.default_rng(V)
    logits = (rng.standard_normal((T, V)) * 3).astype(np.float16)
    logits[0, 7] = logits[0, 9] = np.float16(30.0)  # tie -> first index
    p0, t0 = oracle.softmax_argmax(logits)
    probs = torch.empty(T, V, dtype=torch.float32, device=DEV)
    tok = torch.empty(T, dtype=torch.int64, device=DEV)
    ops.softmax_argmax(dev(logits), probs, tok)
    assert np.array_equal(host(tok), t0) and t0[0] == 7
    assert np.array_equal(host(probs).view(np.uint32), p0.view(np.uint32))


@pytest.mark.parametrize("T,V,K", [(4, 128256, 4096), (16, 128256, 4096), (1, 128256, 4096), (3, 32000, 2048), (16, 2048, 1024), (8, 16384, 8192),
                                   (32, 128256, 4096), (17, 20000, 4096)])
def test_lm_head_softmax_argmax_fused_front_end(ops, oracle, T, V, K):
    """lm_head launch (row maxima from its epilogue) + denominator + write-once probabilities == the two-step path
    (qspec_linear_f16 + qspec_softmax_argmax) bit for bit, and == the oracle's softmax of the GPU's own logits
    (logits_processor.py:92-97 + sampler.py:270-287).  Ties: the first column wins, also across workgroups."""
    rng = np.random.default_rng(V + T)
    x = dev((rng.standard_normal((T, K)) * 1.0).astype(np.float16))
    w_np = (rng.standard_normal((V, K)) * 0.02).astype(np.float16)
    w_np[V // 2 + 5] = w_np[7]          # two identical vocabulary rows, far apart: an exact tie of their logits
    w_np[V - 3] = w_np[7]
    w = dev(w_np)
    logits_a = torch.empty(T, V, dtype=torch.float16, device=DEV)
    probs_a = torch.empty(T, V, dtype=torch.float32, device=DEV); tok_a = torch.empty(T, dtype=torch.int64, device=DEV)
    ops.linear_f16(x, w, logits_a)
    ops.softmax_argmax(logits_a, probs_a, tok_a)
    logits_b = torch.empty_like(logits_a); probs_b = torch.full_like(probs_a, float("nan")); tok_b = torch.empty_like(tok_a)
    assert ops.lm_head_softmax_argmax_supported(T, V, K)
    ops.lm_head_softmax_argmax(x, w, logits_b, probs_b, tok_b)
    torch.cuda.synchronize()
    assert torch.equal(logits_a.view(torch.int16), logits_b.view(torch.int16))
    assert torch.equal(probs_a.view(torch.int32), probs_b.view(torch.int32)) and torch.equal(tok_a, tok_b)
    p0, t0 = oracle.softmax_argmax(host(logits_b))
    assert np.array_equal(host(tok_b), t0)
    assert np.array_equal(host(probs_b).view(np.uint32), p0.view(np.uint32))
    # force the tie to be the row maximum: boost the shared direction
    x2 = dev((w_np[7].astype(np.float32)[None, :] * 50.0).repeat(T, 0).astype(np.float16))
    ops.lm_head_softmax_argmax(x2, w, logits_b, probs_b, tok_b)
    torch.cuda.synchronize()
    assert host(tok_b).tolist() == [7] * T
    assert np.array_equal(host(tok_b), oracle.softmax_argmax(host(logits_b))[1])


def test_rejection_sampler_golden_bit_exact(ops, golden_dir):
    """Outputs of the REFERENCE sampler run on CPU with recorded draws: masks, recovered ids, layout, counters."""
    g = np.load(os.path.join(golden_dir, "rejection.npz"))
    for idx in range(5):
        for flavour in ("random", "agree", "onehot"):
            key = f"c{idx}_{flavour}"
            tq, dp, ids, bonus, U, E = (g[key + s] for s in ("_tq", "_dp", "_ids", "_bonus", "_U", "_E"))
            B, k, V = dp.shape
            out = torch.empty(B, k + 1, dtype=torch.int64, device=DEV)
            acc = torch.empty(B, k, dtype=torch.uint8, device=DEV)
            rec = torch.empty(B, k, dtype=torch.int64, device=DEV)
            counters = torch.zeros(3, dtype=torch.int64, device=DEV)
            ops.rejection_sample(dev(tq), dev(bonus.reshape(-1)), dev(dp), dev(ids), out, acc, rec, counters,
                                 uniform=dev(U), exponential=dev(E))
            assert np.array_equal(host(out), g[key + "_out"]), key
            assert np.array_equal(host(counters), g[key + "_counters"]), key


def test_rejection_sampler_vs_oracle_full_vocab(ops, oracle):
    rng = np.random.default_rng(4)
    B, k, V = 4, 3, 128256
    logits = rng.standard_normal((B, k + 1, V)).astype(np.float32) * 4
    tq = np.exp(logits - logits.max(-1, keepdims=True)); tq /= tq.sum(-1, keepdims=True)
    dl = logits[:, :k] + rng.standard_normal((B, k, V)).astype(np.float32)
    dp = np.exp(dl - dl.max(-1, keepdims=True)); dp /= dp.sum(-1, keepdims=True)
    tq, dp = tq.astype(np.float32), dp.astype(np.float32)
    ids = dp.argmax(-1).astype(np.int64)
    bonus = tq[:, -1].argmax(-1).astype(np.int64)
    U = rng.random((B, k)).astype(np.float32)
    E = rng.exponential(1.0, (B, k, V)).astype(np.float32)
    o0, a0, r0, c0 = oracle.rejection_sample(tq, bonus, dp, ids, U, E)
    out = torch.empty(B, k + 1, dtype=torch.int64, device=DEV)
    acc = torch.empty(B, k, dtype=torch.uint8, device=DEV)
    rec = torch.empty(B, k, dtype=torch.int64, device=DEV)
    counters = torch.zeros(3, dtype=torch.int64, device=DEV)
    ops.rejection_sample(dev(tq), dev(bonus), dev(dp), dev(ids), out, acc, rec, counters, uniform=dev(U), exponential=dev(E))
    assert np.array_equal(host(acc).astype(bool), a0) and np.array_equal(host(rec), r0)
    assert np.array_equal(host(out), o0) and list(host(counters)) == list(c0)


def test_rejection_sampler_philox_path(ops):
    """Without injected draws: deterministic per (seed, offset), structurally valid, and target-distributed
    in the one-hot construction of tests/samplers/test_rejection_sampler.py."""
    B, k, V = 64, 3, 512
    rng = np.random.default_rng(0)
    tq = np.zeros((B, k + 1, V), np.float32); tgt = rng.integers(0, V, (B, k + 1)); np.put_along_axis(tq, tgt[..., None], 1.0, -1)
    dp = np.zeros((B, k, V), np.float32); ids = rng.integers(0, V, (B, k)); np.put_along_axis(dp, ids[..., None], 1.0, -1)
    bonus = tgt[:, -1].astype(np.int64)
    outs = []
    for seed in (1, 1, 2):
        out = torch.empty(B, k + 1, dtype=torch.int64, device=DEV)
        acc = torch.empty(B, k, dtype=torch.uint8, device=DEV)
        rec = torch.empty(B, k, dtype=torch.int64, device=DEV)
        ops.rejection_sample(dev(tq), dev(bonus), dev(dp), dev(ids.astype(np.int64)), out, acc, rec, None, seed=seed, offset=7)
        outs.append((host(out), host(acc), host(rec)))
    assert np.array_equal(outs[0][0], outs[1][0])
    # one-hot: accepted iff draft == target; the recovered token is the target token
    assert np.array_equal(outs[0][1].astype(bool), ids == tgt[:, :k])
    rej = ~(ids == tgt[:, :k])
    assert np.array_equal(outs[0][2][rej], tgt[:, :k][rej])

def test_bookkeeping_launches_with_the_embedding_rows(ops):
    _bookkeeping_with_embedding_check(ops, 16)


@pytest.mark.parametrize("bs", [8, 32])
def test_bookkeeping_launches_with_the_embedding_rows_block_sizes(ops, bs):
    _bookkeeping_with_embedding_check(ops, bs)


def _bookkeeping_with_embedding_check(ops, bs):
    """spec_prepare_draft / spec_advance_draft / spec_prepare_verify with embed=(table, hidden): the same index tensors as the
    plain launches (empty slots, a slot sitting the step out, a row out of blocks included) and hidden[row] = table[token]
    (row 0 for padded rows), i.e. what the plain launch followed by ops.embedding gives -- bit for bit."""
    rng = np.random.default_rng(77)
    B, k, V, H = 6, 3, 500, 256
    max_blocks = 64 // bs   # 64 slots per sequence at every block size
    table = dev((rng.standard_normal((V, H))).astype(np.float16))
    bt = dev(rng.permutation(B * max_blocks).reshape(B, max_blocks).astype(np.int32))
    seq_lens = dev(np.array([37, 0, 5, 63, 64, 20], np.int32))     # slot 1 empty; slot 4: position 63 is its last slot
    mask = dev(np.array([1, 1, 0, 1, 1, 1], np.int32))             # slot 2 sits the step out
    last = dev(rng.integers(0, V, B).astype(np.int64))
    i64, i32 = torch.int64, torch.int32

    def bufs(n):
        return [torch.full((n,), 7, dtype=i64, device=DEV) for _ in range(3)] + [torch.full((B,), 7, dtype=i32, device=DEV)]
    # prepare_draft
    eff0 = seq_lens * mask
    t0, p0, s0, c0 = bufs(B)
    ops.spec_prepare_draft(last, eff0, bt, bs, t0, p0, s0, c0)
    h0 = torch.empty(B, H, dtype=torch.float16, device=DEV)
    ops.embedding(t0, table, h0)
    t1, p1, s1, c1 = bufs(B)
    eff1 = torch.full((B,), -5, dtype=i32, device=DEV)
    h1 = torch.full((B, H), 3.0, dtype=torch.float16, device=DEV)
    ops.spec_prepare_draft(last, seq_lens, bt, bs, t1, p1, s1, c1, embed=(table, h1), step_mask=mask, eff_lens=eff1)
    torch.cuda.synchronize()
    for a, b in ((t0, t1), (p0, p1), (s0, s1), (c0, c1), (eff0, eff1)):
        assert torch.equal(a, b)
    assert torch.equal(h0.view(torch.int16), h1.view(torch.int16))
    assert host(s1).tolist()[1] == -1 and host(s1).tolist()[2] == -1
    # advance_draft (slot 4 runs out of blocks at position 64: frozen, its token still updated)
    sampled = dev(rng.integers(0, V, B).astype(np.int64))
    ta, pa, sa, ca = (x.clone() for x in (t0, p0, s0, c0))
    ops.spec_advance_draft(bs, ta, sampled, pa, ca, sa, bt)
    ha = torch.empty(B, H, dtype=torch.float16, device=DEV)
    ops.embedding(ta, table, ha)
    tb, pb, sb, cb = (x.clone() for x in (t0, p0, s0, c0))
    hb = torch.full((B, H), 3.0, dtype=torch.float16, device=DEV)
    ops.spec_advance_draft(bs, tb, sampled, pb, cb, sb, bt, embed=(table, hb))
    torch.cuda.synchronize()
    for a, b in ((ta, tb), (pa, pb), (sa, sb), (ca, cb)):
        assert torch.equal(a, b)
    assert torch.equal(ha.view(torch.int16), hb.view(torch.int16))
    assert host(sb).tolist()[4] == -1 and host(tb).tolist()[4] == host(sampled).tolist()[4]
    # prepare_verify (draft ids as a strided [B, k] view of a step-major buffer, as the engine passes them)
    ids_kb = dev(rng.integers(0, V, (k, B)).astype(np.int64))
    ids = ids_kb.transpose(0, 1)
    n = B * (k + 1)
    tv0, pv0, sv0, cv0 = bufs(n)
    ops.spec_prepare_verify(last, ids, eff0, bt, bs, tv0, pv0, sv0, cv0)
    hv0 = torch.empty(n, H, dtype=torch.float16, device=DEV)
    ops.embedding(tv0, table, hv0)
    tv1, pv1, sv1, cv1 = bufs(n)
    hv1 = torch.full((n, H), 3.0, dtype=torch.float16, device=DEV)
    ops.spec_prepare_verify(last, ids, eff0, bt, bs, tv1, pv1, sv1, cv1, embed=(table, hv1))
    torch.cuda.synchronize()
    for a, b in ((tv0, tv1), (pv0, pv1), (sv0, sv1), (cv0, cv1)):
        assert torch.equal(a, b)
    assert torch.equal(hv0.view(torch.int16), hv1.view(torch.int16))



def test_advance_step(ops, oracle):
    _advance_step_check(ops, oracle, 16)


@pytest.mark.parametrize("bs", [8, 32])
def test_advance_step_block_sizes(ops, oracle, bs):
    _advance_step_check(ops, oracle, bs)


def _advance_step_check(ops, oracle, bs):
    rng = np.random.default_rng(1)
    n, mb = 4, 160 // bs
    bt = rng.integers(0, 1000, (n, mb)).astype(np.int32)
    seq_lens = np.array([1, bs, 2 * bs - 1, 100], np.int32)   # a block's last slot, the next block's first
    sampled = rng.integers(0, 32000, n).astype(np.int64)
    it, pos, sl, sm = np.zeros(n, np.int64), np.zeros(n, np.int64), seq_lens.copy(), np.zeros(n, np.int64)
    oracle.advance_step(it, sampled, pos, sl, sm, bt, bs)
    d_it, d_pos, d_sl, d_sm = dev(np.zeros(n, np.int64)), dev(np.zeros(n, np.int64)), dev(seq_lens), dev(np.zeros(n, np.int64))
    ops.advance_step_flashattn(n, n, bs, d_it, dev(sampled), d_pos, d_sl, d_sm, dev(bt))
    assert np.array_equal(host(d_it), it) and np.array_equal(host(d_pos), pos)
    assert np.array_equal(host(d_sl), sl) and np.array_equal(host(d_sm), sm)


# ------------------------------------------------------------------ tensor-parallel views

@pytest.mark.parametrize("M,N,K", [(16, 4096, 14336), (5, 4096, 14336), (16, 1024, 14336), (16, 5120, 13824), (3, 1024, 13824)])
def test_w4a16_long_k_slices_and_norm_finish(ops, oracle, M, N, K):
    """Long-K W4A16 (down_proj): K slices -> raw fp32 sums; w4a16_linear finishes them with a small launch, the verify
    pass inside the next norm.  Both against the oracle (1e-3) and against each other (bit for bit)."""
    rng = np.random.default_rng(M + N)
    x = rand_hidden(rng, M, K)
    w = rand_w4(rng, N, K)
    wq = oracle.pack_i4(w)
    ws = (rng.random(N) * 0.002 + 0.0005).astype(np.float16)
    S = ops.w4a16_linear_partial_slices(M, N, K)
    assert S == (3 if K == 13824 else 4)   # four slices first: a workgroup stages as many activation bytes as it streams weight bytes
    out = torch.empty(M, N, dtype=torch.float16, device=DEV)
    ops.w4a16_linear(dev(x), dev(wq), dev(ws), out)
    assert_close_1e3(host(out), oracle.gemm_w4a16(x, wq, ws))
    if N % 1024 == 0:   # the norm-side finish needs a hidden size the norm kernel is built for
        part = torch.empty(S, M, N, dtype=torch.float32, device=DEV)
        ops.w4a16_linear_partial(dev(x), dev(wq), part, S)
        hidden = dev(rand_hidden(rng, M, N))
        n0 = torch.empty_like(hidden); h0 = torch.empty_like(hidden)
        ops.add_rms_norm_fp16(n0, h0, hidden, out, 1e-5)
        n1 = torch.empty_like(hidden); h1 = torch.empty_like(hidden)
        ops.add_rms_norm_fp16_partial(n1, h1, hidden, part, dev(ws), S, 1e-5)
        torch.cuda.synchronize()
        assert torch.equal(h0.view(torch.int16), h1.view(torch.int16))
        assert torch.equal(n0.view(torch.int16), n1.view(torch.int16))


@pytest.mark.parametrize("M,N,K", [(32, 4096, 4096), (32, 8192, 8192), (192, 4096, 14336), (32, 4096, 14336), (64, 5120, 13824),
                                   (192, 4096, 4096), (100, 1024, 4096)])
def test_w4a16_tiled_plan_slices_finished_in_the_norm(ops, oracle, M, N, K):
    """17+ tokens: where the M-tiled kernel's launch plan cuts K into slices, the verify pass leaves their raw fp32 sums to the
    norm that follows (hidden = x + h(sum * ws), LN) instead of a finishing launch: the same bits as w4a16_linear followed by
    add_rms_norm_fp16, and the GEMM within 1e-3 of the oracle.  A shape the plan does not slice answers 0."""
    rng = np.random.default_rng(M + N + K)
    x = rand_hidden(rng, M, K)
    wq = dev(oracle.pack_i4(rand_w4(rng, N, K)))
    ws_np = (rng.random(N) * 0.002 + 0.0005).astype(np.float16)
    ws = dev(ws_np)
    S = ops.w4a16_linear_partial_slices(M, N, K)
    assert S == 0 or 2 <= S <= 8
    out = torch.empty(M, N, dtype=torch.float16, device=DEV)
    ops.w4a16_linear(dev(x), wq, ws, out)
    if M <= 64:
        assert_close_1e3(host(out), oracle.gemm_w4a16(x, host(wq), ws_np))
    if S == 0:
        with pytest.raises(RuntimeError):
            ops.w4a16_linear_partial(dev(x), wq, torch.empty(2, M, N, dtype=torch.float32, device=DEV), 2)
        return
    part = torch.empty(S, M, N, dtype=torch.float32, device=DEV)
    ops.w4a16_linear_partial(dev(x), wq, part, S)
    hidden = dev(rand_hidden(rng, M, N))
    n0 = torch.empty_like(hidden); h0 = torch.empty_like(hidden)
    ops.add_rms_norm_fp16(n0, h0, hidden, out, 1e-5)
    n1 = torch.empty_like(hidden); h1 = torch.empty_like(hidden)
    ops.add_rms_norm_fp16_partial(n1, h1, hidden, part, ws, S, 1e-5)
    torch.cuda.synchronize()
    assert torch.equal(h0.view(torch.int16), h1.view(torch.int16))
    assert torch.equal(n0.view(torch.int16), n1.view(torch.int16))
    with pytest.raises(RuntimeError):   # another count than the plan's
        ops.w4a16_linear_partial(dev(x), wq, torch.empty(S + 1, M, N, dtype=torch.float32, device=DEV), S + 1)


@pytest.mark.parametrize("M,N,K,world", [(16, 4096, 4096, 8), (16, 4096, 14336, 8), (4, 1024, 3584, 2)])
def test_w4a16_ksliced_partials_sum_to_full(ops, oracle, M, N, K, world):
    from qspec_amd.parallel import shard_range
    rng = np.random.default_rng(K + world)
    x = dev(rand_hidden(rng, M, K))
    wq = dev(oracle.pack_i4(rand_w4(rng, N, K)))
    ws = dev((rng.random(N) * 0.002 + 0.0005).astype(np.float16))
    full = torch.empty(M, N, dtype=torch.float16, device=DEV)
    ops.w4a16_linear(x, wq, ws, full)
    acc = torch.zeros(M, N, dtype=torch.float32, device=DEV)
    for r in range(world):
        k0, k1 = shard_range(K, world, r, 128)
        part = torch.empty(M, N, dtype=torch.float16, device=DEV)
        ops.w4a16_linear_ksliced(x, wq, ws, part, k0, k1)
        acc += part.float()
    # each partial is rounded to fp16 before the all-reduce sums them: a few fp16 ulps of the partial magnitudes
    d = np.abs(host(acc) - host(full).astype(np.float32))
    assert d.max() < 4e-3 * max(1.0, float(np.abs(host(full)).max())), d.max()
    # a single full-range "slice" is the plain op, bit for bit
    one = torch.empty_like(full)
    ops.w4a16_linear_ksliced(x, wq, ws, one, 0, K)
    assert torch.equal(one.view(torch.int16), full.view(torch.int16))


@pytest.mark.parametrize("M,N,K,world", [(16, 4096, 4096, 8), (16, 4096, 14336, 8), (16, 4096, 14336, 2), (4, 1024, 3584, 2),
                                         (16, 5120, 13824, 2), (32, 8192, 28672, 8), (32, 8192, 8192, 8)])
def test_w4a16_ksliced_raw_partials_reduce_to_the_oracle(ops, oracle, M, N, K, world):
    """Row-parallel shards as raw fp32 sums (the TP verify pass): summed over the ranks in fp32, then scale + ONE fp16
    rounding + residual add + norm in qspec_add_rms_norm_fp16_partial -- against the oracle's GEMM / add / norm."""
    from qspec_amd.parallel import shard_range
    rng = np.random.default_rng(K + world + 1)
    x = rand_hidden(rng, M, K)
    wq = oracle.pack_i4(rand_w4(rng, N, K))
    ws = (rng.random(N) * 0.002 + 0.0005).astype(np.float16)
    resid = rand_hidden(rng, M, N)
    xd, wd = dev(x), dev(wq)
    acc = torch.zeros(1, M, N, dtype=torch.float32, device=DEV)
    for r in range(world):
        k0, k1 = shard_range(K, world, r, 128)
        part = torch.full((M, N), float("nan"), dtype=torch.float32, device=DEV)
        ops.w4a16_linear_ksliced_raw(xd, wd, part, k0, k1)
        acc[0] += part
    ref = oracle.gemm_w4a16(x, wq, ws)
    got = (acc[0] * dev(ws).float()[None, :]).half()
    assert_close_1e3(host(got), ref)
    if N % 1024 == 0:
        normed = torch.empty(M, N, dtype=torch.float16, device=DEV); hid = torch.empty_like(normed)
        ops.add_rms_norm_fp16_partial(normed, hid, dev(resid), acc, dev(ws), 1, 1e-5)
        h_ref = oracle.add_f16(resid, ref).astype(np.float64)
        err = np.abs(host(hid).astype(np.float64) - h_ref)
        # 1e-3 of the GEMM result (its one fp16 rounding may flip) + 1e-3 of the sum (the add's own rounding)
        bar = 1e-3 * (np.maximum(1.0, np.abs(ref.astype(np.float64))) + np.maximum(1.0, np.abs(h_ref)))
        assert (err <= bar).all(), (err / bar).max()


@pytest.mark.parametrize("M,I,K,world", [(16, 14336, 4096, 2), (16, 14336, 4096, 8), (4, 3584, 1024, 2)])
def test_gate_up_shards_concatenate_to_full(ops, oracle, M, I, K, world):
    from qspec_amd.parallel import shard_range
    rng = np.random.default_rng(I + world)
    x = dev(rand_hidden(rng, M, K))
    wq = dev(oracle.pack_i4(rand_w4(rng, 2 * I, K)))
    ws = dev((rng.random(2 * I) * 0.002 + 0.0005).astype(np.float16))
    full = ops.gate_up_silu_linear(x, None, wq, ws, torch.empty(M, I, dtype=torch.float16, device=DEV))
    act = torch.zeros(M, I, dtype=torch.float16, device=DEV)
    for r in range(world):
        c0, c1 = shard_range(I, world, r, 32)
        ops.gate_up_silu_linear_shard(x, wq, ws, act, c0, c1 - c0)
    torch.cuda.synchronize()
    # a shard launch may pick a different K-block split than the full launch (fp32 summation order), so the
    # concatenation equals the unsharded result to rounding, not bit for bit
    assert_close_1e3(host(act), host(full))
    assert (host(act) != 0).mean() > 0.99   # every channel range was written


def _run_tp_check(args, nproc, extra_env=None):
    import subprocess, sys, socket
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = os.path.join(root, "tests", "tp_check.py")
    if nproc:
        s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), script] + args
    else:
        cmd = [sys.executable, script] + args
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=root, env=dict(os.environ, **(extra_env or {})))
    if "TP_OK" not in r.stdout:   # the full output of the ranks, for the post-mortem (pytest truncates long reprs)
        os.makedirs(os.path.join(root, "gpurun_out"), exist_ok=True)
        with open(os.path.join(root, "gpurun_out", "tp_check_%s.log" % "_".join(a.strip("-") for a in args)), "w") as f:
            f.write(r.stdout + "\n---- stderr ----\n" + r.stderr)
    assert "TP_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    print(r.stdout.strip().splitlines()[-1])


def test_oneshot_all_reduce_two_processes_one_gpu():
    """The one-shot push all-reduce over IPC-mapped peer buffers (csrc/comm.hip; contract: vllm custom_all_reduce.py:
    50-56,242-255) with two processes on this GPU: eager, inside a replayed hipGraph, and the fallback path."""
    import subprocess, sys, socket
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(root, "tests", "oneshot_check.py")],
                       capture_output=True, text=True, timeout=300, cwd=root, env=env)
    if "ONESHOT_OK" not in r.stdout or "ONESHOT_DEAD_PEER_OK" not in r.stdout:
        os.makedirs(os.path.join(root, "gpurun_out"), exist_ok=True)
        with open(os.path.join(root, "gpurun_out", "oneshot_check.log"), "w") as f:
            f.write(r.stdout + "\n---- stderr ----\n" + r.stderr)
    assert "ONESHOT_OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    # a raised error word ends every later wait at once (a lost peer costs ONE timeout, not one per collective)
    assert "ONESHOT_DEAD_PEER_OK" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


def test_tensor_parallel_engine_two_ranks():
    """2 gloo ranks (processes) on this GPU: TP verify path vs single-GPU path + engine cycles (tests/tp_check.py)."""
    _run_tp_check(["--family", "tiny"], 2)


def test_tensor_parallel_engine_two_ranks_oneshot_all_reduce():
    """The same check with the row-parallel partials reduced by the one-shot push all-reduce (QSPEC_ONESHOT_AR=1)
    instead of the host-staged gloo collective: the path a multi-GPU run takes over xGMI, here over IPC on one GPU."""
    _run_tp_check(["--family", "tiny"], 2, {"QSPEC_ONESHOT_AR": "1", "HSA_ENABLE_IPC_MODE_LEGACY": "0"})


def test_tensor_parallel_llama2_13b_width_two_ranks():
    """BASELINE.json configs[3] in its TP form: one full-width Llama-2-13B layer (40 heads = had40 on the head axis,
    I = 13824 = had108 x 128; K ranges of 5120 / 13824), 2 gloo ranks."""
    _run_tp_check(["--family", "llama-2-13b"], 2)


def test_tensor_parallel_llama3_70b_width_eight_ranks():
    """configs[4] in its TP form: one full-width Llama-3-70B layer, bs = 8, eight ranks (threads of one process: the
    GPU box admits at most 6 processes on its card)."""
    _run_tp_check(["--family", "llama-3-70b", "--threads", "8"], 0)


def test_tensor_parallel_llama3_70b_width_four_process_ranks():
    """The same layer with 4 gloo ranks as processes (host-staged collectives)."""
    _run_tp_check(["--family", "llama-3-70b"], 4)


# ------------------------------------------------------------------ W4A16, prefill-sized M (M-tiled kernel)

@pytest.mark.parametrize("M,N,K", [(33, 256, 512), (64, 128, 768), (96, 384, 1024), (192, 6144, 4096),
                                   (200, 4096, 4096), (129, 256, 11008), (512, 512, 14336), (1000, 128, 2048)])
def test_w4a16_tiled_within_1e3(ops, oracle, M, N, K):
    """Prompt-pass / large-batch verify GEMM: tiles of 32..128 tokens x 128 weight rows over the packed int4 buffer
    (both ring depths: K % 512 == 0 and K % 256 == 0; ragged last token block)."""
    rng = np.random.default_rng(M + N + K)
    x = rand_hidden(rng, M, K)
    wq = oracle.pack_i4(rand_w4(rng, N, K))
    ws = (rng.random(N) * 0.002 + 0.0005).astype(np.float16)
    out = torch.full((M + 1, N), 7.0, dtype=torch.float16, device=DEV)   # guard row: nothing beyond M is written
    ops.w4a16_linear(dev(x), dev(wq), dev(ws), out[:M])
    assert_close_1e3(host(out[:M]), oracle.gemm_w4a16(x, wq, ws))
    assert torch.all(out[M] == 7.0)


def test_w4a16_tiled_exact_on_integer_data(ops, oracle):
    """Integer activations: every fp32 partial sum is exact, so a k-permutation / lane-map error is a bit mismatch."""
    rng = np.random.default_rng(55)
    M, N, K = 160, 256, 1024
    x = rng.integers(-4, 5, (M, K)).astype(np.float16)
    wq = oracle.pack_i4(rand_w4(rng, N, K))
    ws = np.ones(N, np.float16)
    out = torch.empty(M, N, dtype=torch.float16, device=DEV)
    ops.w4a16_linear(dev(x), dev(wq), dev(ws), out)
    assert np.array_equal(bits(host(out)), bits(oracle.gemm_w4a16(x, wq, ws)))


# ------------------------------------------------------------------ head Hadamard for head counts with a table factor

@pytest.mark.parametrize("T,heads,d", [(3, 40, 128), (2, 24, 64), (1, 80, 128), (5, 12, 128)])
def test_heads_hadamard_mix_bit_exact(ops, oracle, T, heads, d):
    from qspec_amd import hadamard_tables
    rng = np.random.default_rng(heads + T)
    hadK, K = hadamard_tables.get_hadK(heads)
    assert K > 1
    x = (rng.standard_normal((T, heads * d))).astype(np.float16)
    scale = oracle.rsqrt_scale(heads)
    ref = oracle.heads_hadamard(x, heads, scale, hadK.numpy().astype(np.float16), K)
    out = torch.empty(T, heads * d, dtype=torch.float16, device=DEV)
    ops.heads_hadamard_mix(dev(x).view(T, heads, d), hadK.to(torch.float16).to(DEV), K, scale, out)
    assert np.array_equal(bits(host(out)), bits(ref))


def test_fwht_rows_of_one(ops, oracle):
    """get_hadK(n) with n / K == 1 (12, 20, 28, 40 heads): the FWHT stage only scales and rounds."""
    rng = np.random.default_rng(3)
    x = rng.standard_normal((1000, 1)).astype(np.float16)
    out = torch.empty(1000, 1, dtype=torch.float16, device=DEV)
    ops.faster_fast_hadamard_transform(dev(x), 0.158, out)
    assert np.array_equal(bits(host(out)), bits(oracle.fwht(x, 0.158)))


@pytest.mark.parametrize("M,N,K", [(17, 160, 512), (32, 2048, 4096), (192, 1504, 4096), (200, 128, 768), (513, 96, 1024)])
def test_linear_f16_tiled_within_1e3(ops, oracle, M, N, K):
    """lm_head at prefill / large-batch M (M-tiled kernel): ragged token block, N not a multiple of the 128-row tile."""
    rng = np.random.default_rng(M + N + K)
    x = rand_hidden(rng, M, K)
    w = (rng.standard_normal((N, K)) * 0.02).astype(np.float16)
    out = torch.full((M + 1, N), 7.0, dtype=torch.float16, device=DEV)
    ops.linear_f16(dev(x), dev(w), out[:M])
    assert_close_1e3(host(out[:M]), oracle.gemm_f16(x, w))
    assert torch.all(out[M] == 7.0)


@pytest.mark.parametrize("M,N", [(1, 16384), (4, 16400), (16, 32768), (3, 128256), (17, 16384), (32, 32768), (24, 20000)])
def test_linear_f16_lds_dma_stream_within_1e3(ops, oracle, M, N):
    """The long-stream lm_head (K = 4096, >= 4 tiles per workgroup) through self-service LDS-DMA (`gemm_f16_sdma_kernel`, and
    `gemm_f16_sdma2_kernel` = two 16-token tiles over one weight pass from 17 tokens on): a vocabulary whose tile count is not
    a multiple of the grid, rows beyond M untouched.
    (N = 20000: 1250 tiles on 250 workgroups x 5.)"""
    K = 4096
    rng = np.random.default_rng(M + N)
    x = rand_hidden(rng, M, K)
    w = (rng.standard_normal((N, K)) * 0.02).astype(np.float16)
    out = torch.full((M + 1, N), 7.0, dtype=torch.float16, device=DEV)
    ops.linear_f16(dev(x), dev(w), out[:M])
    assert_close_1e3(host(out[:M]), oracle.gemm_f16(x, w))
    assert torch.all(out[M] == 7.0)
    again = torch.empty(M, N, dtype=torch.float16, device=DEV)
    ops.linear_f16(dev(x), dev(w), again)
    assert torch.equal(again.view(torch.int16), out[:M].view(torch.int16))      # deterministic


# ------------------------------------------------------------------ W4A4 streaming kernels with two token tiles (M 17..32)

@pytest.mark.parametrize("M", [17, 24, 32])
def test_w4a4_two_token_tiles_layer_shapes(ops, oracle, M):
    """Batch 32 draft pass: the streaming W4A4 kernels with two 16-token tiles per workgroup (packed activation
    fragments) at the Llama-3-8B layer shapes -- plain / qkv+RoPE+KV / gate_up+silu / residual epilogues against the
    oracle formula (bit for bit) and against the separate reference ops."""
    rng = np.random.default_rng(M)
    K, nq, nkv, d, bs, I = 4096, 32, 8, 128, 16, 14336
    N = (nq + 2 * nkv) * d
    xq_np, xs_np = oracle.pack_i4(rand_w4(rng, M, K)), (rng.random(M) * 0.1 + 0.01).astype(np.float16)
    xq, xs = dev(xq_np), dev(xs_np)
    w_np = rng.integers(-128, 128, (N, K // 2)).astype(np.int8)
    ws_np = (rng.random(N) * 0.01 + 0.001).astype(np.float16)
    wq, ws = dev(w_np), dev(ws_np)
    # plain, against the oracle
    out = torch.empty(M, N, dtype=torch.float16, device=DEV)
    ops.rowwise_scaled_linear_cutlass_s4s4_unified(xq, xs, wq, ws, None, out)
    assert np.array_equal(bits(host(out)), bits(oracle.gemm_w4a4(xq_np, xs_np, w_np, ws_np)))
    # qkv + RoPE + KV write == plain + rope_kv_write
    cs = dev(oracle.make_cos_sin_cache(d, 2048, 500000.0))
    pos = dev(rng.integers(0, 2048, M).astype(np.int64))
    slots = dev(rng.permutation(64 * bs)[:M].astype(np.int64))
    kc0 = torch.zeros(64, bs, nkv, d, dtype=torch.float16, device=DEV); vc0 = torch.zeros_like(kc0)
    ref = out.clone()
    ops.rope_kv_write(pos, ref, cs, kc0, vc0, slots, nq, nkv, d)
    kc1 = torch.zeros_like(kc0); vc1 = torch.zeros_like(kc0)
    qkv = torch.empty_like(ref)
    ops.qkv_rope_linear(xq, xs, wq, ws, qkv, pos, cs, kc1, vc1, slots, nq, nkv, d)
    torch.cuda.synchronize()
    assert torch.equal(qkv.view(torch.int16), ref.view(torch.int16))
    assert torch.equal(kc1, kc0) and torch.equal(vc1, vc0)
    # gate_up + silu*up == plain + silu_mul
    wg = dev(rng.integers(-128, 128, (2 * I, K // 2)).astype(np.int8)); wgs = dev((rng.random(2 * I) * 0.01 + 0.001).astype(np.float16))
    gu = torch.empty(M, 2 * I, dtype=torch.float16, device=DEV)
    ops.rowwise_scaled_linear_cutlass_s4s4_unified(xq, xs, wg, wgs, None, gu)
    ref_act = ops.silu_mul(gu, torch.empty(M, I, dtype=torch.float16, device=DEV))
    act = ops.gate_up_silu_linear(xq, xs, wg, wgs, torch.empty(M, I, dtype=torch.float16, device=DEV))
    assert torch.equal(act.view(torch.int16), ref_act.view(torch.int16))
    # down_proj (K = 14336, 1024 threads) + residual
    x3_np, w3_np = oracle.pack_i4(rand_w4(rng, M, I)), rng.integers(-128, 128, (K, I // 2)).astype(np.int8)
    w3s_np = (rng.random(K) * 0.002 + 0.0005).astype(np.float16)
    resid_np = rand_hidden(rng, M, K)
    hid = dev(resid_np).clone()
    ops.rowwise_scaled_linear_s4s4_residual(dev(x3_np), xs, dev(w3_np), dev(w3s_np), hid, hid)
    assert np.array_equal(bits(host(hid)), bits(oracle.add_f16(resid_np, oracle.gemm_w4a4(x3_np, xs_np, w3_np, w3s_np))))


@pytest.mark.parametrize("M,N,K", [(20, 256, 8192), (32, 128, 5120), (31, 4096, 14336)])
def test_w4a4_two_token_tiles_other_k(ops, oracle, M, N, K):
    rng = np.random.default_rng(M + K)
    xq, xs = oracle.pack_i4(rand_w4(rng, M, K)), (rng.random(M) * 0.1 + 0.01).astype(np.float16)
    w = rng.integers(-128, 128, (N, K // 2)).astype(np.int8)
    ws = (rng.random(N) * 0.01 + 0.001).astype(np.float16)
    out = torch.full((M + 1, N), 3.0, dtype=torch.float16, device=DEV)
    ops.rowwise_scaled_linear_cutlass_s4s4_unified(dev(xq), dev(xs), dev(w), dev(ws), None, out[:M])
    assert np.array_equal(bits(host(out[:M])), bits(oracle.gemm_w4a4(xq, xs, w, ws)))
    assert torch.all(out[M] == 3.0)


# ------------------------------------------------------------------ attention, prompt-sized queries (64-row flash kernel)

@pytest.mark.parametrize("ctx_lens,q_lens,nq,nkv", [
    ([300], [300], 32, 8),                  # one full prompt, ragged last row block and last key chunk
    ([64, 129, 511], [64, 129, 511], 8, 2),  # several prompts of different lengths in one call
    ([400, 90], [150, 33], 32, 8),           # chunked prefill: queries are the tail of a longer context
    ([200], [200], 8, 8),                    # no GQA (group 1): 64 query tokens per workgroup
    ([1030], [1030], 16, 4),
])
def test_paged_attention_prompt_sized_queries_within_1e3(ops, oracle, ctx_lens, q_lens, nq, nkv):
    rng = np.random.default_rng(sum(ctx_lens) + nq)
    d, bs = 128, 16
    n_seqs = len(ctx_lens)
    bt, kc, vc = make_paged(rng, n_seqs, ctx_lens, nkv, d, bs)
    T = sum(q_lens)
    row = (nq + 2 * nkv) * d
    qkv = (rng.standard_normal((T, row)) * 0.5).astype(np.float16)
    q_start = np.concatenate([[0], np.cumsum(q_lens)]).astype(np.int32)
    ctx = np.array(ctx_lens, np.int32)
    scale = d ** -0.5
    ref = oracle.paged_attention(qkv[:, : nq * d], kc, vc, bt, ctx, q_start, scale)
    ws = torch.zeros(ops.paged_attention_workspace_bytes(n_seqs * max(q_lens), nq, d, 1), dtype=torch.uint8, device=DEV)
    out = torch.full((T + 1, nq * d), 5.0, dtype=torch.float16, device=DEV)
    ops.paged_attention(dev(qkv), row, dev(kc), dev(vc), dev(bt), dev(ctx), dev(q_start), T, max(q_lens), nq, scale, 1,
                        ws, out[:T])
    assert_close_1e3(host(out[:T]), ref)
    assert torch.all(out[T] == 5.0)
    # the un-merged form (single-split partials for the head-Hadamard launch) gives the same rows
    if nq in (32,) and len(set(q_lens)) == 1:
        ws2 = torch.zeros_like(ws)
        ops.paged_attention(dev(qkv), row, dev(kc), dev(vc), dev(bt), dev(ctx), dev(q_start), T, max(q_lens), nq, scale,
                            1, ws2, None)
        had_a = torch.empty(T, nq * d, dtype=torch.float16, device=DEV)
        ops.heads_hadamard_merged(ws2, n_seqs * max(q_lens), 1, T, nq, d, 0.1767, out_f16=had_a)
        had_b = torch.empty_like(had_a)
        ops.heads_hadamard(out[:T].contiguous(), 0.1767, out_f16=had_b, heads=nq)
        assert torch.equal(had_a.view(torch.int16), had_b.view(torch.int16))


@pytest.mark.parametrize("ctx_lens,q_len,n_splits,nq,nkv", [
    ([37, 130, 260, 515], 4, 1, 32, 8),      # one split over the whole context: 32-key slices over the four waves
    ([700], 6, 2, 32, 8),                    # verify with k = 5; a ragged last slice per split
    ([1500, 3000, 17], 1, 4, 32, 8),         # long contexts next to a sequence shorter than one slice
    ([333, 90], 2, 1, 64, 8),                # 64 heads, GQA group 8
])
def test_attention_partials_long_splits_then_merge_within_1e3(ops, oracle, ctx_lens, q_len, n_splits, nq, nkv):
    """Partials mode with splits that may exceed one 128-key chunk (the keys-over-waves kernel) + the merging head
    Hadamard, against the oracle's attention followed by the oracle's head Hadamard."""
    rng = np.random.default_rng(sum(ctx_lens) + q_len + nq)
    d, bs = 128, 16
    n_seqs = len(ctx_lens)
    bt, kc, vc = make_paged(rng, n_seqs, ctx_lens, nkv, d, bs)
    assert bt.shape[1] * bs > 128 * n_splits
    T = n_seqs * q_len
    row = (nq + 2 * nkv) * d
    qkv = (rng.standard_normal((T, row)) * 0.5).astype(np.float16)
    q_start = (np.arange(n_seqs + 1) * q_len).astype(np.int32)
    ctx = np.array(ctx_lens, np.int32)
    scale = d ** -0.5
    had_scale = oracle.rsqrt_scale(nq)
    ref = oracle.heads_hadamard(oracle.paged_attention(qkv[:, : nq * d], kc, vc, bt, ctx, q_start, scale), nq, had_scale)
    ws = torch.zeros(ops.paged_attention_workspace_bytes(T, nq, d, n_splits), dtype=torch.uint8, device=DEV)
    ops.paged_attention(dev(qkv), row, dev(kc), dev(vc), dev(bt), dev(ctx), dev(q_start), T, q_len, nq, scale, n_splits,
                        ws, None)
    out = torch.empty(T, nq * d, dtype=torch.float16, device=DEV)
    ops.heads_hadamard_merged(ws, T, n_splits, T, nq, d, had_scale, out_f16=out)
    # the head transform sums 32 / 64 attention outputs scaled by 1/sqrt(heads): errors of 1e-3 each stay below 1e-3 * sqrt(heads) / sqrt(heads)
    assert_close_1e3(host(out), ref)


@pytest.mark.skipif(not os.path.exists(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qspec_amd", "csrc",
                                                    "libqspec_hip_experimental.so")),
                    reason="experimental library not built (make -C qspec_amd/csrc experimental)")
@pytest.mark.parametrize("switch,kexpr", [("QSPEC_ATTN_FAST=0", "(long_splits_then_merge or reference_fixture_within) and not dev_forms"),
                                          ("QSPEC_ATTN_NW=8", "(long_splits_then_merge or reference_fixture_within) and not dev_forms"),
                                          ("QSPEC_QKV_LEVEL=1", "qkv and not dev_forms")],
                         ids=["attn_fast_0", "attn_nw_8", "qkv_level_1"])   # ids without the -k words: the child must not select THIS test
def test_attention_waves_kernel_dev_forms(switch, kexpr):
    """Forms that are built, measured and off against the same oracle comparisons as the
    defaults, re-run in a child process with the switch on (the library reads it once per process):
    paged_attention_waves_kernel's general per-lane table lookup instead of the two wave-uniform entries per slice, and its
    eight-wave form; the levelled qkv tiling (twelve RoPE pairs per workgroup, stream_common.cuh:qkv_pair) in the W4A16 and
    W4A4 qkv + RoPE + KV-write launches of this file."""
    import os
    import subprocess
    import sys
    from qspec_amd import _lib
    k, v = switch.split("=")
    env = dict(os.environ)
    env[k] = v
    env["QSPEC_HIP_LIB"] = _lib.EXPERIMENTAL_LIB_PATH   # dev knobs and rejected forms exist only in the experimental build
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-k", kexpr], env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert " passed" in r.stdout


def test_sample_top_k_top_p_reference_fixture(ops, oracle, golden_dir):
    """The non-greedy sampler front end (temperature, top-k, top-p, softmax, multinomial by exponential noise) on the GPU against
    the reference's own _apply_top_k_top_p / _multinomial run on CPU (tests/golden/sampling.npz).  Distinct logits: the kept
    set and the tokens exact, probabilities within 1e-6.  Equal logits: identical outside the boundary group, which is kept
    WHOLE here (the reference's unstable sort splits it arbitrarily); twice in a row on the self-cleaning workspace; and a
    greedy row (temperature 0) inside the batch takes the argmax."""
    g = np.load(os.path.join(golden_dir, "sampling.npz"))
    for name in ("distinct", "ties"):
        lg = g[name + "_logits"]
        T, V = lg.shape
        for rep in range(2):
            probs = torch.full((T, V), -1.0, dtype=torch.float32, device=DEV)
            tok = torch.full((T,), -1, dtype=torch.int64, device=DEV)
            ops.sample_top_k_top_p(dev(lg), probs, tok, dev(g[name + "_temperature"]), dev(g[name + "_top_k"]), dev(g[name + "_top_p"]),
                                   exponential=dev(g[name + "_E"]))
            pr, tk = host(probs), host(tok)
            rk, rp, rt = g[name + "_keep"], g[name + "_probs"], g[name + "_token"]
            assert np.allclose(pr.sum(1), 1.0, atol=1e-5)
            for t in range(T):
                kept = pr[t] > 0
                if name == "distinct":
                    assert np.array_equal(kept, rk[t]), (t, kept.sum(), rk[t].sum())
                    assert np.abs(pr[t] - rp[t]).max() <= 1e-6 and tk[t] == rt[t], t
                else:
                    b = lg[t][rk[t]].min()
                    off = lg[t] != b
                    assert np.array_equal(kept[off], rk[t][off]), t
                    assert kept[~off].all()                    # the boundary group as a whole
        ws = ops.sample_workspace(T, torch.device(DEV))
        assert int(ws[:T * 65536 * 4].view(torch.int32).abs().max().item()) == 0      # the histogram is left zeroed
    # a mixed batch: row 0 greedy (temperature 0), row 1 sampled; defaults (None) = temperature 1, no masking
    lg = g["distinct_logits"][:2]
    probs = torch.empty(2, lg.shape[1], dtype=torch.float32, device=DEV); tok = torch.empty(2, dtype=torch.int64, device=DEV)
    ops.sample_top_k_top_p(dev(lg), probs, tok, dev(np.array([0.0, 1.0], np.float32)), exponential=dev(g["distinct_E"][:2]))
    p0, t0 = oracle.softmax_argmax(lg)
    assert host(tok)[0] == t0[0] and np.array_equal(host(probs)[0], p0[0])
    pr, tk, _ = oracle.sample_top_k_top_p(lg, np.array([0.0, 1.0], np.float32), None, None, g["distinct_E"][:2])
    assert np.array_equal(host(tok), tk) and np.abs(host(probs) - pr).max() <= 1e-7
    # Philox path: a valid distribution, a token inside the kept set, and a new draw on every call
    rng = torch.tensor([123, 0], dtype=torch.int64, device=DEV)
    seen = set()
    for _ in range(8):
        ops.sample_top_k_top_p(dev(g["distinct_logits"][1:2]), probs[:1], tok[:1], dev(np.array([0.7], np.float32)),
                               dev(np.array([50], np.int32)), rng_state=rng)
        assert host(probs)[0][int(host(tok)[0])] > 0
        seen.add(int(host(tok)[0]))
    assert int(rng[1].item()) == 8 and len(seen) > 1


def test_sample_top_k_top_p_edge_rows_and_full_vocabulary(ops, oracle):
    """Edge rows against the oracle (whose rule is the reference's, test_oracle_golden.py): a uniform row of 1003 tokens (every
    logit equal: one group of V tokens -- kept whole whatever top-k / top-p say; the 131080-token one, a 128 k count in one
    histogram bin, is a row of the selection matrix, test_sampling_cases_gpu.py), a row at the fp16 ceiling, -inf logits (never kept), top_k = 1, top_p -> 0, a vocabulary that is no multiple of 8; then the full Llama-3
    vocabulary at 16 rows (the verify pass's shape) with DISTINCT-per-row-ordering logits: kept sets equal, tokens equal."""
    rng = np.random.default_rng(5)
    V = 1003
    lg = (rng.standard_normal((6, V)) * 3).astype(np.float16)
    lg[0] = np.float16(0.25)                                  # uniform
    lg[1, 17] = np.float16(60000.0)                           # the fp16 ceiling: everything else underflows
    lg[2, ::3] = -np.inf                                      # masked-out tokens of a previous stage
    temp = np.array([1.0, 1.0, 0.8, 1.0, 1.5, 0.6], np.float32)
    top_k = np.array([5, -1, 40, 1, -1, 900], np.int32)
    top_p = np.array([0.3, 0.9, 0.95, 1.0, 1e-6, 0.999], np.float32)
    E = rng.exponential(1.0, (6, V)).astype(np.float32)
    probs = torch.empty(6, V, dtype=torch.float32, device=DEV); tok = torch.empty(6, dtype=torch.int64, device=DEV)
    ops.sample_top_k_top_p(dev(lg), probs, tok, dev(temp), dev(top_k), dev(top_p), exponential=dev(E))
    pr, tk = host(probs), host(tok)
    assert np.allclose(pr.sum(1), 1.0, atol=1e-5) and not np.isnan(pr).any()
    assert (pr[0] > 0).all() and np.allclose(pr[0], 1.0 / V, rtol=1e-5)             # the uniform group stays whole
    assert pr[1, 17] == 1.0 and tk[1] == 17
    assert (pr[2, ::3] == 0).all()
    assert (pr[3] > 0).sum() == (lg[3] == lg[3].max()).sum() and lg[3][tk[3]] == lg[3].max()      # top_k = 1 (+ ties)
    assert (pr[4] > 0).sum() == (lg[4] == lg[4].max()).sum()                         # top_p -> 0: the top group only
    po, to, keep = oracle.sample_top_k_top_p(lg, temp, top_k, top_p, E)
    for t in (1, 2, 5):                                       # rows whose boundary group is a single token: the oracle's rule exactly
        b = lg[t][keep[t]].min()
        if (lg[t] == b).sum() == 1:
            assert np.array_equal(pr[t] > 0, keep[t]) and tk[t] == to[t], t
    # the full vocabulary, 16 rows
    V, T = 128256, 16
    base = np.linspace(-12, 12, 60000).astype(np.float16)
    base = np.unique(base)                                     # ~50 k distinct fp16 values: ties are unavoidable at V = 128 k
    lg = np.stack([base[rng.integers(0, base.size, V)] for _ in range(T)])
    temp = rng.uniform(0.5, 1.5, T).astype(np.float32); top_k = rng.integers(1, 200, T).astype(np.int32)
    top_p = rng.uniform(0.5, 1.0, T).astype(np.float32)
    E = rng.exponential(1.0, (T, V)).astype(np.float32)
    probs = torch.empty(T, V, dtype=torch.float32, device=DEV); tok = torch.empty(T, dtype=torch.int64, device=DEV)
    ops.sample_top_k_top_p(dev(lg), probs, tok, dev(temp), dev(top_k), dev(top_p), exponential=dev(E))
    pr, tk = host(probs), host(tok)
    po, to, keep = oracle.sample_top_k_top_p(lg, temp, top_k, top_p, E)
    assert np.allclose(pr.sum(1), 1.0, atol=1e-5)
    for t in range(T):
        b = lg[t][keep[t]].min()
        off = lg[t] != b
        assert np.array_equal((pr[t] > 0)[off], keep[t][off]) and (pr[t] > 0)[~off].all(), t
        if np.array_equal(pr[t] > 0, keep[t]):
            assert tk[t] == to[t] and np.abs(pr[t] - po[t]).max() <= 1e-6, t


def test_typical_acceptance_sampler_reference_fixture(ops, oracle, golden_dir):
    """TypicalAcceptanceSampler on the GPU against the REFERENCE class run on CPU (tests/golden/typical_acceptance.npz, 20
    deterministic cases): output layout, accept masks, counters exact; the replacement token = the target's argmax; through
    the class with the reference's call surface, with strided draft ids and an inactive row."""
    from qspec_amd.spec_decode import TypicalAcceptanceSampler
    g = np.load(os.path.join(golden_dir, "typical_acceptance.npz"))
    for i in range(int(g["cases"])):
        thr, alpha = (float(v) for v in g[f"t{i}_params"])
        tq, ids, bonus = g[f"t{i}_tq"], g[f"t{i}_ids"], g[f"t{i}_bonus"]
        B, k = ids.shape
        s = TypicalAcceptanceSampler(thr, alpha)
        s.init_gpu_tensors(DEV)
        acc = torch.empty(B, k, dtype=torch.uint8, device=DEV); rec = torch.empty(B, k, dtype=torch.int64, device=DEV)
        ids_kb = dev(np.ascontiguousarray(ids.T))                      # step-major draft ids, as the engine holds them
        out = s(dev(tq), dev(bonus), None, ids_kb.transpose(0, 1), accepted=acc, recovered=rec)
        torch.cuda.synchronize()
        assert np.array_equal(host(out), g[f"t{i}_out"]), i
        assert np.array_equal(host(acc).astype(bool), g[f"t{i}_accepted"]), i
        assert s.counters.tolist() == list(g[f"t{i}_counters"]), i
        assert np.array_equal(host(rec), tq[:, :-1].argmax(-1)), i
        o2, a2, r2, c2, _ = oracle.typical_acceptance_sample(tq, bonus, ids, thr, alpha)
        assert np.array_equal(host(out), o2) and np.array_equal(host(acc).astype(bool), a2)
    # an empty batch slot emits nothing and is not counted
    tq, ids, bonus = g["t8_tq"], g["t8_ids"], g["t8_bonus"]
    B, k = ids.shape
    s = TypicalAcceptanceSampler(*(float(v) for v in g["t8_params"]))
    s.init_gpu_tensors(DEV)
    lens = torch.ones(B, dtype=torch.int32, device=DEV); lens[3] = 0
    out = s(dev(tq), dev(bonus), None, dev(ids), active_lens=lens)
    ref = g["t8_out"].copy(); ref[3] = -1
    assert np.array_equal(host(out), ref) and int(s.counters[2]) == (B - 1) * k


# ------------------------------------------------------------------ the reference's own pure-torch formulas (fixtures)
# tests/golden/{attention,rope_cache_softmax}.npz: outputs of ref_paged_attn (tests/kernels/test_flash_attn.py:19-75),
# RotaryEmbedding.forward_native (rotary_embedding.py:201-229), the reshape_and_cache_flash reference loop
# (tests/kernels/test_cache.py:295-304) and torch.softmax / log_softmax / argmax (sampler.py:278-287), produced by
# tests/golden/make_golden.py from /root/reference.  The HIP kernels run on the same inputs.

@pytest.mark.parametrize("idx", [0, 1, 2])
@pytest.mark.parametrize("n_splits", [1, 3])
def test_paged_attention_reference_fixture_within_1e3(ops, golden_dir, idx, n_splits):
    from test_oracle_golden import attention_case
    c = attention_case(np.load(os.path.join(golden_dir, "attention.npz")), idx)
    nb, bs, nkv, d = c["key_cache"].shape
    T = c["q"].shape[0]
    nq = c["q"].shape[1] // d
    q_lens = np.diff(c["q_start"])
    ws = torch.zeros(ops.paged_attention_workspace_bytes(len(q_lens) * int(q_lens.max()), nq, d, n_splits),
                     dtype=torch.uint8, device=DEV)
    out = torch.empty(T, nq * d, dtype=torch.float16, device=DEV)
    ops.paged_attention(dev(c["q"]), nq * d, dev(c["key_cache"]), dev(c["value_cache"]), dev(c["block_tables"]),
                        dev(c["ctx_lens"]), dev(c["q_start"]), T, int(q_lens.max()), nq, c["scale"], n_splits, ws, out)
    got = host(out).astype(np.float64)
    assert np.abs(got - c["ref32"]).max() <= 1e-3, np.abs(got - c["ref32"]).max()
    assert np.allclose(got, c["ref16"].astype(np.float64), atol=2e-2, rtol=1e-2)   # the reference test's own bar


@pytest.mark.parametrize("idx", [0, 1])
def test_rope_reference_fixture_bit_exact(ops, golden_dir, idx):
    from qspec_amd.model import make_cos_sin_cache
    g = np.load(os.path.join(golden_dir, "rope_cache_softmax.npz"))
    key = f"rope{idx}_"
    d, max_pos, nq, nkv = (int(v) for v in g[key + "cfg"])
    cs = make_cos_sin_cache(d, max_pos, float(g[key + "base"])).to(DEV)      # the table the product builds
    q, k = dev(g[key + "q"]), dev(g[key + "k"])
    ops.rotary_embedding(dev(g[key + "pos"]), q, k, d, cs)
    assert np.array_equal(bits(host(q)), bits(g[key + "q_out"]))
    assert np.array_equal(bits(host(k)), bits(g[key + "k_out"]))


def test_reshape_and_cache_flash_reference_fixture_bit_exact(ops, golden_dir):
    _reshape_and_cache_fixture_check(ops, golden_dir, 16)


@pytest.mark.parametrize("bs", [8, 32])
def test_reshape_and_cache_flash_reference_fixture_bit_exact_block_sizes(ops, golden_dir, bs):
    _reshape_and_cache_fixture_check(ops, golden_dir, bs)


def _reshape_and_cache_fixture_check(ops, golden_dir, bs):
    """The fixture's cache (6 blocks of 16) viewed at block size 8 / 32: a slot is the same row of the flash layout
    [num_blocks, block_size, n_kv, d] at every block size, so the expected cache is the fixture's, re-viewed."""
    g = np.load(os.path.join(golden_dir, "rope_cache_softmax.npz"))
    nb, bs0, nkv, d = g["cache_key_cache_in"].shape
    assert (nb * bs0) % bs == 0
    view = lambda a: a.reshape(nb * bs0 // bs, bs, nkv, d)  # noqa: E731
    kc, vc = dev(view(g["cache_key_cache_in"])), dev(view(g["cache_value_cache_in"]))
    ops.reshape_and_cache_flash(dev(g["cache_key"]), dev(g["cache_value"]), kc, vc, dev(g["cache_slot_mapping"]))
    assert np.array_equal(bits(host(kc)), bits(view(g["cache_key_cache_out"])))
    assert np.array_equal(bits(host(vc)), bits(view(g["cache_value_cache_out"])))


def test_softmax_argmax_reference_fixture(ops, golden_dir):
    g = np.load(os.path.join(golden_dir, "rope_cache_softmax.npz"))
    logits = g["sm_logits"]
    T, V = logits.shape
    probs = torch.empty(T, V, dtype=torch.float32, device=DEV)
    tok = torch.empty(T, dtype=torch.int64, device=DEV)
    ops.softmax_argmax(dev(logits), probs, tok)
    ref = g["sm_probs"].astype(np.float64)
    got = host(probs)
    assert np.array_equal(host(tok), g["sm_argmax"])
    assert np.abs(got - ref).max() <= 1e-3
    big = ref > 1e-30
    assert (np.abs(got[big] - ref[big]) / ref[big]).max() < 1e-5
