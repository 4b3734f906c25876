// extern "C" boundary: argument checks, error strings, launch-error capture.
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/qspec_hip.h"
#include "kernels.h"

using qspec::f16;

static thread_local char g_err[512] = "";

static int fail(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return 1;
}
static int finish(const char* op, int rc) {
    if (rc == -10) return fail("%s: the experimental LDS-DMA QKV variants (QSPEC_SDMA) write fp16 caches only: no fp8 form", op);
    if (rc != 0) return fail("%s: unsupported shape/arguments (code %d)", op, rc);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail("%s: launch failed: %s", op, hipGetErrorString(e));
    return 0;
}
#define NONNULL(op, p) \
    if (!(p)) return fail("%s: argument `%s` is NULL", op, #p)
#define ST ((hipStream_t)stream)
#define H(p) reinterpret_cast<f16*>(p)
#define CH(p) reinterpret_cast<const f16*>(p)

// QSPEC_OLD_GEMM=1 keeps the first-generation one-tile-per-workgroup W4A4 kernel (A/B measurements)
static bool use_stream() {
    static const int old = QS_DEV_KNOB("QSPEC_OLD_GEMM", 0);
    return old != 1;
}
// smallest M routed to the M-tiled W4A16 kernel (gemm_tiled.hip); QSPEC_TILED_MIN_M overrides (0 disables)
static int tiled_min_m() {
    // (33 until round 4: 17..32 rows ran the 2-D kernel of gemm.hip -- 70B gate_up at 32 rows 83.8 us)
    static const int v = QS_DEV_KNOB("QSPEC_TILED_MIN_M", 17);
    return v <= 0 ? (1 << 30) : v;
}

// Several entry points are one op in more than one form: `_xp` (fragment-major activation tiles between the verify pass's
// producers and its W4A16 GEMMs), `_kv8` (FP8 e4m3 KV cache: the cache pointers address bytes), `_seeded`, `_min_p`,
// `_constrained`, `_embed`.  Such an op has ONE body in the anonymous namespace below; what tells the forms apart arrives as
// ordinary arguments -- `op` (the name of the entry that was called, for error strings), `xp`, `kq`, or a flag saying that the
// entry has the optional arrays -- and every entry is a single call of its op's body.  Nothing but g_err is file-scope state.

// A `_kv8` entry checks its scales and builds the KvQuant its body hands to the kernels: the inverses are computed here, once,
// on the host, in fp32.
#define KV_SCALES(op)                                                                                                \
    if (!(k_scale > 0.0f && k_scale < __builtin_inff() && v_scale > 0.0f && v_scale < __builtin_inff()))             \
        return fail("%s: k_scale=%g, v_scale=%g must be positive and finite", op, (double)k_scale, (double)v_scale); \
    const qspec::KvQuant kq{1, k_scale, v_scale, 1.0f / k_scale, 1.0f / v_scale}

// shape queries that entries ask as well (the extern "C" queries of the same names return these)
static int w4a16_act_layout32_supported(int M, int N, int K) { return use_stream() && qspec::gemm_w4a16_stream32_supported(M, N, K) ? 1 : 0; }
static int w4a16_linear_partial_slices_xp32(int M, int N, int K) { return use_stream() ? qspec::gemm_w4a16_stream32_partial_slices(M, N, K) : 0; }
static int heads_hadamard_merged_spread_supported(int tokens, int heads, int head_dim) {
    return tokens >= 0 && tokens * 8 <= 1024 && heads == 32 && head_dim == 128;
}
static int w4a16_linear_partial_slices(int M, int N, int K) {
    if (M > 16)   // the M-tiled kernel's launch plan (narrow layers at a few dozen to a few hundred tokens)
        return M >= tiled_min_m() ? qspec::gemm_w4a16_tiled_partial_slices(M, N, K) : 0;
    return use_stream() ? qspec::gemm_w4a16_stream_partial_slices(M, N, K) : 0;
}

namespace {

int add_rms_norm_fp16(const char* op, int xp, qspec_half* out, qspec_half* hidden_out, const qspec_half* x,
                      const qspec_half* delta, float eps, int tokens, int hidden, void* stream) {
    if (tokens < 0) return fail("%s: tokens < 0", op);
    if (tokens == 0) return 0;
    NONNULL(op, out); NONNULL(op, x);
    if (delta) NONNULL(op, hidden_out);
    if (hidden % 1024 || hidden > 8192 || hidden <= 0) return fail("%s: hidden=%d must be a multiple of 1024, <= 8192", op, hidden);
    if (xp && tokens > 32) return fail("%s: the fragment-major layout is one or two 16-row tiles (tokens=%d)", op, tokens);
    return finish(op, qspec::ln_fp16(CH(x), CH(delta), H(hidden_out), H(out), eps, tokens, hidden, ST, xp));
}
int add_rms_norm_fp16_partial(const char* op, int xp, qspec_half* out, qspec_half* hidden_out, const qspec_half* x,
                              const float* part, const qspec_half* ws, int slices, float eps, int tokens, int hidden,
                              void* stream) {
    if (tokens < 0) return fail("%s: tokens < 0", op);
    if (tokens == 0) return 0;
    NONNULL(op, out); NONNULL(op, x); NONNULL(op, part); NONNULL(op, ws); NONNULL(op, hidden_out);
    if (slices < 1) return fail("%s: slices < 1", op);
    if (hidden % 1024 || hidden > 8192 || hidden <= 0) return fail("%s: hidden=%d must be a multiple of 1024, <= 8192", op, hidden);
    if (xp && tokens > 32) return fail("%s: the fragment-major layout is one or two 16-row tiles (tokens=%d)", op, tokens);
    return finish(op, qspec::ln_fp16_partial(CH(x), part, CH(ws), slices, H(hidden_out), H(out), eps, tokens, hidden, ST, xp));
}
int heads_hadamard_merged(const char* op, int xp, const void* attn_workspace, int max_tokens, int n_splits, qspec_half* out_f16,
                          int8_t* q, qspec_half* scale, float had_scale, float clip_ratio, int tokens, int heads, int head_dim,
                          void* stream) {
    if (tokens < 0) return fail("%s: tokens < 0", op);
    if (tokens == 0) return 0;
    NONNULL(op, attn_workspace);
    if (q) { NONNULL(op, scale); } else { NONNULL(op, out_f16); }
    if (!((head_dim == 128 && (heads == 32 || heads == 64)) || (heads == 32 && head_dim % 8 == 0 && head_dim >= 8 && head_dim <= 256)))
        return fail("%s: built for 32 / 64 heads of 128 and 32 heads of another size %% 8 == 0 (got %d x %d)", op, heads, head_dim);
    if (xp && (q || !(heads == 32 || heads == 64) || tokens > 32 || head_dim != 128))
        return fail("%s: the fragment-major fp16 output exists for 32 / 64 heads of 128, <= 32 tokens, no quantiser", op);
    return finish(op, qspec::heads_hadamard_merge((const float*)attn_workspace, max_tokens, n_splits, H(out_f16), q, H(scale), had_scale, clip_ratio, tokens, heads, head_dim, ST, xp));
}
int heads_hadamard_mix_merged_spread(const char* op, int xp, const void* attn_workspace, int max_tokens, int n_splits,
                                     const qspec_half* hadK, int K, qspec_half* out_f16, float* part_amax, float had_scale,
                                     int tokens, int heads, int head_dim, void* stream) {
    if (tokens < 0) return fail("%s: tokens < 0", op);
    if (tokens == 0) return 0;
    NONNULL(op, attn_workspace); NONNULL(op, hadK); NONNULL(op, out_f16);
    if (!qspec::heads_hadamard_mix_merge_spread_supported(tokens, heads, head_dim, K))
        return fail("%s: needs head_dim 128, heads = K * 2^p <= 64 with 2 <= K <= 172, at most 128 tokens (got %d x %d, K = %d, %d tokens)",
                    op, heads, head_dim, K, tokens);
    if (xp && (part_amax || tokens > 32)) return fail("%s: the fragment-major fp16 output: <= 32 tokens, no part_amax", op);
    return finish(op, qspec::heads_hadamard_mix_merge_spread((const float*)attn_workspace, max_tokens, n_splits, CH(hadK), H(out_f16),
                                                             part_amax, had_scale, tokens, heads, head_dim, K, ST, xp));
}
int mlp_hadamard(const char* op, int xp, const qspec_half* act, const qspec_half* hadK, qspec_half* out_f16, int8_t* q,
                 qspec_half* scale, float had_scale, float clip_ratio, int tokens, int intermediate, int K, void* workspace,
                 void* stream) {
    if (tokens < 0) return fail("%s: tokens < 0", op);
    if (tokens == 0) return 0;
    NONNULL(op, act);
    if (K > 1) NONNULL(op, hadK);
    if (q) { NONNULL(op, scale); } else { NONNULL(op, out_f16); }
    if (intermediate % 8) return fail("%s: intermediate %% 8 != 0", op);
    if (xp && (q || tokens > 32))
        return fail("%s: the fragment-major fp16 output: <= 32 tokens, no quantiser", op);
    return finish(op, qspec::silu_mul_hadamard(CH(act), CH(hadK), H(out_f16), q, H(scale), had_scale, clip_ratio, tokens, intermediate, K, 1, workspace, ST, xp));
}
int w4a16_linear(const char* op, int xp, const qspec_half* x, const int8_t* wq, const qspec_half* ws, const qspec_half* bias,
                 qspec_half* out, int M, int N, int K, void* workspace, void* stream) {
    if (M < 0 || N < 0) return fail("%s: negative size", op);
    if (M == 0 || N == 0) return 0;
    NONNULL(op, x); NONNULL(op, wq); NONNULL(op, ws); NONNULL(op, out);
    if (N % 16 || K % 128 || K <= 0) return fail("%s: need N %% 16 == 0 and K %% 128 == 0 (N=%d K=%d)", op, N, K);
    if (xp && !(!bias && use_stream() && qspec::gemm_w4a16_stream_supported(M, N, K) && qspec::gemm_w4a16_xperm_supported(M, K)))
        return fail("%s: no fragment-major form for (M=%d N=%d K=%d): ask qspec_w4a16_act_layout_supported", op, M, N, K);
    if (!bias && use_stream() && qspec::gemm_w4a16_stream_supported(M, N, K))
        return finish(op, qspec::gemm_w4a16_stream(CH(x), 0, wq, 0, CH(ws), H(out), M, N, K, ST, xp));
    // long K (down_proj): K slices of a built length, raw sums in the workspace (behind its ticket counters), finish
    const int S = (!bias && use_stream() && workspace) ? qspec::gemm_w4a16_stream_partial_slices(M, N, K) : 0;
    if (S > 0 && (size_t)S * M * N * sizeof(float) + 8192 <= qspec::gemm_w4a16_ws_bytes()) {
        float* part = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + 8192);
        int rc = qspec::gemm_w4a16_stream_partial(CH(x), 0, wq, 0, part, M, N, K, S, ST);
        if (rc == 0) rc = qspec::gemm_w4a16_partial_finish(part, CH(ws), H(out), M, N, S, ST);
        return finish(op, rc);
    }
    if (!bias && M >= tiled_min_m() && qspec::gemm_w4a16_tiled_supported(M, N, K))   // prefill-sized M: M-tiled kernel
        return finish(op, qspec::gemm_w4a16_tiled(CH(x), wq, CH(ws), H(out), M, N, K,
                                                  workspace ? reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + 8192) : nullptr,
                                                  workspace ? qspec::gemm_w4a16_ws_bytes() - 8192 : 0, ST));
    return finish(op, qspec::gemm_w4a16(CH(x), wq, CH(ws), CH(bias), H(out), M, N, K, workspace, ST));
}
int w4a16_linear_partial(const char* op, int xp, const qspec_half* x, const int8_t* wq, float* part, int M, int N, int K,
                         int slices, void* stream) {
    if (M == 0 || N == 0) return 0;
    NONNULL(op, x); NONNULL(op, wq); NONNULL(op, part);
    if (M > 16) {
        if (xp) return fail("%s: the fragment-major layout is a 16-row tile (M=%d)", op, M);
        if (slices < 2 || slices != w4a16_linear_partial_slices(M, N, K))
            return fail("%s: (M=%d N=%d K=%d) takes %d slices (qspec_w4a16_linear_partial_slices), got %d", op, M, N, K,
                        w4a16_linear_partial_slices(M, N, K), slices);
        return finish(op, qspec::gemm_w4a16_tiled_partial(CH(x), wq, part, M, N, K, slices, ST));
    }
    // the planned count (qspec_w4a16_linear_partial_slices), or -- for shapes that also run unsliced -- any count whose
    // slices the streaming kernel takes (the verify pass's o_proj experiment)
    const int planned = qspec::gemm_w4a16_stream_partial_slices(M, N, K);
    if (slices < 2 || slices > 8 || K % slices || (planned ? slices != planned : !qspec::gemm_w4a16_stream_supported(M, N, K / slices)))
        return fail("%s: (M=%d N=%d K=%d) takes %d slices (qspec_w4a16_linear_partial_slices), got %d", op, M, N, K, planned, slices);
    if (xp && !qspec::gemm_w4a16_xperm_supported(M, K / slices)) return fail("%s: no fragment-major form for slices of %d", op, K / slices);
    return finish(op, qspec::gemm_w4a16_stream_partial(CH(x), 0, wq, 0, part, M, N, K, slices, ST, xp));
}
int gate_up_silu_linear_w4a16(const char* op, int xp, const qspec_half* x, const int8_t* wq, const qspec_half* ws,
                              qspec_half* act, int M, int intermediate, int K, void* workspace, void* stream) {
    if (M == 0) return 0;
    NONNULL(op, x); NONNULL(op, wq); NONNULL(op, ws); NONNULL(op, act);
    if (xp && !(use_stream() && qspec::gemm_w4a16_stream_supported(M, 2 * intermediate, K) && qspec::gemm_w4a16_xperm_supported(M, K)))
        return fail("%s: no fragment-major form for (M=%d I=%d K=%d)", op, M, intermediate, K);
    if (use_stream() && qspec::gemm_w4a16_stream_supported(M, 2 * intermediate, K))
        return finish(op, qspec::gemm_w4a16_stream_gate_up_silu(CH(x), wq, CH(ws), H(act), M, intermediate, K, 0, intermediate, ST, xp));
    return finish(op, qspec::gemm_w4a16_gate_up_silu(CH(x), wq, CH(ws), H(act), M, intermediate, K, 0, intermediate, workspace, ST));
}
int qkv_rope_linear_w4a16(const char* op, int xp, const qspec::KvQuant& kq, const qspec_half* x, const int8_t* wq,
                          const qspec_half* ws, qspec_half* qkv, int M, int N, int K, const int64_t* positions,
                          const qspec_half* cos_sin_cache, void* key_cache, void* value_cache, const int64_t* slot_mapping,
                          int num_heads, int num_kv_heads, int head_size, int rot_dim, void* workspace, void* stream) {
    if (M == 0) return 0;
    NONNULL(op, x); NONNULL(op, wq); NONNULL(op, ws); NONNULL(op, qkv); NONNULL(op, positions);
    NONNULL(op, cos_sin_cache); NONNULL(op, key_cache); NONNULL(op, value_cache); NONNULL(op, slot_mapping);
    if ((head_size != 128 && head_size != 64) || rot_dim != head_size) return fail("%s: head_size = rot_dim = 128 or 64 only", op);
    if (head_size == 64 && !(use_stream() && qspec::gemm_w4a16_stream_supported(M, N, K)))
        return fail("%s: head_size 64 exists on the streaming kernel only (M=%d N=%d K=%d): ask qspec_qkv_rope_linear_supported", op, M, N, K);
    if (xp && !(use_stream() && qspec::gemm_w4a16_stream_supported(M, N, K) && qspec::gemm_w4a16_xperm_supported(M, K)))
        return fail("%s: no fragment-major form for (M=%d N=%d K=%d)", op, M, N, K);
    if (use_stream() && qspec::gemm_w4a16_stream_supported(M, N, K))
        return finish(op, qspec::gemm_w4a16_stream_qkv_rope(CH(x), wq, CH(ws), H(qkv), M, N, K, positions, CH(cos_sin_cache), H(key_cache), H(value_cache), slot_mapping, num_heads, num_kv_heads, head_size, rot_dim, ST, xp, kq));
    return finish(op, qspec::gemm_w4a16_qkv_rope(CH(x), wq, CH(ws), H(qkv), M, N, K, positions, CH(cos_sin_cache), H(key_cache), H(value_cache), slot_mapping, num_heads, num_kv_heads, head_size, rot_dim, workspace, ST, kq));
}
int qkv_rope_linear_w4a16_xp32(const char* op, const qspec::KvQuant& kq, const qspec_half* x, const int8_t* wq,
                               const qspec_half* ws, qspec_half* qkv, int M, int N, int K, const int64_t* positions,
                               const qspec_half* cos_sin_cache, void* key_cache, void* value_cache, const int64_t* slot_mapping,
                               int num_heads, int num_kv_heads, int head_size, int rot_dim, void* stream) {
    if (M == 0) return 0;
    NONNULL(op, x); NONNULL(op, wq); NONNULL(op, ws); NONNULL(op, qkv); NONNULL(op, positions);
    NONNULL(op, cos_sin_cache); NONNULL(op, key_cache); NONNULL(op, value_cache); NONNULL(op, slot_mapping);
    if ((head_size != 128 && head_size != 64) || rot_dim != head_size) return fail("%s: head_size = rot_dim = 128 or 64 only", op);
    if (!w4a16_act_layout32_supported(M, N, K))
        return fail("%s: no two-tile streaming form for (M=%d N=%d K=%d)", op, M, N, K);
    return finish(op, qspec::gemm_w4a16_stream32_qkv_rope(CH(x), wq, CH(ws), H(qkv), M, N, K, positions, CH(cos_sin_cache), H(key_cache), H(value_cache), slot_mapping, num_heads, num_kv_heads, head_size, rot_dim, ST, kq));
}
int qkv_rope_linear_s4s4(const char* op, const qspec::KvQuant& kq, const int8_t* xq, const qspec_half* xs, const int8_t* wq,
                         const qspec_half* ws, qspec_half* qkv, int M, int N, int K, const int64_t* positions,
                         const qspec_half* cos_sin_cache, void* key_cache, void* value_cache, const int64_t* slot_mapping,
                         int num_heads, int num_kv_heads, int head_size, int rot_dim, void* stream) {
    if (M == 0) return 0;
    NONNULL(op, xq); NONNULL(op, xs); NONNULL(op, wq); NONNULL(op, ws); NONNULL(op, qkv); NONNULL(op, positions);
    NONNULL(op, cos_sin_cache); NONNULL(op, key_cache); NONNULL(op, value_cache); NONNULL(op, slot_mapping);
    if ((head_size != 128 && head_size != 64) || rot_dim != head_size) return fail("%s: head_size = rot_dim = 128 or 64 only", op);
    if (head_size == 64 && !(use_stream() && qspec::gemm_w4a4_stream_supported(M, N, K, false)))
        return fail("%s: head_size 64 exists on the streaming kernel only (M=%d N=%d K=%d): ask qspec_qkv_rope_linear_supported", op, M, N, K);
    if (use_stream() && qspec::gemm_w4a4_stream_supported(M, N, K, false)) {
        qspec::StreamActs x;
        x.xq = xq; x.xs = CH(xs);
        return finish(op, qspec::gemm_w4a4_stream_qkv_rope(x, wq, CH(ws), H(qkv), M, N, K, positions, CH(cos_sin_cache), H(key_cache), H(value_cache), slot_mapping, num_heads, num_kv_heads, head_size, rot_dim, ST, kq));
    }
    return finish(op, qspec::gemm_w4a4_qkv_rope(xq, CH(xs), wq, CH(ws), H(qkv), M, N, K, positions, CH(cos_sin_cache), H(key_cache), H(value_cache), slot_mapping, num_heads, num_kv_heads, head_size, rot_dim, ST, kq));
}
int ln_qkv_rope_linear_s4s4(const char* op, const qspec::KvQuant& kq, const qspec_half* hidden_in, const qspec_half* delta,
                            qspec_half* hidden_out, float eps, const int8_t* wq, const qspec_half* ws, qspec_half* qkv, int M,
                            int N, int K, const int64_t* positions, const qspec_half* cos_sin_cache, void* key_cache,
                            void* value_cache, const int64_t* slot_mapping, int num_heads, int num_kv_heads, int head_size,
                            int rot_dim, void* sync_workspace, void* stream) {
    if (M == 0) return 0;
    NONNULL(op, hidden_in); NONNULL(op, wq); NONNULL(op, ws); NONNULL(op, qkv); NONNULL(op, positions);
    NONNULL(op, cos_sin_cache); NONNULL(op, key_cache); NONNULL(op, value_cache); NONNULL(op, slot_mapping);
    if (hidden_out == hidden_in) return fail("%s: hidden_out must not alias hidden_in (every workgroup reads it)", op);
    if ((head_size != 128 && head_size != 64) || rot_dim != head_size) return fail("%s: head_size = rot_dim = 128 or 64 only", op);
    if (!qspec::gemm_w4a4_stream_supported(M, N, K, true))
        return fail("%s: need M <= 16, N %% 16 == 0, K in {1024, 2048, 4096, 5120, 8192} (M=%d N=%d K=%d)", op, M, N, K);
    qspec::StreamActs x;
    x.hidden_in = CH(hidden_in); x.delta = CH(delta); x.hidden_out = H(hidden_out); x.eps = eps;
    x.sync = reinterpret_cast<int*>(sync_workspace);
    return finish(op, qspec::gemm_w4a4_stream_qkv_rope(x, wq, CH(ws), H(qkv), M, N, K, positions, CH(cos_sin_cache), H(key_cache), H(value_cache), slot_mapping, num_heads, num_kv_heads, head_size, rot_dim, ST, kq));
}
int reshape_and_cache_flash(const char* op, const qspec::KvQuant& kq, const qspec_half* key, const qspec_half* value,
                            void* key_cache, void* value_cache, const int64_t* slot_mapping, int tokens, int num_kv_heads,
                            int head_size, int64_t key_stride, int64_t value_stride, void* stream) {
    if (tokens == 0) return 0;
    NONNULL(op, key); NONNULL(op, value); NONNULL(op, key_cache); NONNULL(op, value_cache); NONNULL(op, slot_mapping);
    return finish(op, qspec::reshape_and_cache_flash(CH(key), CH(value), H(key_cache), H(value_cache), slot_mapping, tokens, num_kv_heads, head_size, key_stride, value_stride, ST, kq));
}
int rope_kv_write(const char* op, const qspec::KvQuant& kq, const int64_t* positions, qspec_half* qkv,
                  const qspec_half* cos_sin_cache, void* key_cache, void* value_cache, const int64_t* slot_mapping, int tokens,
                  int num_heads, int num_kv_heads, int head_size, int rot_dim, void* stream) {
    if (tokens == 0) return 0;
    NONNULL(op, positions); NONNULL(op, qkv); NONNULL(op, cos_sin_cache); NONNULL(op, key_cache); NONNULL(op, value_cache); NONNULL(op, slot_mapping);
    return finish(op, qspec::rope_kv_write(positions, H(qkv), CH(cos_sin_cache), H(key_cache), H(value_cache), slot_mapping, tokens, num_heads, num_kv_heads, head_size, rot_dim, ST, kq));
}
int paged_attention(const char* op, const qspec::KvQuant& kq, const qspec_half* q, int64_t q_stride, const void* key_cache,
                    const void* value_cache, const int32_t* block_tables, int max_blocks_per_seq, const int32_t* ctx_lens,
                    const int32_t* q_start, int n_seqs, int tokens, int max_q_len, int num_heads, int num_kv_heads,
                    int head_size, int block_size, float sm_scale, int n_splits, void* workspace, qspec_half* out,
                    void* stream) {
    if (n_seqs == 0 || tokens == 0) return 0;
    NONNULL(op, q); NONNULL(op, key_cache); NONNULL(op, value_cache); NONNULL(op, block_tables); NONNULL(op, ctx_lens);
    NONNULL(op, q_start); NONNULL(op, workspace);   /* out == NULL: partials only, see qspec_heads_hadamard_merged */
    if (head_size != 128 && (head_size > 256 || head_size % 2 || (!out && head_size % 8)))
        return fail("%s: head_size=%d: the matrix-core kernel is built for 128; other even sizes <= 256 run the generic kernel (partials, out = NULL: multiples of 8)", op, head_size);
    if (tokens > n_seqs * max_q_len) return fail("%s: tokens=%d > n_seqs*max_q_len=%d", op, tokens, n_seqs * max_q_len);
    if (kq.fp8 && head_size % 8) return fail("%s: head_size=%d: no fp8 form of the scalar generic kernel (the fp8 cache is read in pieces of eight elements)", op, head_size);
    int rc = qspec::paged_attention(CH(q), q_stride, CH(key_cache), CH(value_cache), block_tables, max_blocks_per_seq, ctx_lens, q_start, n_seqs, max_q_len, num_heads, num_kv_heads, head_size, block_size, sm_scale, n_splits, (float*)workspace, H(out), ST, kq);
    return finish(op, rc);
}
int sample_top_k_top_p(const char* op, bool seeded, const qspec_half* logits, const float* temperature, const int32_t* top_k,
                       const float* top_p, const float* min_p, const float* exponential, uint64_t seed, uint64_t offset,
                       uint64_t* rng_state, float* probs, int64_t* token, int64_t token_stride, int tokens, int vocab,
                       const int64_t* seq_seeds, const int32_t* seq_seeded, const int32_t* base_pos, int num_seqs,
                       int rows_per_seq, int j_base, int draw_stream, void* workspace, void* stream) {
    if (tokens < 0) return fail("%s: tokens < 0", op);
    if (tokens == 0) return 0;
    NONNULL(op, logits); NONNULL(op, probs); NONNULL(op, token); NONNULL(op, workspace);
    if (seeded) { NONNULL(op, seq_seeds); NONNULL(op, seq_seeded); NONNULL(op, base_pos); }
    if (vocab < 1) return fail("%s: vocab < 1", op);
    qspec::SeedRows sr{};
    if (seeded) {
        if (rows_per_seq < 1) return fail("%s: rows_per_seq=%d must be >= 1", op, rows_per_seq);
        if ((int64_t)num_seqs * rows_per_seq < tokens)
            return fail("%s: num_seqs=%d x rows_per_seq=%d does not cover tokens=%d", op, num_seqs, rows_per_seq, tokens);
        if (j_base < 0 || j_base + rows_per_seq > 65536)
            return fail("%s: j_base=%d + rows_per_seq=%d outside the 16-bit sub-index", op, j_base, rows_per_seq);
        if (draw_stream != 1 && draw_stream != 2) return fail("%s: draw_stream=%d must be 1 (draft) or 2 (target)", op, draw_stream);
        sr = qspec::SeedRows{seq_seeds, seq_seeded, base_pos, rows_per_seq, j_base, (uint32_t)draw_stream};
    }
    const qspec::SampleArgs a{CH(logits), temperature, top_k, top_p, min_p, exponential, seed, offset, rng_state, probs, token,
                              token_stride, tokens, vocab, sr, num_seqs, workspace};
    return finish(op, qspec::sample_top_k_top_p(a, ST));
}
int rejection_sample(const char* op, bool seeded, const float* target_with_bonus_probs, const int64_t* bonus_token_ids,
                     const float* draft_probs, const int64_t* draft_token_ids, const float* uniform, const float* exponential,
                     uint64_t seed, uint64_t offset, uint64_t* rng_state, int batch, int k, int vocab, int64_t dp_stride_b,
                     int64_t dp_stride_k, int64_t ids_stride_b, int64_t ids_stride_k, int64_t bonus_stride, int64_t* out_tokens,
                     uint8_t* accepted, int64_t* recovered, int64_t* counters, const int32_t* active_lens,
                     const int64_t* seq_seeds, const int32_t* seq_seeded, const int32_t* base_pos, void* workspace,
                     void* stream) {
    if (batch == 0) return 0;
    NONNULL(op, target_with_bonus_probs); NONNULL(op, bonus_token_ids); NONNULL(op, draft_probs);
    NONNULL(op, draft_token_ids); NONNULL(op, out_tokens); NONNULL(op, accepted); NONNULL(op, recovered);
    if (seeded) { NONNULL(op, seq_seeds); NONNULL(op, seq_seeded); NONNULL(op, base_pos); }
    NONNULL(op, workspace);
    if (seeded && batch < 0) return fail("%s: batch < 0", op);   // (the unseeded entry never had this check)
    if (batch * k > 4096) return fail("%s: batch*k=%d too large", op, batch * k);
    if (k < 1) return fail("%s: k=%d must be >= 1", op, k);
    const qspec::SeedRows sr = seeded ? qspec::SeedRows{seq_seeds, seq_seeded, base_pos, 1, 0, 0u} : qspec::SeedRows{};
    const qspec::RejectionArgs a{target_with_bonus_probs, draft_probs, draft_token_ids, bonus_token_ids, uniform, exponential, seed,
                                 offset, rng_state, batch, k, vocab, dp_stride_b, dp_stride_k, ids_stride_b, ids_stride_k,
                                 bonus_stride, out_tokens, accepted, recovered, counters, active_lens, sr, workspace};
    return finish(op, qspec::rejection_sample(a, ST));
}
int process_logits(const char* op, bool constrained, const qspec_half* logits, qspec_half* out, int tokens, int vocab,
                   const uint32_t* tok_table, int num_slots, const int32_t* slot_ids, const int32_t* active_lens,
                   const qspec_half* repetition, const qspec_half* frequency, const qspec_half* presence,
                   const int32_t* min_tokens, const int32_t* gen_base, const int32_t* gen_lens, const int32_t* stop_ids,
                   const int32_t* num_stop_ids, int stop_ids_per_slot, const int64_t* draft_ids, int draft_rows,
                   int64_t ids_stride_b, int64_t ids_stride_k, int rows_per_seq, int j_base, const uint32_t* deny,
                   int deny_words, const int32_t* meta, const int32_t* bias_ids, const float* bias_vals, const int32_t* words,
                   const int32_t* word_lens, const int32_t* tail, const int64_t* gen_tokens, int gen_cap,
                   const qspec::LpGuide* guide, void* stream) {
    if (tokens < 0) return fail("%s: tokens < 0", op);
    if (tokens == 0) return 0;
    NONNULL(op, logits); NONNULL(op, out); NONNULL(op, tok_table); NONNULL(op, repetition); NONNULL(op, frequency);
    NONNULL(op, presence); NONNULL(op, min_tokens); NONNULL(op, gen_base); NONNULL(op, gen_lens); NONNULL(op, stop_ids);
    NONNULL(op, num_stop_ids);
    if (constrained) {
        NONNULL(op, deny); NONNULL(op, meta); NONNULL(op, bias_ids); NONNULL(op, bias_vals); NONNULL(op, words);
        NONNULL(op, word_lens); NONNULL(op, tail); NONNULL(op, gen_tokens);
        if ((int64_t)deny_words * 32 < vocab) return fail("%s: deny_words=%d does not cover vocab=%d", op, deny_words, vocab);
        if (gen_cap < 1) return fail("%s: gen_cap=%d must be >= 1", op, gen_cap);
    }
    if (guide) {
        const void *guide_allow = guide->allow, *guide_rank = guide->rank, *guide_off = guide->off, *guide_next = guide->nxt,
                   *guide_slots = guide->gslot;   // (the names the header gives them: the messages name the argument)
        NONNULL(op, guide_allow); NONNULL(op, guide_rank); NONNULL(op, guide_off); NONNULL(op, guide_next);
        NONNULL(op, guide_slots);
        if (guide->words % 4 || (int64_t)guide->words * 32 < vocab)
            return fail("%s: guide_words=%d must be a multiple of 4 that covers vocab=%d", op, guide->words, vocab);
        if (guide->n_states < 1 || guide->n_trans < 1)
            return fail("%s: guide_states=%d / guide_transitions=%d must be >= 1", op, guide->n_states, guide->n_trans);
    }
    if (logits == out) return fail("%s: the pass is out of place (logits == out)", op);
    if (vocab < 1) return fail("%s: vocab < 1", op);
    if (num_slots < 1) return fail("%s: num_slots=%d must be >= 1", op, num_slots);
    if (rows_per_seq < 1) return fail("%s: rows_per_seq=%d must be >= 1", op, rows_per_seq);
    if (j_base < 0) return fail("%s: j_base < 0", op);
    if (stop_ids_per_slot < 0 || stop_ids_per_slot > QS_MAX_STOP_IDS)
        return fail("%s: stop_ids_per_slot=%d outside 0..%d", op, stop_ids_per_slot, QS_MAX_STOP_IDS);
    if (draft_rows < 0 || (draft_rows > 0 && !draft_ids)) return fail("%s: draft_rows=%d without draft_ids", op, draft_rows);
    if (j_base + rows_per_seq - 1 > draft_rows)
        return fail("%s: row j=%d needs %d in-flight tokens, draft_ids has %d rows", op, j_base + rows_per_seq - 1,
                    j_base + rows_per_seq - 1, draft_rows);
    if (j_base + rows_per_seq - 1 > 64) return fail("%s: more than 64 in-flight tokens", op);
    if (!slot_ids && (int64_t)num_slots * rows_per_seq < tokens)
        return fail("%s: num_slots=%d x rows_per_seq=%d does not cover tokens=%d", op, num_slots, rows_per_seq, tokens);
    qspec::LpArgsG a{};
    static_cast<qspec::LpArgs&>(a) = qspec::LpArgs{CH(logits), H(out), tok_table, slot_ids, active_lens, CH(repetition),
                                                   CH(frequency), CH(presence), min_tokens, gen_base, gen_lens, stop_ids,
                                                   num_stop_ids, draft_rows > 0 ? draft_ids : nullptr, ids_stride_b, ids_stride_k,
                                                   vocab, rows_per_seq, j_base, num_slots, stop_ids_per_slot};
    if (constrained) a.c = qspec::LpCons{deny, meta, bias_ids, bias_vals, words, word_lens, tail, gen_tokens, gen_cap, deny_words};
    if (guide) a.g = *guide;
    return finish(op, qspec::process_logits(a, tokens, ST));
}
int spec_advance_draft(const char* op, bool embed, int batch, int block_size, int max_blocks_per_seq, int64_t* input_tokens,
                       const int64_t* sampled_token_ids, int64_t* positions, int32_t* ctx_lens, int64_t* slot_mapping,
                       const int32_t* block_tables, int64_t block_tables_stride, const qspec_half* embed_tokens,
                       qspec_half* hidden_out, int hidden, int vocab, void* stream) {
    if (batch == 0) return 0;
    NONNULL(op, input_tokens); NONNULL(op, sampled_token_ids); NONNULL(op, positions); NONNULL(op, ctx_lens);
    NONNULL(op, slot_mapping); NONNULL(op, block_tables);
    if (!embed)
        return finish(op, qspec::spec_advance_draft(batch, block_size, max_blocks_per_seq, input_tokens, sampled_token_ids, positions, ctx_lens, slot_mapping, block_tables, block_tables_stride, ST));
    NONNULL(op, embed_tokens); NONNULL(op, hidden_out);
    if (hidden % 8 || hidden <= 0) return fail("%s: hidden=%d must be a positive multiple of 8", op, hidden);
    return finish(op, qspec::spec_advance_draft_embed(batch, block_size, max_blocks_per_seq, input_tokens, sampled_token_ids, positions, ctx_lens, slot_mapping, block_tables, block_tables_stride, CH(embed_tokens), H(hidden_out), hidden, vocab, ST));
}
int spec_prepare_draft(const char* op, bool embed, int batch, int block_size, int max_blocks_per_seq, const int64_t* last_token,
                       const int32_t* seq_lens, const int32_t* step_mask, int32_t* eff_lens, const int32_t* block_tables,
                       int64_t block_tables_stride, int64_t* input_tokens, int64_t* positions, int64_t* slot_mapping,
                       int32_t* ctx_lens, const qspec_half* embed_tokens, qspec_half* hidden_out, int hidden, int vocab,
                       void* stream) {
    if (batch == 0) return 0;
    NONNULL(op, last_token); NONNULL(op, seq_lens); NONNULL(op, block_tables); NONNULL(op, input_tokens);
    NONNULL(op, positions); NONNULL(op, slot_mapping); NONNULL(op, ctx_lens);
    if (!embed)
        return finish(op, qspec::spec_prepare_draft(batch, block_size, max_blocks_per_seq, last_token, seq_lens, block_tables, block_tables_stride, input_tokens, positions, slot_mapping, ctx_lens, ST));
    NONNULL(op, embed_tokens); NONNULL(op, hidden_out);
    if (step_mask && !eff_lens) return fail("%s: step_mask needs eff_lens", op);
    if (hidden % 8 || hidden <= 0) return fail("%s: hidden=%d must be a positive multiple of 8", op, hidden);
    return finish(op, qspec::spec_prepare_draft_embed(batch, block_size, max_blocks_per_seq, last_token, seq_lens, step_mask, eff_lens, block_tables, block_tables_stride, input_tokens, positions, slot_mapping, ctx_lens, CH(embed_tokens), H(hidden_out), hidden, vocab, ST));
}
int spec_prepare_verify(const char* op, bool embed, int batch, int k, int block_size, int max_blocks_per_seq,
                        const int64_t* last_token, const int64_t* draft_token_ids, int64_t ids_stride_b, int64_t ids_stride_k,
                        const int32_t* seq_lens, const int32_t* block_tables, int64_t block_tables_stride, int64_t* tokens,
                        int64_t* positions, int64_t* slot_mapping, int32_t* ctx_lens, const qspec_half* embed_tokens,
                        qspec_half* hidden_out, int hidden, int vocab, void* stream) {
    if (batch == 0) return 0;
    NONNULL(op, last_token); NONNULL(op, draft_token_ids); NONNULL(op, seq_lens); NONNULL(op, block_tables);
    NONNULL(op, tokens); NONNULL(op, positions); NONNULL(op, slot_mapping); NONNULL(op, ctx_lens);
    if (!embed)
        return finish(op, qspec::spec_prepare_verify(batch, k, block_size, max_blocks_per_seq, last_token, draft_token_ids, ids_stride_b, ids_stride_k, seq_lens, block_tables, block_tables_stride, tokens, positions, slot_mapping, ctx_lens, ST));
    NONNULL(op, embed_tokens); NONNULL(op, hidden_out);
    if (hidden % 8 || hidden <= 0) return fail("%s: hidden=%d must be a positive multiple of 8", op, hidden);
    return finish(op, qspec::spec_prepare_verify_embed(batch, k, block_size, max_blocks_per_seq, last_token, draft_token_ids, ids_stride_b, ids_stride_k, seq_lens, block_tables, block_tables_stride, tokens, positions, slot_mapping, ctx_lens, CH(embed_tokens), H(hidden_out), hidden, vocab, ST));
}

}  // namespace

extern "C" {

int qspec_abi_version(void) { return 6; }
const char* qspec_last_error(void) { return g_err; }

int qspec_rms_norm_general_fuse_sum_i4(int8_t* out_q, const qspec_half* x, qspec_half* input_sum, qspec_half* scaling,
                                       float eps, int tokens, int hidden, void* stream) {
    const char* op = "qspec_rms_norm_general_fuse_sum_i4";
    if (tokens < 0) return fail("%s: tokens < 0", op);
    if (tokens == 0) return 0;
    NONNULL(op, out_q); NONNULL(op, x); NONNULL(op, scaling);
    if (hidden % 1024 || hidden > 8192 || hidden <= 0) return fail("%s: hidden=%d must be a multiple of 1024, <= 8192", op, hidden);
    return finish(op, qspec::ln_quant_i4(CH(x), nullptr, nullptr, out_q, H(scaling), H(input_sum), eps, tokens, hidden, ST));
}
int qspec_rms_norm_general_fuse_sum_fp16(qspec_half* out, const qspec_half* x, float eps, int tokens, int hidden,
                                         void* stream) {
    const char* op = "qspec_rms_norm_general_fuse_sum_fp16";
    if (tokens < 0) return fail("%s: tokens < 0", op);
    if (tokens == 0) return 0;
    NONNULL(op, out); NONNULL(op, x);
    if (hidden % 1024 || hidden > 8192 || hidden <= 0) return fail("%s: hidden=%d must be a multiple of 1024, <= 8192", op, hidden);
    return finish(op, qspec::ln_fp16(CH(x), nullptr, nullptr, H(out), eps, tokens, hidden, ST));
}
int qspec_add_rms_norm_i4(int8_t* out_q, qspec_half* scaling, qspec_half* hidden_out, const qspec_half* x,
                          const qspec_half* delta, float eps, int tokens, int hidden, void* stream) {
    const char* op = "qspec_add_rms_norm_i4";
    if (tokens < 0) return fail("%s: tokens < 0", op);
    if (tokens == 0) return 0;
    NONNULL(op, out_q); NONNULL(op, x); NONNULL(op, scaling);
    if (delta) NONNULL(op, hidden_out);
    if (hidden % 1024 || hidden > 8192 || hidden <= 0) return fail("%s: hidden=%d must be a multiple of 1024, <= 8192", op, hidden);
    return finish(op, qspec::ln_quant_i4(CH(x), CH(delta), H(hidden_out), out_q, H(scaling), nullptr, eps, tokens, hidden, ST));
}
int qspec_add_rms_norm_fp16(qspec_half* out, qspec_half* hidden_out, const qspec_half* x, const qspec_half* delta, float eps,
                            int tokens, int hidden, void* stream) {
    return add_rms_norm_fp16("qspec_add_rms_norm_fp16", 0, out, hidden_out, x, delta, eps, tokens, hidden, stream);
}
int qspec_add_rms_norm_fp16_xp(qspec_half* out, qspec_half* hidden_out, const qspec_half* x, const qspec_half* delta, float eps,
                               int tokens, int hidden, void* stream) {
    return add_rms_norm_fp16("qspec_add_rms_norm_fp16_xp", 1, out, hidden_out, x, delta, eps, tokens, hidden, stream);
}
int qspec_fuse_sym_quant(const qspec_half* x, qspec_half* scale, int8_t* q, float clip_ratio, int tokens, int k,
                         void* stream) {
    const char* op = "qspec_fuse_sym_quant";
    if (tokens < 0) return fail("%s: tokens < 0", op);
    if (tokens == 0) return 0;
    NONNULL(op, x); NONNULL(op, scale); NONNULL(op, q);
    if (k <= 0 || k % 2) return fail("%s: k=%d must be positive and even", op, k);
    return finish(op, qspec::rowabsmax_quant(CH(x), H(scale), q, clip_ratio, tokens, k, ST));
}
int qspec_fast_hadamard_transform(const qspec_half* x, float scale, qspec_half* out, int64_t rows, int n,
                                  void* stream) {
    const char* op = "qspec_fast_hadamard_transform";
    if (rows < 0) return fail("%s: rows < 0", op);
    if (rows == 0) return 0;
    NONNULL(op, x); NONNULL(op, out);
    if (n < 1 || n > 32768 || (n & (n - 1))) return fail("%s: n=%d must be a power of two in [1, 32768]", op, n);
    if (rows > 2147483647LL) return fail("%s: too many rows", op);
    return finish(op, qspec::fwht(CH(x), scale, H(out), rows, n, ST));
}
int qspec_hadamard_mix(const qspec_half* y, const qspec_half* hadK, qspec_half* out, int tokens, int K, int m,
                       void* stream) {
    const char* op = "qspec_hadamard_mix";
    if (tokens < 0) return fail("%s: tokens < 0", op);
    if (tokens == 0) return 0;
    NONNULL(op, y); NONNULL(op, hadK); NONNULL(op, out);
    if (y == out) return fail("%s: in-place not supported", op);
    return finish(op, qspec::hadk_mix(CH(y), CH(hadK), H(out), tokens, K, m, ST));
}
int qspec_heads_hadamard(const qspec_half* attn, qspec_half* out_f16, int8_t* q, qspec_half* scale, float had_scale,
                         float clip_ratio, int tokens, int heads, int head_dim, void* stream) {
    const char* op = "qspec_heads_hadamard";
    if (tokens < 0) return fail("%s: tokens < 0", op);
    if (tokens == 0) return 0;
    NONNULL(op, attn);
    if (q) { NONNULL(op, scale); } else { NONNULL(op, out_f16); }
    return finish(op, qspec::heads_hadamard(CH(attn), H(out_f16), q, H(scale), had_scale, clip_ratio, tokens, heads, head_dim, ST));
}
int qspec_heads_hadamard_mix(const qspec_half* attn, const qspec_half* hadK, qspec_half* out, float had_scale, int tokens,
                             int heads, int head_dim, int K, void* stream) {
    const char* op = "qspec_heads_hadamard_mix";
    if (tokens < 0) return fail("%s: tokens < 0", op);
    if (tokens == 0) return 0;
    NONNULL(op, attn); NONNULL(op, hadK); NONNULL(op, out);
    if (attn == out) return fail("%s: in-place not supported", op);
    return finish(op, qspec::heads_hadamard_mix(CH(attn), CH(hadK), H(out), had_scale, tokens, heads, head_dim, K, ST));
}
int qspec_silu_mul(const qspec_half* gate_up, qspec_half* out, int tokens, int intermediate, void* stream) {
    const char* op = "qspec_silu_mul";
    if (tokens == 0) return 0;
    NONNULL(op, gate_up); NONNULL(op, out);
    return finish(op, qspec::silu_mul(CH(gate_up), H(out), tokens, intermediate, ST));
}
int qspec_silu_mul_hadamard(const qspec_half* gate_up, const qspec_half* hadK, qspec_half* out_f16, int8_t* q,
                            qspec_half* scale, float had_scale, float clip_ratio, int tokens, int intermediate, int K,
                            void* stream) {
    const char* op = "qspec_silu_mul_hadamard";
    if (tokens < 0) return fail("%s: tokens < 0", op);
    if (tokens == 0) return 0;
    NONNULL(op, gate_up);
    if (K > 1) NONNULL(op, hadK);
    if (q) { NONNULL(op, scale); } else { NONNULL(op, out_f16); }
    if (intermediate % 8) return fail("%s: intermediate %% 8 != 0", op);
    return finish(op, qspec::silu_mul_hadamard(CH(gate_up), CH(hadK), H(out_f16), q, H(scale), had_scale, clip_ratio, tokens, intermediate, K, 0, nullptr, ST));
}
int qspec_rowwise_scaled_linear_s4s4(const int8_t* xq, const qspec_half* xs, const int8_t* wq, const qspec_half* ws,
                                     const qspec_half* bias, qspec_half* out, int M, int N, int K, void* stream) {
    const char* op = "qspec_rowwise_scaled_linear_s4s4";
    if (M < 0 || N < 0) return fail("%s: negative size", op);
    if (M == 0 || N == 0) return 0;
    NONNULL(op, xq); NONNULL(op, xs); NONNULL(op, wq); NONNULL(op, ws); NONNULL(op, out);
    if (N % 16 || K % 128 || K <= 0) return fail("%s: need N %% 16 == 0 and K %% 128 == 0 (N=%d K=%d)", op, N, K);
    if (!bias && use_stream() && qspec::gemm_w4a4_stream_supported(M, N, K, false)) {
        qspec::StreamActs x;
        x.xq = xq; x.xs = CH(xs);
        return finish(op, qspec::gemm_w4a4_stream(x, wq, CH(ws), H(out), M, N, K, ST));
    }
    return finish(op, qspec::gemm_w4a4(xq, CH(xs), wq, CH(ws), CH(bias), H(out), M, N, K, ST));
}
int qspec_rowwise_scaled_linear_s4s4_residual(const int8_t* xq, const qspec_half* xs, const int8_t* wq,
                                              const qspec_half* ws, const qspec_half* resid_in, qspec_half* resid_out,
                                              int M, int N, int K, void* stream) {
    const char* op = "qspec_rowwise_scaled_linear_s4s4_residual";
    if (M < 0 || N < 0) return fail("%s: negative size", op);
    if (M == 0 || N == 0) return 0;
    NONNULL(op, xq); NONNULL(op, xs); NONNULL(op, wq); NONNULL(op, ws); NONNULL(op, resid_in); NONNULL(op, resid_out);
    if (!qspec::gemm_w4a4_stream_supported(M, N, K, false))
        return fail("%s: need M <= 32, N %% 16 == 0 and a built K (M=%d N=%d K=%d)", op, M, N, K);
    qspec::StreamActs x;
    x.xq = xq; x.xs = CH(xs);
    return finish(op, qspec::gemm_w4a4_stream_residual(x, wq, CH(ws), CH(resid_in), H(resid_out), M, N, K, ST));
}
int qspec_rowwise_scaled_linear_s4s4_residual_supported(int M, int N, int K) {
    return qspec::gemm_w4a4_stream_supported(M, N, K, false) ? 1 : 0;
}
int qspec_rowwise_scaled_linear_s4s4_residual_hq_supported(int M, int N, int K, int n_parts) {
    return qspec::gemm_w4a4_stream_residual_hq_supported(M, N, K, n_parts) ? 1 : 0;
}
int qspec_rowwise_scaled_linear_s4s4_residual_hq(const qspec_half* x16, const float* part_amax, int n_parts,
                                                 float clip_ratio, const int8_t* wq, const qspec_half* ws,
                                                 const qspec_half* resid_in, qspec_half* resid_out, int M, int N, int K,
                                                 void* stream) {
    const char* op = "qspec_rowwise_scaled_linear_s4s4_residual_hq";
    if (M < 0 || N < 0) return fail("%s: negative size", op);
    if (M == 0 || N == 0) return 0;
    NONNULL(op, x16); NONNULL(op, part_amax); NONNULL(op, wq); NONNULL(op, ws); NONNULL(op, resid_in); NONNULL(op, resid_out);
    if (!qspec::gemm_w4a4_stream_residual_hq_supported(M, N, K, n_parts))
        return fail("%s: need M <= 4, K = 4096, n_parts = 8, N %% 16 == 0 (M=%d N=%d K=%d n_parts=%d)", op, M, N, K, n_parts);
    return finish(op, qspec::gemm_w4a4_stream_residual_hq(CH(x16), part_amax, n_parts, clip_ratio, wq, CH(ws), CH(resid_in),
                                                          H(resid_out), M, N, K, ST));
}
size_t qspec_w4a16_workspace_bytes(void) { return qspec::gemm_w4a16_ws_bytes(); }
int qspec_w4a16_linear(const qspec_half* x, const int8_t* wq, const qspec_half* ws, const qspec_half* bias, qspec_half* out,
                       int M, int N, int K, void* workspace, void* stream) {
    return w4a16_linear("qspec_w4a16_linear", 0, x, wq, ws, bias, out, M, N, K, workspace, stream);
}
int qspec_w4a16_act_layout32_supported(int M, int N, int K) { return w4a16_act_layout32_supported(M, N, K); }
int qspec_w4a16_linear_xp32(const qspec_half* x, const int8_t* wq, const qspec_half* ws, qspec_half* out, int M, int N, int K,
                            void* stream) {
    const char* op = "qspec_w4a16_linear_xp32";
    if (M == 0 || N == 0) return 0;
    NONNULL(op, x); NONNULL(op, wq); NONNULL(op, ws); NONNULL(op, out);
    if (!w4a16_act_layout32_supported(M, N, K))
        return fail("%s: no two-tile streaming form for (M=%d N=%d K=%d): ask qspec_w4a16_act_layout32_supported", op, M, N, K);
    return finish(op, qspec::gemm_w4a16_stream32(CH(x), wq, CH(ws), H(out), M, N, K, ST));
}
int qspec_w4a16_linear_partial_slices_xp32(int M, int N, int K) { return w4a16_linear_partial_slices_xp32(M, N, K); }
int qspec_w4a16_linear_partial_xp32(const qspec_half* x, const int8_t* wq, float* part, int M, int N, int K, int slices, void* stream) {
    const char* op = "qspec_w4a16_linear_partial_xp32";
    if (M == 0 || N == 0) return 0;
    NONNULL(op, x); NONNULL(op, wq); NONNULL(op, part);
    if (slices < 2 || slices != w4a16_linear_partial_slices_xp32(M, N, K))
        return fail("%s: (M=%d N=%d K=%d) takes %d slices (qspec_w4a16_linear_partial_slices_xp32), got %d", op, M, N, K,
                    w4a16_linear_partial_slices_xp32(M, N, K), slices);
    return finish(op, qspec::gemm_w4a16_stream32_partial(CH(x), wq, part, M, N, K, slices, ST));
}
int qspec_qkv_rope_linear_w4a16_xp32(const qspec_half* x, const int8_t* wq, const qspec_half* ws, qspec_half* qkv, int M, int N,
                                     int K, const int64_t* positions, const qspec_half* cos_sin_cache, qspec_half* key_cache,
                                     qspec_half* value_cache, const int64_t* slot_mapping, int num_heads, int num_kv_heads,
                                     int head_size, int rot_dim, void* stream) {
    return qkv_rope_linear_w4a16_xp32("qspec_qkv_rope_linear_w4a16_xp32", qspec::KvQuant(), x, wq, ws, qkv, M, N, K, positions,
                                      cos_sin_cache, key_cache, value_cache, slot_mapping, num_heads, num_kv_heads, head_size,
                                      rot_dim, stream);
}
int qspec_gate_up_silu_linear_w4a16_xp32(const qspec_half* x, const int8_t* wq, const qspec_half* ws, qspec_half* act, int M,
                                         int intermediate, int K, void* stream) {
    const char* op = "qspec_gate_up_silu_linear_w4a16_xp32";
    if (M == 0) return 0;
    NONNULL(op, x); NONNULL(op, wq); NONNULL(op, ws); NONNULL(op, act);
    if (intermediate % 8 || !w4a16_act_layout32_supported(M, 2 * intermediate, K))
        return fail("%s: no two-tile streaming form for (M=%d I=%d K=%d)", op, M, intermediate, K);
    return finish(op, qspec::gemm_w4a16_stream32_gate_up_silu(CH(x), wq, CH(ws), H(act), M, intermediate, K, ST));
}
int qspec_mlp_hadamard_act_layout_supported(int tokens, int intermediate, int K) {
    return qspec::mlp_hadamard_xperm_supported(tokens, intermediate, K) ? 1 : 0;
}
int qspec_w4a16_act_layout_supported(int M, int K) { return use_stream() && qspec::gemm_w4a16_xperm_supported(M, K) ? 1 : 0; }
int qspec_w4a16_linear_xp(const qspec_half* x, const int8_t* wq, const qspec_half* ws, const qspec_half* bias, qspec_half* out,
                          int M, int N, int K, void* workspace, void* stream) {
    return w4a16_linear("qspec_w4a16_linear_xp", 1, x, wq, ws, bias, out, M, N, K, workspace, stream);
}
int qspec_linear_f16(const qspec_half* x, const qspec_half* w, qspec_half* out, int M, int N, int K, void* stream) {
    const char* op = "qspec_linear_f16";
    if (M < 0 || N < 0) return fail("%s: negative size", op);
    if (M == 0 || N == 0) return 0;
    NONNULL(op, x); NONNULL(op, w); NONNULL(op, out);
    if (K % 32 || K <= 0) return fail("%s: need K %% 32 == 0 (K=%d)", op, K);
    if (use_stream() && qspec::gemm_f16_stream_supported(M, N, K))
        return finish(op, qspec::gemm_f16_stream(CH(x), CH(w), H(out), M, N, K, nullptr, ST));
    if (M > 16 && tiled_min_m() < (1 << 30) && qspec::gemm_f16_tiled_supported(M, N, K))   // prefill / large-batch logits
        return finish(op, qspec::gemm_f16_tiled(CH(x), CH(w), H(out), M, N, K, ST));
    return finish(op, qspec::gemm_f16(CH(x), CH(w), H(out), M, N, K, ST));
}
int qspec_dequant_w4(const int8_t* wq, const qspec_half* ws, qspec_half* out, int N, int K, void* stream) {
    const char* op = "qspec_dequant_w4";
    if (N == 0) return 0;
    NONNULL(op, wq); NONNULL(op, ws); NONNULL(op, out);
    return finish(op, qspec::dequant_w4(wq, CH(ws), H(out), N, K, ST));
}
int qspec_rotary_embedding(const int64_t* positions, qspec_half* q, qspec_half* k, const qspec_half* cos_sin_cache,
                           int tokens, int num_heads, int num_kv_heads, int head_size, int rot_dim, int64_t q_stride,
                           int64_t k_stride, void* stream) {
    const char* op = "qspec_rotary_embedding";
    if (tokens == 0) return 0;
    NONNULL(op, positions); NONNULL(op, q); NONNULL(op, k); NONNULL(op, cos_sin_cache);
    return finish(op, qspec::rotary_embedding(positions, H(q), H(k), CH(cos_sin_cache), tokens, num_heads, num_kv_heads, head_size, rot_dim, q_stride, k_stride, ST));
}
int qspec_reshape_and_cache_flash(const qspec_half* key, const qspec_half* value, qspec_half* key_cache,
                                  qspec_half* value_cache, const int64_t* slot_mapping, int tokens, int num_kv_heads,
                                  int head_size, int64_t key_stride, int64_t value_stride, void* stream) {
    return reshape_and_cache_flash("qspec_reshape_and_cache_flash", qspec::KvQuant(), key, value, key_cache, value_cache,
                                   slot_mapping, tokens, num_kv_heads, head_size, key_stride, value_stride, stream);
}
int qspec_rope_kv_write(const int64_t* positions, qspec_half* qkv, const qspec_half* cos_sin_cache, qspec_half* key_cache,
                        qspec_half* value_cache, const int64_t* slot_mapping, int tokens, int num_heads, int num_kv_heads,
                        int head_size, int rot_dim, void* stream) {
    return rope_kv_write("qspec_rope_kv_write", qspec::KvQuant(), positions, qkv, cos_sin_cache, key_cache, value_cache,
                         slot_mapping, tokens, num_heads, num_kv_heads, head_size, rot_dim, stream);
}
size_t qspec_paged_attention_workspace_bytes(int max_tokens, int num_heads, int head_size, int n_splits) {
    return qspec::paged_attention_ws_bytes(max_tokens, num_heads, head_size, n_splits);
}
int qspec_paged_attention_family(int n_seqs, int max_q_len, int num_heads, int num_kv_heads, int head_size, int block_size,
                                 int max_blocks_per_seq, int n_splits, int merged) {
    return qspec::paged_attention_family(n_seqs, max_q_len, num_heads, num_kv_heads, head_size, block_size, max_blocks_per_seq,
                                         n_splits, merged != 0);
}
int qspec_paged_attention(const qspec_half* q, int64_t q_stride, const qspec_half* key_cache, const qspec_half* value_cache,
                          const int32_t* block_tables, int max_blocks_per_seq, const int32_t* ctx_lens, const int32_t* q_start,
                          int n_seqs, int tokens, int max_q_len, int num_heads, int num_kv_heads, int head_size, int block_size,
                          float sm_scale, int n_splits, void* workspace, qspec_half* out, void* stream) {
    return paged_attention("qspec_paged_attention", qspec::KvQuant(), q, q_stride, key_cache, value_cache, block_tables,
                           max_blocks_per_seq, ctx_lens, q_start, n_seqs, tokens, max_q_len, num_heads, num_kv_heads, head_size,
                           block_size, sm_scale, n_splits, workspace, out, stream);
}
int qspec_heads_hadamard_merged(const void* attn_workspace, int max_tokens, int n_splits, qspec_half* out_f16, int8_t* q,
                                qspec_half* scale, float had_scale, float clip_ratio, int tokens, int heads, int head_dim,
                                void* stream) {
    return heads_hadamard_merged("qspec_heads_hadamard_merged", 0, attn_workspace, max_tokens, n_splits, out_f16, q, scale,
                                 had_scale, clip_ratio, tokens, heads, head_dim, stream);
}
int qspec_heads_hadamard_merged_xp(const void* attn_workspace, int max_tokens, int n_splits, qspec_half* out_f16, int8_t* q,
                                   qspec_half* scale, float had_scale, float clip_ratio, int tokens, int heads, int head_dim,
                                   void* stream) {
    return heads_hadamard_merged("qspec_heads_hadamard_merged_xp", 1, attn_workspace, max_tokens, n_splits, out_f16, q, scale,
                                 had_scale, clip_ratio, tokens, heads, head_dim, stream);
}
int qspec_heads_hadamard_merged_spread_supported(int tokens, int heads, int head_dim) {
    return heads_hadamard_merged_spread_supported(tokens, heads, head_dim);
}
int qspec_heads_hadamard_merged_spread(const void* attn_workspace, int max_tokens, int n_splits, qspec_half* out_f16,
                                       float* part_amax, float had_scale, int tokens, int heads, int head_dim,
                                       void* stream) {
    const char* op = "qspec_heads_hadamard_merged_spread";
    if (tokens < 0) return fail("%s: tokens < 0", op);
    if (tokens == 0) return 0;
    NONNULL(op, attn_workspace); NONNULL(op, out_f16); NONNULL(op, part_amax);
    if (!heads_hadamard_merged_spread_supported(tokens, heads, head_dim))
        return fail("%s: built for 32 heads of 128 and at most 128 tokens (got %d x %d, %d tokens)", op, heads, head_dim, tokens);
    return finish(op, qspec::heads_hadamard_merge_spread((const float*)attn_workspace, max_tokens, n_splits, H(out_f16),
                                                         part_amax, had_scale, tokens, heads, head_dim, ST));
}
int qspec_heads_hadamard_mix_merged_spread_supported(int tokens, int heads, int head_dim, int K) {
    return qspec::heads_hadamard_mix_merge_spread_supported(tokens, heads, head_dim, K) ? 1 : 0;
}
int qspec_heads_hadamard_mix_merged_spread(const void* attn_workspace, int max_tokens, int n_splits, const qspec_half* hadK,
                                           int K, qspec_half* out_f16, float* part_amax, float had_scale, int tokens, int heads,
                                           int head_dim, void* stream) {
    return heads_hadamard_mix_merged_spread("qspec_heads_hadamard_mix_merged_spread", 0, attn_workspace, max_tokens, n_splits,
                                            hadK, K, out_f16, part_amax, had_scale, tokens, heads, head_dim, stream);
}
int qspec_heads_hadamard_mix_merged_spread_xp(const void* attn_workspace, int max_tokens, int n_splits, const qspec_half* hadK,
                                              int K, qspec_half* out_f16, float* part_amax, float had_scale, int tokens,
                                              int heads, int head_dim, void* stream) {
    return heads_hadamard_mix_merged_spread("qspec_heads_hadamard_mix_merged_spread_xp", 1, attn_workspace, max_tokens,
                                            n_splits, hadK, K, out_f16, part_amax, had_scale, tokens, heads, head_dim, stream);
}
int qspec_embedding(const int64_t* ids, const qspec_half* table, qspec_half* out, int tokens, int hidden, int vocab,
                    void* stream) {
    const char* op = "qspec_embedding";
    if (tokens == 0) return 0;
    NONNULL(op, ids); NONNULL(op, table); NONNULL(op, out);
    return finish(op, qspec::embedding(ids, CH(table), H(out), tokens, hidden, vocab, ST));
}
size_t qspec_sampler_workspace_bytes(int rows) { return qspec::sampler_ws_bytes(rows); }
int qspec_softmax_argmax(const qspec_half* logits, float* probs, int64_t* token, int tokens, int vocab,
                         void* workspace, void* stream) {
    const char* op = "qspec_softmax_argmax";
    if (tokens == 0) return 0;
    NONNULL(op, logits); NONNULL(op, probs); NONNULL(op, token); NONNULL(op, workspace);
    return finish(op, qspec::softmax_argmax(CH(logits), probs, token, tokens, vocab, workspace, ST));
}
size_t qspec_lm_head_sampler_workspace_bytes(int rows) { return qspec::head_softmax_ws_bytes(rows); }
int qspec_lm_head_softmax_argmax(const qspec_half* hidden, const qspec_half* lm_head, qspec_half* logits, float* probs,
                                 int64_t* token, int tokens, int vocab, int K, void* workspace, void* stream) {
    const char* op = "qspec_lm_head_softmax_argmax";
    if (tokens == 0) return 0;
    NONNULL(op, hidden); NONNULL(op, lm_head); NONNULL(op, logits); NONNULL(op, probs); NONNULL(op, token);
    NONNULL(op, workspace);
    if (!(use_stream() && qspec::gemm_f16_stream_supported(tokens, vocab, K)))
        return fail("%s: (tokens=%d vocab=%d K=%d) is not a streaming lm_head shape (tokens <= 16, vocab %% 16 == 0); "
                    "use qspec_linear_f16 + qspec_softmax_argmax", op, tokens, vocab, K);
    int rc = qspec::gemm_f16_stream(CH(hidden), CH(lm_head), H(logits), tokens, vocab, K,
                                    qspec::head_softmax_part_max(workspace, tokens), ST);
    if (rc == 0)
        rc = qspec::head_softmax_argmax(CH(logits), probs, token, tokens, vocab, qspec::gemm_f16_stream_grid(vocab),
                                        workspace, ST);
    return finish(op, rc);
}
int qspec_lm_head_softmax_argmax_supported(int tokens, int vocab, int K) {
    return use_stream() && qspec::gemm_f16_stream_supported(tokens, vocab, K) ? 1 : 0;
}
int qspec_rejection_sample(const float* target_with_bonus_probs, const int64_t* bonus_token_ids, const float* draft_probs,
                           const int64_t* draft_token_ids, const float* uniform, const float* exponential, uint64_t seed,
                           uint64_t offset, uint64_t* rng_state, int batch, int k, int vocab, int64_t dp_stride_b,
                           int64_t dp_stride_k, int64_t ids_stride_b, int64_t ids_stride_k, int64_t bonus_stride,
                           int64_t* out_tokens, uint8_t* accepted, int64_t* recovered, int64_t* counters,
                           const int32_t* active_lens, void* workspace, void* stream) {
    return rejection_sample("qspec_rejection_sample", false, target_with_bonus_probs, bonus_token_ids, draft_probs,
                            draft_token_ids, uniform, exponential, seed, offset, rng_state, batch, k, vocab, dp_stride_b,
                            dp_stride_k, ids_stride_b, ids_stride_k, bonus_stride, out_tokens, accepted, recovered, counters,
                            active_lens, nullptr, nullptr, nullptr, workspace, stream);
}
size_t qspec_sample_workspace_bytes(int rows) { return qspec::sample_ws_bytes(rows); }
int qspec_sample_top_k_top_p(const qspec_half* logits, const float* temperature, const int32_t* top_k, const float* top_p,
                             const float* exponential, uint64_t seed, uint64_t offset, uint64_t* rng_state, float* probs,
                             int64_t* token, int64_t token_stride, int tokens, int vocab, void* workspace, void* stream) {
    return sample_top_k_top_p("qspec_sample_top_k_top_p", false, logits, temperature, top_k, top_p, nullptr, exponential, seed,
                              offset, rng_state, probs, token, token_stride, tokens, vocab, nullptr, nullptr, nullptr, 0, 0, 0,
                              0, workspace, stream);
}
// Seeded twins of qspec_rejection_sample / qspec_sample_top_k_top_p: rows of a sequence with seq_seeded != 0 draw from
// Philox keyed by (seed, base position, stream, j, v) alone (include/qspec_hip.h, "seeded draws"); the reference honours
// SamplingParams.seed through seeded_seqs (vllm/spec_decode/spec_decode_worker.py:295,901-906 ->
// vllm/model_executor/layers/rejection_sampler.py:60-67,229-250,387-399; Sampler: sampler.py:585-604).
int qspec_rejection_sample_seeded(const float* target_with_bonus_probs, const int64_t* bonus_token_ids,
                                  const float* draft_probs, const int64_t* draft_token_ids, const float* uniform,
                                  const float* exponential, uint64_t seed, uint64_t offset, uint64_t* rng_state, int batch,
                                  int k, int vocab, int64_t dp_stride_b, int64_t dp_stride_k, int64_t ids_stride_b,
                                  int64_t ids_stride_k, int64_t bonus_stride, int64_t* out_tokens, uint8_t* accepted,
                                  int64_t* recovered, int64_t* counters, const int32_t* active_lens, const int64_t* seq_seeds,
                                  const int32_t* seq_seeded, const int32_t* base_pos, void* workspace, void* stream) {
    return rejection_sample("qspec_rejection_sample_seeded", true, target_with_bonus_probs, bonus_token_ids, draft_probs,
                            draft_token_ids, uniform, exponential, seed, offset, rng_state, batch, k, vocab, dp_stride_b,
                            dp_stride_k, ids_stride_b, ids_stride_k, bonus_stride, out_tokens, accepted, recovered, counters,
                            active_lens, seq_seeds, seq_seeded, base_pos, workspace, stream);
}
int qspec_sample_top_k_top_p_seeded(const qspec_half* logits, const float* temperature, const int32_t* top_k,
                                    const float* top_p, const float* exponential, uint64_t seed, uint64_t offset,
                                    uint64_t* rng_state, float* probs, int64_t* token, int64_t token_stride, int tokens,
                                    int vocab, const int64_t* seq_seeds, const int32_t* seq_seeded, const int32_t* base_pos,
                                    int num_seqs, int rows_per_seq, int j_base, int draw_stream, void* workspace,
                                    void* stream) {
    return sample_top_k_top_p("qspec_sample_top_k_top_p_seeded", true, logits, temperature, top_k, top_p, nullptr, exponential,
                              seed, offset, rng_state, probs, token, token_stride, tokens, vocab, seq_seeds, seq_seeded,
                              base_pos, num_seqs, rows_per_seq, j_base, draw_stream, workspace, stream);
}
// min_p twins of qspec_sample_top_k_top_p(_seeded): _apply_min_p (vllm/model_executor/layers/sampler.py:416-430) as one more
// boundary of the selection kernel; min_p NULL = the entry without it, bit for bit.
int qspec_sample_top_k_top_p_min_p(const qspec_half* logits, const float* temperature, const int32_t* top_k, const float* top_p,
                                   const float* min_p, const float* exponential, uint64_t seed, uint64_t offset,
                                   uint64_t* rng_state, float* probs, int64_t* token, int64_t token_stride, int tokens,
                                   int vocab, void* workspace, void* stream) {
    return sample_top_k_top_p("qspec_sample_top_k_top_p_min_p", false, logits, temperature, top_k, top_p, min_p, exponential,
                              seed, offset, rng_state, probs, token, token_stride, tokens, vocab, nullptr, nullptr, nullptr, 0,
                              0, 0, 0, workspace, stream);
}
int qspec_sample_top_k_top_p_min_p_seeded(const qspec_half* logits, const float* temperature, const int32_t* top_k,
                                          const float* top_p, const float* min_p, const float* exponential, uint64_t seed,
                                          uint64_t offset, uint64_t* rng_state, float* probs, int64_t* token,
                                          int64_t token_stride, int tokens, int vocab, const int64_t* seq_seeds,
                                          const int32_t* seq_seeded, const int32_t* base_pos, int num_seqs, int rows_per_seq,
                                          int j_base, int draw_stream, void* workspace, void* stream) {
    return sample_top_k_top_p("qspec_sample_top_k_top_p_min_p_seeded", true, logits, temperature, top_k, top_p, min_p,
                              exponential, seed, offset, rng_state, probs, token, token_stride, tokens, vocab, seq_seeds,
                              seq_seeded, base_pos, num_seqs, rows_per_seq, j_base, draw_stream, workspace, stream);
}
// Logit processors: Sampler.forward's _apply_min_tokens_penalty + apply_penalties (vllm/model_executor/layers/sampler.py:258-266,
// :338-384; vllm/model_executor/layers/utils.py:24-57), per row of a speculative cycle (include/qspec_hip.h, "logit processors").
int qspec_logit_table_set_prompt(uint32_t* tok_table, int32_t* counted_len, int num_slots, int vocab, int slot,
                                 const int64_t* prompt_ids, int num_prompt, const int64_t* output_ids, int num_outputs,
                                 void* stream) {
    const char* op = "qspec_logit_table_set_prompt";
    NONNULL(op, tok_table); NONNULL(op, counted_len);
    if (vocab < 1) return fail("%s: vocab < 1", op);
    if (slot < 0 || slot >= num_slots) return fail("%s: slot=%d outside the %d slots of the table", op, slot, num_slots);
    if (num_prompt < 0 || num_outputs < 0) return fail("%s: negative token count", op);
    if (num_prompt > 0) NONNULL(op, prompt_ids);
    if (num_outputs > 0) NONNULL(op, output_ids);
    return finish(op, qspec::logit_table_set_prompt(tok_table, vocab, slot, prompt_ids, num_prompt, output_ids, num_outputs,
                                                    counted_len, ST));
}
int qspec_logit_table_catch_up(uint32_t* tok_table, int32_t* counted_len, const int32_t* need_counts, int num_slots, int vocab,
                               const int64_t* gen_tokens, int gen_cap, const int32_t* gen_lens, void* stream) {
    const char* op = "qspec_logit_table_catch_up";
    if (num_slots < 0) return fail("%s: num_slots < 0", op);
    if (num_slots == 0) return 0;
    NONNULL(op, tok_table); NONNULL(op, counted_len); NONNULL(op, need_counts); NONNULL(op, gen_tokens); NONNULL(op, gen_lens);
    if (vocab < 1) return fail("%s: vocab < 1", op);
    if (gen_cap < 1) return fail("%s: gen_cap=%d must be >= 1", op, gen_cap);
    return finish(op, qspec::logit_table_catch_up(num_slots, vocab, tok_table, counted_len, need_counts, gen_tokens, gen_cap,
                                                  gen_lens, ST));
}
int qspec_process_logits(const qspec_half* logits, qspec_half* out, int tokens, int vocab, const uint32_t* tok_table,
                         int num_slots, const int32_t* slot_ids, const int32_t* active_lens, const qspec_half* repetition,
                         const qspec_half* frequency, const qspec_half* presence, const int32_t* min_tokens,
                         const int32_t* gen_base, const int32_t* gen_lens, const int32_t* stop_ids, const int32_t* num_stop_ids,
                         int stop_ids_per_slot, const int64_t* draft_ids, int draft_rows, int64_t ids_stride_b,
                         int64_t ids_stride_k, int rows_per_seq, int j_base, void* stream) {
    return process_logits("qspec_process_logits", false, logits, out, tokens, vocab, tok_table, num_slots, slot_ids,
                          active_lens, repetition, frequency, presence, min_tokens, gen_base, gen_lens, stop_ids, num_stop_ids,
                          stop_ids_per_slot, draft_ids, draft_rows, ids_stride_b, ids_stride_k, rows_per_seq, j_base, nullptr,
                          0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, stream);
}
// Token constraints (include/qspec_hip.h, "token constraints"): vllm/entrypoints/openai/logits_processors.py:10-50 and
// vllm/logits_process.py:48-119 inside the pre-pass launch.
int qspec_process_logits_constrained(const qspec_half* logits, qspec_half* out, int tokens, int vocab,
                                     const uint32_t* tok_table, int num_slots, const int32_t* slot_ids,
                                     const int32_t* active_lens, const qspec_half* repetition, const qspec_half* frequency,
                                     const qspec_half* presence, const int32_t* min_tokens, const int32_t* gen_base,
                                     const int32_t* gen_lens, const int32_t* stop_ids, const int32_t* num_stop_ids,
                                     int stop_ids_per_slot, const int64_t* draft_ids, int draft_rows, int64_t ids_stride_b,
                                     int64_t ids_stride_k, int rows_per_seq, int j_base, const uint32_t* deny, int deny_words,
                                     const int32_t* meta, const int32_t* bias_ids, const float* bias_vals, const int32_t* words,
                                     const int32_t* word_lens, const int32_t* tail, const int64_t* gen_tokens, int gen_cap,
                                     void* stream) {
    return process_logits("qspec_process_logits_constrained", true, logits, out, tokens, vocab, tok_table, num_slots, slot_ids,
                          active_lens, repetition, frequency, presence, min_tokens, gen_base, gen_lens, stop_ids, num_stop_ids,
                          stop_ids_per_slot, draft_ids, draft_rows, ids_stride_b, ids_stride_k, rows_per_seq, j_base, deny,
                          deny_words, meta, bias_ids, bias_vals, words, word_lens, tail, gen_tokens, gen_cap, nullptr, stream);
}
// Token guides (include/qspec_hip.h, "token guides"): vllm/model_executor/guided_decoding/outlines_logits_processors.py:34-93
// inside the pre-pass launch, the automaton resident on the device.
int qspec_process_logits_guided(const qspec_half* logits, qspec_half* out, int tokens, int vocab, const uint32_t* tok_table,
                                int num_slots, const int32_t* slot_ids, const int32_t* active_lens, const qspec_half* repetition,
                                const qspec_half* frequency, const qspec_half* presence, const int32_t* min_tokens,
                                const int32_t* gen_base, const int32_t* gen_lens, const int32_t* stop_ids,
                                const int32_t* num_stop_ids, int stop_ids_per_slot, const int64_t* draft_ids, int draft_rows,
                                int64_t ids_stride_b, int64_t ids_stride_k, int rows_per_seq, int j_base, const uint32_t* deny,
                                int deny_words, const int32_t* meta, const int32_t* bias_ids, const float* bias_vals,
                                const int32_t* words, const int32_t* word_lens, const int32_t* tail, const int64_t* gen_tokens,
                                int gen_cap, const uint32_t* guide_allow, const int32_t* guide_rank, const int32_t* guide_off,
                                const int32_t* guide_next, const int32_t* guide_slots, int guide_words, int guide_states,
                                int guide_transitions, void* stream) {
    const qspec::LpGuide g{guide_allow, guide_rank, guide_off, guide_next, guide_slots, guide_words, guide_states, guide_transitions};
    return process_logits("qspec_process_logits_guided", true, logits, out, tokens, vocab, tok_table, num_slots, slot_ids,
                          active_lens, repetition, frequency, presence, min_tokens, gen_base, gen_lens, stop_ids, num_stop_ids,
                          stop_ids_per_slot, draft_ids, draft_rows, ids_stride_b, ids_stride_k, rows_per_seq, j_base, deny,
                          deny_words, meta, bias_ids, bias_vals, words, word_lens, tail, gen_tokens, gen_cap, &g, stream);
}
int qspec_guide_build(uint32_t* guide_allow, int32_t* guide_rank, int32_t* guide_off, int32_t* guide_next, int guide_words,
                      int row_stride, int vocab, int max_states, int max_transitions, int state_base, int transition_base,
                      int num_states, int num_transitions, const int32_t* row_ptr, const int32_t* tokens,
                      const int32_t* next_states, void* stream) {
    const char* op = "qspec_guide_build";
    NONNULL(op, guide_allow); NONNULL(op, guide_rank); NONNULL(op, guide_off); NONNULL(op, guide_next); NONNULL(op, row_ptr);
    NONNULL(op, tokens); NONNULL(op, next_states);
    if (vocab < 1) return fail("%s: vocab < 1", op);
    if (guide_words < 4 || guide_words % 4 || guide_words > 8192 || (int64_t)guide_words * 32 < vocab)
        return fail("%s: guide_words=%d must be a multiple of 4 in 4..8192 that covers vocab=%d", op, guide_words, vocab);
    if (row_stride < guide_words || row_stride % 4)
        return fail("%s: row_stride=%d must be a multiple of 4 >= guide_words=%d", op, row_stride, guide_words);
    if (num_states < 1 || state_base < 0 || (int64_t)state_base + num_states > max_states)
        return fail("%s: states %d..%d outside the arena's %d", op, state_base, state_base + num_states, max_states);
    if (num_transitions < 1 || transition_base < 0 || (int64_t)transition_base + num_transitions > max_transitions)
        return fail("%s: transitions %d..%d outside the arena's %d", op, transition_base, transition_base + num_transitions,
                    max_transitions);
    return finish(op, qspec::guide_build(guide_allow, guide_rank, guide_off, guide_next, guide_words, row_stride, vocab, state_base,
                                         transition_base, num_states, row_ptr, tokens, next_states, num_transitions, ST));
}
int qspec_guide_catch_up(int32_t* guide_slots, int num_slots, int vocab, const uint32_t* guide_allow, const int32_t* guide_rank,
                         const int32_t* guide_off, const int32_t* guide_next, int guide_words, int guide_states,
                         int guide_transitions, const int64_t* gen_tokens, int gen_cap, const int32_t* gen_lens, void* stream) {
    const char* op = "qspec_guide_catch_up";
    if (num_slots < 0) return fail("%s: num_slots < 0", op);
    if (num_slots == 0) return 0;
    NONNULL(op, guide_slots); NONNULL(op, guide_allow); NONNULL(op, guide_rank); NONNULL(op, guide_off); NONNULL(op, guide_next);
    NONNULL(op, gen_tokens); NONNULL(op, gen_lens);
    if (vocab < 1) return fail("%s: vocab < 1", op);
    if (gen_cap < 1) return fail("%s: gen_cap=%d must be >= 1", op, gen_cap);
    if (guide_words % 4 || (int64_t)guide_words * 32 < vocab)
        return fail("%s: guide_words=%d must be a multiple of 4 that covers vocab=%d", op, guide_words, vocab);
    if (guide_states < 1 || guide_transitions < 1)
        return fail("%s: guide_states=%d / guide_transitions=%d must be >= 1", op, guide_states, guide_transitions);
    const qspec::LpGuide g{guide_allow, guide_rank, guide_off, guide_next, guide_slots, guide_words, guide_states, guide_transitions};
    return finish(op, qspec::guide_catch_up(num_slots, vocab, guide_slots, g, gen_tokens, gen_cap, gen_lens, ST));
}
int qspec_token_constraints_set(uint32_t* deny, int deny_words, int32_t* meta, int32_t* bias_ids, float* bias_vals,
                                int32_t* words, int32_t* word_lens, int num_slots, int vocab, int slot,
                                const int64_t* allowed_ids, int num_allowed, const int64_t* banned_ids, int num_banned,
                                const int32_t* src_bias_ids, const float* src_bias_vals, int num_bias,
                                const int32_t* src_words, const int32_t* src_word_lens, int num_words, int bad_words_present,
                                void* stream) {
    const char* op = "qspec_token_constraints_set";
    NONNULL(op, deny); NONNULL(op, meta); NONNULL(op, bias_ids); NONNULL(op, bias_vals); NONNULL(op, words); NONNULL(op, word_lens);
    if (vocab < 1) return fail("%s: vocab < 1", op);
    if ((int64_t)deny_words * 32 < vocab) return fail("%s: deny_words=%d does not cover vocab=%d", op, deny_words, vocab);
    if (slot < 0 || slot >= num_slots) return fail("%s: slot=%d outside the %d slots", op, slot, num_slots);
    if (num_allowed < 0 || num_banned < 0) return fail("%s: negative id count", op);
    if (num_bias < 0 || num_bias > QS_MAX_LOGIT_BIAS) return fail("%s: num_bias=%d outside 0..%d", op, num_bias, QS_MAX_LOGIT_BIAS);
    if (num_words < 0 || num_words > QS_MAX_BAD_WORDS) return fail("%s: num_words=%d outside 0..%d", op, num_words, QS_MAX_BAD_WORDS);
    if (num_allowed > 0) NONNULL(op, allowed_ids);
    if (num_banned > 0) NONNULL(op, banned_ids);
    if (num_bias > 0) { NONNULL(op, src_bias_ids); NONNULL(op, src_bias_vals); }
    if (num_words > 0) { NONNULL(op, src_words); NONNULL(op, src_word_lens); }
    return finish(op, qspec::token_constraints_set(deny, deny_words, meta, bias_ids, bias_vals, words, word_lens, vocab, slot,
                                                   allowed_ids, num_allowed, banned_ids, num_banned, src_bias_ids, src_bias_vals,
                                                   num_bias, src_words, src_word_lens, num_words, bad_words_present, ST));
}
int qspec_typical_acceptance_sample(const float* target_with_bonus_probs, const int64_t* bonus_token_ids,
                                    const int64_t* draft_token_ids, float posterior_threshold, float posterior_alpha, int batch,
                                    int k, int vocab, int64_t ids_stride_b, int64_t ids_stride_k, int64_t bonus_stride,
                                    int64_t* out_tokens, uint8_t* accepted, int64_t* recovered, int64_t* counters,
                                    const int32_t* active_lens, void* workspace, void* stream) {
    const char* op = "qspec_typical_acceptance_sample";
    if (batch == 0) return 0;
    NONNULL(op, target_with_bonus_probs); NONNULL(op, bonus_token_ids); NONNULL(op, draft_token_ids); NONNULL(op, out_tokens);
    NONNULL(op, accepted); NONNULL(op, recovered); NONNULL(op, workspace);
    if (batch * k > 4096) return fail("%s: batch*k=%d too large", op, batch * k);
    if (k < 1) return fail("%s: k=%d must be >= 1", op, k);
    return finish(op, qspec::typical_acceptance_sample(target_with_bonus_probs, draft_token_ids, bonus_token_ids, posterior_threshold,
                                                       posterior_alpha, batch, k, vocab, ids_stride_b, ids_stride_k, bonus_stride,
                                                       out_tokens, accepted, recovered, counters, active_lens, workspace, ST));
}
int qspec_advance_step_flashattn(int num_seqs, int block_size, int64_t* input_tokens,
                                 const int64_t* sampled_token_ids, int64_t* input_positions, int32_t* seq_lens,
                                 int64_t* slot_mapping, const int32_t* block_tables, int64_t block_tables_stride,
                                 void* stream) {
    const char* op = "qspec_advance_step_flashattn";
    if (num_seqs == 0) return 0;
    NONNULL(op, input_tokens); NONNULL(op, sampled_token_ids); NONNULL(op, input_positions); NONNULL(op, seq_lens);
    NONNULL(op, slot_mapping); NONNULL(op, block_tables);
    return finish(op, qspec::advance_step(num_seqs, block_size, input_tokens, sampled_token_ids, input_positions, seq_lens, slot_mapping, block_tables, block_tables_stride, ST));
}

int qspec_spec_advance_draft(int batch, int block_size, int max_blocks_per_seq, int64_t* input_tokens,
                             const int64_t* sampled_token_ids, int64_t* positions, int32_t* ctx_lens, int64_t* slot_mapping,
                             const int32_t* block_tables, int64_t block_tables_stride, void* stream) {
    return spec_advance_draft("qspec_spec_advance_draft", false, batch, block_size, max_blocks_per_seq, input_tokens,
                              sampled_token_ids, positions, ctx_lens, slot_mapping, block_tables, block_tables_stride, nullptr,
                              nullptr, 0, 0, stream);
}
int qspec_spec_prepare_draft(int batch, int block_size, int max_blocks_per_seq, const int64_t* last_token,
                             const int32_t* seq_lens, const int32_t* block_tables, int64_t block_tables_stride,
                             int64_t* input_tokens, int64_t* positions, int64_t* slot_mapping, int32_t* ctx_lens,
                             void* stream) {
    return spec_prepare_draft("qspec_spec_prepare_draft", false, batch, block_size, max_blocks_per_seq, last_token, seq_lens,
                              nullptr, nullptr, block_tables, block_tables_stride, input_tokens, positions, slot_mapping,
                              ctx_lens, nullptr, nullptr, 0, 0, stream);
}
int qspec_spec_prepare_verify(int batch, int k, int block_size, int max_blocks_per_seq, const int64_t* last_token,
                              const int64_t* draft_token_ids, int64_t ids_stride_b, int64_t ids_stride_k,
                              const int32_t* seq_lens, const int32_t* block_tables, int64_t block_tables_stride,
                              int64_t* tokens, int64_t* positions, int64_t* slot_mapping, int32_t* ctx_lens, void* stream) {
    return spec_prepare_verify("qspec_spec_prepare_verify", false, batch, k, block_size, max_blocks_per_seq, last_token,
                               draft_token_ids, ids_stride_b, ids_stride_k, seq_lens, block_tables, block_tables_stride, tokens,
                               positions, slot_mapping, ctx_lens, nullptr, nullptr, 0, 0, stream);
}
int qspec_spec_prepare_draft_embed(int batch, int block_size, int max_blocks_per_seq, const int64_t* last_token,
                                   const int32_t* seq_lens, const int32_t* step_mask, int32_t* eff_lens,
                                   const int32_t* block_tables, int64_t block_tables_stride, int64_t* input_tokens,
                                   int64_t* positions, int64_t* slot_mapping, int32_t* ctx_lens, const qspec_half* embed_tokens,
                                   qspec_half* hidden_out, int hidden, int vocab, void* stream) {
    return spec_prepare_draft("qspec_spec_prepare_draft_embed", true, batch, block_size, max_blocks_per_seq, last_token,
                              seq_lens, step_mask, eff_lens, block_tables, block_tables_stride, input_tokens, positions,
                              slot_mapping, ctx_lens, embed_tokens, hidden_out, hidden, vocab, stream);
}
int qspec_spec_advance_draft_embed(int batch, int block_size, int max_blocks_per_seq, int64_t* input_tokens,
                                   const int64_t* sampled_token_ids, int64_t* positions, int32_t* ctx_lens,
                                   int64_t* slot_mapping, const int32_t* block_tables, int64_t block_tables_stride,
                                   const qspec_half* embed_tokens, qspec_half* hidden_out, int hidden, int vocab,
                                   void* stream) {
    return spec_advance_draft("qspec_spec_advance_draft_embed", true, batch, block_size, max_blocks_per_seq, input_tokens,
                              sampled_token_ids, positions, ctx_lens, slot_mapping, block_tables, block_tables_stride,
                              embed_tokens, hidden_out, hidden, vocab, stream);
}
int qspec_spec_prepare_verify_embed(int batch, int k, int block_size, int max_blocks_per_seq, const int64_t* last_token,
                                    const int64_t* draft_token_ids, int64_t ids_stride_b, int64_t ids_stride_k,
                                    const int32_t* seq_lens, const int32_t* block_tables, int64_t block_tables_stride,
                                    int64_t* tokens, int64_t* positions, int64_t* slot_mapping, int32_t* ctx_lens,
                                    const qspec_half* embed_tokens, qspec_half* hidden_out, int hidden, int vocab,
                                    void* stream) {
    return spec_prepare_verify("qspec_spec_prepare_verify_embed", true, batch, k, block_size, max_blocks_per_seq, last_token,
                               draft_token_ids, ids_stride_b, ids_stride_k, seq_lens, block_tables, block_tables_stride, tokens,
                               positions, slot_mapping, ctx_lens, embed_tokens, hidden_out, hidden, vocab, stream);
}
int qspec_spec_commit(int batch, int k, const int64_t* out_tokens, int32_t* seq_lens, int64_t* last_token,
                      int64_t* gen_tokens, int32_t* gen_lens, int gen_capacity, void* stream) {
    const char* op = "qspec_spec_commit";
    if (batch == 0) return 0;
    NONNULL(op, out_tokens); NONNULL(op, seq_lens); NONNULL(op, last_token);
    if (gen_tokens) NONNULL(op, gen_lens);
    return finish(op, qspec::spec_commit(batch, k, out_tokens, seq_lens, last_token, gen_tokens, gen_lens, gen_capacity, ST));
}

int qspec_spec_snapshot(int batch, int restore, int32_t* seq_lens, int32_t* gen_lens, int64_t* last_token,
                        int64_t* counters, int64_t* rng_state, int32_t* snap_i32, int64_t* snap_i64, void* stream) {
    const char* op = "qspec_spec_snapshot";
    if (batch < 0) return fail("%s: batch < 0", op);
    NONNULL(op, seq_lens); NONNULL(op, gen_lens); NONNULL(op, last_token); NONNULL(op, counters); NONNULL(op, rng_state);
    NONNULL(op, snap_i32); NONNULL(op, snap_i64);
    return finish(op, qspec::spec_snapshot(batch, restore, seq_lens, gen_lens, last_token, counters, rng_state, snap_i32, snap_i64, ST));
}
int qspec_collect_error_words(int32_t* w0, int32_t* w1, int32_t* w2, int32_t* w3, int clear, int64_t* out, void* stream) {
    const char* op = "qspec_collect_error_words";
    if (!out && !clear) return fail("%s: nothing to do (out == NULL and clear == 0)", op);
    return finish(op, qspec::collect_error_words(w0, w1, w2, w3, clear, out, ST));
}

// logprobs (logprobs.hip): one body for both entry points; LOGITS selects the kernel's input form (fp16 logits / fp32 probs)
static int token_logprobs(const char* op, bool LOGITS, const void* x, int64_t row_stride, const int64_t* token_ids, int rows, int vocab, int num_top,
                          float* token_logprob, int32_t* token_rank, int32_t* top_ids, float* top_logprobs, void* stream) {
    if (rows < 0) return fail("%s: rows < 0", op);
    if (vocab < 1) return fail("%s: vocab = %d < 1", op, vocab);
    if (num_top < 0 || num_top > QS_MAX_LOGPROBS) return fail("%s: num_top = %d outside 0..%d", op, num_top, QS_MAX_LOGPROBS);
    if (row_stride < vocab) return fail("%s: row_stride = %lld < vocab = %d", op, (long long)row_stride, vocab);
    if (rows == 0) return 0;
    NONNULL(op, x); NONNULL(op, token_ids); NONNULL(op, token_logprob); NONNULL(op, token_rank);
    if (num_top > 0) { NONNULL(op, top_ids); NONNULL(op, top_logprobs); }
    if (LOGITS)
        return finish(op, qspec::token_logprobs_from_logits(reinterpret_cast<const f16*>(x), row_stride, token_ids, rows, vocab,
                                                            num_top, token_logprob, token_rank, top_ids, top_logprobs, ST));
    return finish(op, qspec::token_logprobs_from_probs(reinterpret_cast<const float*>(x), row_stride, token_ids, rows, vocab, num_top,
                                                       token_logprob, token_rank, top_ids, top_logprobs, ST));
}
int qspec_token_logprobs_from_probs(const float* probs, int64_t row_stride, const int64_t* token_ids, int rows, int vocab,
                                    int num_top, float* token_logprob, int32_t* token_rank, int32_t* top_ids, float* top_logprobs,
                                    void* stream) {
    return token_logprobs("qspec_token_logprobs_from_probs", false, probs, row_stride, token_ids, rows, vocab, num_top,
                                 token_logprob, token_rank, top_ids, top_logprobs, stream);
}
int qspec_token_logprobs_from_logits(const qspec_half* logits, int64_t row_stride, const int64_t* token_ids, int rows, int vocab,
                                     int num_top, float* token_logprob, int32_t* token_rank, int32_t* top_ids, float* top_logprobs,
                                     void* stream) {
    return token_logprobs("qspec_token_logprobs_from_logits", true, logits, row_stride, token_ids, rows, vocab, num_top,
                                token_logprob, token_rank, top_ids, top_logprobs, stream);
}

size_t qspec_xwg_workspace_bytes(void) { return qspec::xwg_workspace_bytes(); }
int qspec_mlp_hadamard(const qspec_half* act, const qspec_half* hadK, qspec_half* out_f16, int8_t* q, qspec_half* scale,
                       float had_scale, float clip_ratio, int tokens, int intermediate, int K, void* workspace, void* stream) {
    return mlp_hadamard("qspec_mlp_hadamard", 0, act, hadK, out_f16, q, scale, had_scale, clip_ratio, tokens, intermediate, K,
                        workspace, stream);
}
int qspec_mlp_hadamard_xp(const qspec_half* act, const qspec_half* hadK, qspec_half* out_f16, int8_t* q, qspec_half* scale,
                          float had_scale, float clip_ratio, int tokens, int intermediate, int K, void* workspace,
                          void* stream) {
    return mlp_hadamard("qspec_mlp_hadamard_xp", 1, act, hadK, out_f16, q, scale, had_scale, clip_ratio, tokens, intermediate,
                        K, workspace, stream);
}
int qspec_qkv_rope_linear_s4s4(const int8_t* xq, const qspec_half* xs, const int8_t* wq, const qspec_half* ws, qspec_half* qkv,
                               int M, int N, int K, const int64_t* positions, const qspec_half* cos_sin_cache,
                               qspec_half* key_cache, qspec_half* value_cache, const int64_t* slot_mapping, int num_heads,
                               int num_kv_heads, int head_size, int rot_dim, void* stream) {
    return qkv_rope_linear_s4s4("qspec_qkv_rope_linear_s4s4", qspec::KvQuant(), xq, xs, wq, ws, qkv, M, N, K, positions,
                                cos_sin_cache, key_cache, value_cache, slot_mapping, num_heads, num_kv_heads, head_size,
                                rot_dim, stream);
}
int qspec_qkv_rope_linear_supported(int w4a4, int M, int N, int K, int head_size) {
    if (head_size == 128) return 1;   // every shape: the streaming kernels, else the first-generation fused kernels
    if (head_size != 64 || !use_stream()) return 0;
    return (w4a4 ? qspec::gemm_w4a4_stream_supported(M, N, K, false) : qspec::gemm_w4a16_stream_supported(M, N, K)) ? 1 : 0;
}
int qspec_qkv_rope_linear_w4a16(const qspec_half* x, const int8_t* wq, const qspec_half* ws, qspec_half* qkv, int M, int N,
                                int K, const int64_t* positions, const qspec_half* cos_sin_cache, qspec_half* key_cache,
                                qspec_half* value_cache, const int64_t* slot_mapping, int num_heads, int num_kv_heads,
                                int head_size, int rot_dim, void* workspace, void* stream) {
    return qkv_rope_linear_w4a16("qspec_qkv_rope_linear_w4a16", 0, qspec::KvQuant(), x, wq, ws, qkv, M, N, K, positions,
                                 cos_sin_cache, key_cache, value_cache, slot_mapping, num_heads, num_kv_heads, head_size,
                                 rot_dim, workspace, stream);
}
int qspec_qkv_rope_linear_w4a16_xp(const qspec_half* x, const int8_t* wq, const qspec_half* ws, qspec_half* qkv, int M, int N,
                                   int K, const int64_t* positions, const qspec_half* cos_sin_cache, qspec_half* key_cache,
                                   qspec_half* value_cache, const int64_t* slot_mapping, int num_heads, int num_kv_heads,
                                   int head_size, int rot_dim, void* workspace, void* stream) {
    return qkv_rope_linear_w4a16("qspec_qkv_rope_linear_w4a16_xp", 1, qspec::KvQuant(), x, wq, ws, qkv, M, N, K, positions,
                                 cos_sin_cache, key_cache, value_cache, slot_mapping, num_heads, num_kv_heads, head_size,
                                 rot_dim, workspace, stream);
}
int qspec_gate_up_silu_linear_s4s4(const int8_t* xq, const qspec_half* xs, const int8_t* wq, const qspec_half* ws,
                                   qspec_half* act, int M, int intermediate, int K, void* stream) {
    const char* op = "qspec_gate_up_silu_linear_s4s4";
    if (M == 0) return 0;
    NONNULL(op, xq); NONNULL(op, xs); NONNULL(op, wq); NONNULL(op, ws); NONNULL(op, act);
    if (use_stream() && qspec::gemm_w4a4_stream_supported(M, 2 * intermediate, K, false)) {
        qspec::StreamActs x;
        x.xq = xq; x.xs = CH(xs);
        return finish(op, qspec::gemm_w4a4_stream_gate_up_silu(x, wq, CH(ws), H(act), M, intermediate, K, ST));
    }
    return finish(op, qspec::gemm_w4a4_gate_up_silu(xq, CH(xs), wq, CH(ws), H(act), M, intermediate, K, ST));
}
int qspec_gate_up_silu_linear_w4a16(const qspec_half* x, const int8_t* wq, const qspec_half* ws, qspec_half* act, int M,
                                    int intermediate, int K, void* workspace, void* stream) {
    return gate_up_silu_linear_w4a16("qspec_gate_up_silu_linear_w4a16", 0, x, wq, ws, act, M, intermediate, K, workspace,
                                     stream);
}
int qspec_gate_up_silu_linear_w4a16_xp(const qspec_half* x, const int8_t* wq, const qspec_half* ws, qspec_half* act, int M,
                                       int intermediate, int K, void* workspace, void* stream) {
    return gate_up_silu_linear_w4a16("qspec_gate_up_silu_linear_w4a16_xp", 1, x, wq, ws, act, M, intermediate, K, workspace,
                                     stream);
}

int qspec_w4a16_linear_ksliced(const qspec_half* x, int64_t ldx, const int8_t* wq, int64_t ldw_bytes,
                               const qspec_half* ws, qspec_half* out, int M, int N, int K, void* workspace,
                               void* stream) {
    const char* op = "qspec_w4a16_linear_ksliced";
    if (M == 0 || N == 0) return 0;
    NONNULL(op, x); NONNULL(op, wq); NONNULL(op, ws); NONNULL(op, out);
    if (N % 16 || K % 128 || ldw_bytes % 16 || ldx % 8) return fail("%s: need N%%16, K%%128, ldw%%16, ldx%%8 == 0", op);
    if (use_stream() && qspec::gemm_w4a16_stream_supported(M, N, K))
        return finish(op, qspec::gemm_w4a16_stream(CH(x), ldx, wq, ldw_bytes, CH(ws), H(out), M, N, K, ST));
    {
        const int S = (use_stream() && workspace) ? qspec::gemm_w4a16_stream_partial_slices(M, N, K) : 0;
        if (S > 0 && (size_t)S * M * N * sizeof(float) + 8192 <= qspec::gemm_w4a16_ws_bytes()) {
            float* part = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + 8192);
            int rc = qspec::gemm_w4a16_stream_partial(CH(x), ldx, wq, ldw_bytes, part, M, N, K, S, ST);
            if (rc == 0) rc = qspec::gemm_w4a16_partial_finish(part, CH(ws), H(out), M, N, S, ST);
            return finish(op, rc);
        }
    }
    return finish(op, qspec::gemm_w4a16_strided(CH(x), ldx, wq, ldw_bytes, CH(ws), H(out), M, N, K, workspace, ST));
}
int qspec_w4a16_linear_ksliced_raw(const qspec_half* x, int64_t ldx, const int8_t* wq, int64_t ldw_bytes, float* part,
                                   int M, int N, int K, void* workspace, void* stream) {
    const char* op = "qspec_w4a16_linear_ksliced_raw";
    if (M == 0 || N == 0) return 0;
    NONNULL(op, x); NONNULL(op, wq); NONNULL(op, part);
    if (M > 32) return fail("%s: M=%d > 32 (decode-sized verify batches only)", op, M);
    if (N % 16 || K % 128 || ldw_bytes % 16 || ldx % 8) return fail("%s: need N%%16, K%%128, ldw%%16, ldx%%8 == 0", op);
    if (use_stream() && qspec::gemm_w4a16_stream_supported(M, N, K))
        return finish(op, qspec::gemm_w4a16_stream_partial(CH(x), ldx, wq, ldw_bytes, part, M, N, K, 1, ST));
    return finish(op, qspec::gemm_w4a16_strided_raw(CH(x), ldx, wq, ldw_bytes, part, M, N, K, workspace, ST));
}
int qspec_gate_up_silu_linear_w4a16_shard(const qspec_half* x, const int8_t* wq, const qspec_half* ws, qspec_half* act,
                                          int M, int intermediate, int K, int first_channel, int num_channels,
                                          void* workspace, void* stream) {
    const char* op = "qspec_gate_up_silu_linear_w4a16_shard";
    if (M == 0 || num_channels == 0) return 0;
    NONNULL(op, x); NONNULL(op, wq); NONNULL(op, ws); NONNULL(op, act);
    if (use_stream() && qspec::gemm_w4a16_stream_supported(M, 2 * intermediate, K))
        return finish(op, qspec::gemm_w4a16_stream_gate_up_silu(CH(x), wq, CH(ws), H(act), M, intermediate, K, first_channel, num_channels, ST));
    return finish(op, qspec::gemm_w4a16_gate_up_silu(CH(x), wq, CH(ws), H(act), M, intermediate, K, first_channel, num_channels, workspace, ST));
}

int qspec_ln_qkv_rope_linear_s4s4(const qspec_half* hidden_in, const qspec_half* delta, qspec_half* hidden_out, float eps,
                                  const int8_t* wq, const qspec_half* ws, qspec_half* qkv, int M, int N, int K,
                                  const int64_t* positions, const qspec_half* cos_sin_cache, qspec_half* key_cache,
                                  qspec_half* value_cache, const int64_t* slot_mapping, int num_heads, int num_kv_heads,
                                  int head_size, int rot_dim, void* sync_workspace, void* stream) {
    return ln_qkv_rope_linear_s4s4("qspec_ln_qkv_rope_linear_s4s4", qspec::KvQuant(), hidden_in, delta, hidden_out, eps, wq, ws,
                                   qkv, M, N, K, positions, cos_sin_cache, key_cache, value_cache, slot_mapping, num_heads,
                                   num_kv_heads, head_size, rot_dim, sync_workspace, stream);
}
int qspec_ln_gate_up_silu_linear_s4s4(const qspec_half* hidden_in, const qspec_half* delta, qspec_half* hidden_out,
                                      float eps, const int8_t* wq, const qspec_half* ws, qspec_half* act, int M,
                                      int intermediate, int K, void* sync_workspace, void* stream) {
    const char* op = "qspec_ln_gate_up_silu_linear_s4s4";
    if (M == 0) return 0;
    NONNULL(op, hidden_in); NONNULL(op, wq); NONNULL(op, ws); NONNULL(op, act);
    if (hidden_out == hidden_in) return fail("%s: hidden_out must not alias hidden_in (every workgroup reads it)", op);
    if (!qspec::gemm_w4a4_stream_supported(M, 2 * intermediate, K, true) || intermediate % 8)
        return fail("%s: need M <= 16, intermediate %% 8 == 0, K in {1024, 2048, 4096, 5120, 8192} (M=%d I=%d K=%d)", op, M, intermediate, K);
    qspec::StreamActs x;
    x.hidden_in = CH(hidden_in); x.delta = CH(delta); x.hidden_out = H(hidden_out); x.eps = eps;
    x.sync = reinterpret_cast<int*>(sync_workspace);
    return finish(op, qspec::gemm_w4a4_stream_gate_up_silu(x, wq, CH(ws), H(act), M, intermediate, K, ST));
}
size_t qspec_ln_linear_workspace_bytes(void) { return qspec::gemm_w4a4_stream_sync_bytes(); }
int qspec_w4a16_linear_partial_slices(int M, int N, int K) { return w4a16_linear_partial_slices(M, N, K); }
int qspec_w4a16_linear_partial(const qspec_half* x, const int8_t* wq, float* part, int M, int N, int K, int slices,
                               void* stream) {
    return w4a16_linear_partial("qspec_w4a16_linear_partial", 0, x, wq, part, M, N, K, slices, stream);
}
int qspec_w4a16_linear_partial_xp(const qspec_half* x, const int8_t* wq, float* part, int M, int N, int K, int slices,
                                  void* stream) {
    return w4a16_linear_partial("qspec_w4a16_linear_partial_xp", 1, x, wq, part, M, N, K, slices, stream);
}
int qspec_add_rms_norm_fp16_partial(qspec_half* out, qspec_half* hidden_out, const qspec_half* x, const float* part,
                                    const qspec_half* ws, int slices, float eps, int tokens, int hidden, void* stream) {
    return add_rms_norm_fp16_partial("qspec_add_rms_norm_fp16_partial", 0, out, hidden_out, x, part, ws, slices, eps, tokens,
                                     hidden, stream);
}
int qspec_add_rms_norm_fp16_partial_xp(qspec_half* out, qspec_half* hidden_out, const qspec_half* x, const float* part,
                                       const qspec_half* ws, int slices, float eps, int tokens, int hidden, void* stream) {
    return add_rms_norm_fp16_partial("qspec_add_rms_norm_fp16_partial_xp", 1, out, hidden_out, x, part, ws, slices, eps, tokens,
                                     hidden, stream);
}
int qspec_rowwise_scaled_linear_s4s4_partial_slices(int M, int N, int K) { return qspec::gemm_w4a4_stream_partial_slices(M, N, K); }
int qspec_rowwise_scaled_linear_s4s4_partial(const int8_t* xq, const int8_t* wq, int32_t* ipart, int M, int N, int K, int slices,
                                             void* stream) {
    const char* op = "qspec_rowwise_scaled_linear_s4s4_partial";
    if (M <= 0 || N <= 0) return fail("%s: empty problem", op);
    NONNULL(op, xq); NONNULL(op, wq); NONNULL(op, ipart);
    if (slices < 2 || slices != qspec::gemm_w4a4_stream_partial_slices(M, N, K))
        return fail("%s: (M=%d N=%d K=%d) is not built for %d K slices (ask qspec_rowwise_scaled_linear_s4s4_partial_slices)", op, M, N, K, slices);
    return finish(op, qspec::gemm_w4a4_stream_partial(xq, wq, ipart, M, N, K, slices, ST));
}
int qspec_add_rms_norm_ipartial(int8_t* q, qspec_half* scale, qspec_half* out_f16, qspec_half* hidden_out, const qspec_half* x,
                                const int32_t* ipart, const qspec_half* xs, const qspec_half* ws, int slices, float eps,
                                int tokens, int hidden, void* stream) {
    const char* op = "qspec_add_rms_norm_ipartial";
    if (tokens < 0) return fail("%s: tokens < 0", op);
    if (tokens == 0) return 0;
    NONNULL(op, x); NONNULL(op, ipart); NONNULL(op, xs); NONNULL(op, ws); NONNULL(op, hidden_out);
    if (q) { NONNULL(op, scale); } else { NONNULL(op, out_f16); }
    if (slices < 1) return fail("%s: slices < 1", op);
    if (hidden % 1024 || hidden > 8192 || hidden <= 0) return fail("%s: hidden=%d must be a multiple of 1024, <= 8192", op, hidden);
    return finish(op, qspec::ln_ipartial(CH(x), ipart, CH(xs), CH(ws), slices, H(hidden_out), H(out_f16), q, H(scale), eps, tokens,
                                         hidden, ST));
}
#ifdef QS_EXPERIMENTAL   // (csrc/experimental/qspec_hip_experimental.h)
int qspec_prefetch(const void* p, size_t bytes, int workgroups, void* stream) {
    const char* op = "qspec_prefetch";
    if (bytes == 0) return 0;
    NONNULL(op, p);
    if (((uintptr_t)p) % 16) return fail("%s: pointer must be 16-byte aligned", op);
    return finish(op, qspec::prefetch_l2(p, bytes, workgroups, ST));
}
int qspec_prefetch_tiles(const void* p, size_t tile_bytes, int first_tile, int ntiles, int workgroups, void* stream) {
    const char* op = "qspec_prefetch_tiles";
    if (ntiles <= 0) return 0;
    NONNULL(op, p);
    if (((uintptr_t)p) % 16 || tile_bytes % 16) return fail("%s: pointer and tile_bytes must be multiples of 16", op);
    return finish(op, qspec::prefetch_tiles(p, tile_bytes, first_tile, ntiles, workgroups, ST));
}
#endif
int qspec_ln_linear_s4s4_supported(int M, int N, int K) { return qspec::gemm_w4a4_stream_supported(M, N, K, true) ? 1 : 0; }

/* ---- FP8 (e4m3fn) KV cache: the bodies of the fp16 entries, handed the scales (qspec_hip.h, "FP8 KV cache") ---- */
int qspec_reshape_and_cache_flash_kv8(const qspec_half* key, const qspec_half* value, uint8_t* key_cache, uint8_t* value_cache,
                                      float k_scale, float v_scale, const int64_t* slot_mapping, int tokens, int num_kv_heads,
                                      int head_size, int64_t key_stride, int64_t value_stride, void* stream) {
    KV_SCALES("qspec_reshape_and_cache_flash_kv8");
    return reshape_and_cache_flash("qspec_reshape_and_cache_flash_kv8", kq, key, value, key_cache, value_cache, slot_mapping,
                                   tokens, num_kv_heads, head_size, key_stride, value_stride, stream);
}
int qspec_rope_kv_write_kv8(const int64_t* positions, qspec_half* qkv, const qspec_half* cos_sin_cache, uint8_t* key_cache,
                            uint8_t* value_cache, float k_scale, float v_scale, const int64_t* slot_mapping, int tokens,
                            int num_heads, int num_kv_heads, int head_size, int rot_dim, void* stream) {
    KV_SCALES("qspec_rope_kv_write_kv8");
    return rope_kv_write("qspec_rope_kv_write_kv8", kq, positions, qkv, cos_sin_cache, key_cache, value_cache, slot_mapping,
                         tokens, num_heads, num_kv_heads, head_size, rot_dim, stream);
}
int qspec_paged_attention_kv8(const qspec_half* q, int64_t q_stride, const uint8_t* key_cache, const uint8_t* value_cache,
                              float k_scale, float v_scale, const int32_t* block_tables, int max_blocks_per_seq,
                              const int32_t* ctx_lens, const int32_t* q_start, int n_seqs, int tokens, int max_q_len,
                              int num_heads, int num_kv_heads, int head_size, int block_size, float sm_scale, int n_splits,
                              void* workspace, qspec_half* out, void* stream) {
    KV_SCALES("qspec_paged_attention_kv8");
    return paged_attention("qspec_paged_attention_kv8", kq, q, q_stride, key_cache, value_cache, block_tables,
                           max_blocks_per_seq, ctx_lens, q_start, n_seqs, tokens, max_q_len, num_heads, num_kv_heads, head_size,
                           block_size, sm_scale, n_splits, workspace, out, stream);
}
int qspec_qkv_rope_linear_s4s4_kv8(const int8_t* xq, const qspec_half* xs, const int8_t* wq, const qspec_half* ws,
                                   qspec_half* qkv, int M, int N, int K, const int64_t* positions,
                                   const qspec_half* cos_sin_cache, uint8_t* key_cache, uint8_t* value_cache, float k_scale,
                                   float v_scale, const int64_t* slot_mapping, int num_heads, int num_kv_heads, int head_size,
                                   int rot_dim, void* stream) {
    KV_SCALES("qspec_qkv_rope_linear_s4s4_kv8");
    return qkv_rope_linear_s4s4("qspec_qkv_rope_linear_s4s4_kv8", kq, xq, xs, wq, ws, qkv, M, N, K, positions, cos_sin_cache,
                                key_cache, value_cache, slot_mapping, num_heads, num_kv_heads, head_size, rot_dim, stream);
}
int qspec_qkv_rope_linear_w4a16_kv8(const qspec_half* x, const int8_t* wq, const qspec_half* ws, qspec_half* qkv, int M, int N,
                                    int K, const int64_t* positions, const qspec_half* cos_sin_cache, uint8_t* key_cache,
                                    uint8_t* value_cache, float k_scale, float v_scale, const int64_t* slot_mapping,
                                    int num_heads, int num_kv_heads, int head_size, int rot_dim, void* workspace,
                                    void* stream) {
    KV_SCALES("qspec_qkv_rope_linear_w4a16_kv8");
    return qkv_rope_linear_w4a16("qspec_qkv_rope_linear_w4a16_kv8", 0, kq, x, wq, ws, qkv, M, N, K, positions, cos_sin_cache,
                                 key_cache, value_cache, slot_mapping, num_heads, num_kv_heads, head_size, rot_dim, workspace,
                                 stream);
}
int qspec_qkv_rope_linear_w4a16_xp_kv8(const qspec_half* x, const int8_t* wq, const qspec_half* ws, qspec_half* qkv, int M,
                                       int N, int K, const int64_t* positions, const qspec_half* cos_sin_cache,
                                       uint8_t* key_cache, uint8_t* value_cache, float k_scale, float v_scale,
                                       const int64_t* slot_mapping, int num_heads, int num_kv_heads, int head_size, int rot_dim,
                                       void* workspace, void* stream) {
    KV_SCALES("qspec_qkv_rope_linear_w4a16_xp_kv8");
    return qkv_rope_linear_w4a16("qspec_qkv_rope_linear_w4a16_xp_kv8", 1, kq, x, wq, ws, qkv, M, N, K, positions, cos_sin_cache,
                                 key_cache, value_cache, slot_mapping, num_heads, num_kv_heads, head_size, rot_dim, workspace,
                                 stream);
}
int qspec_qkv_rope_linear_w4a16_xp32_kv8(const qspec_half* x, const int8_t* wq, const qspec_half* ws, qspec_half* qkv, int M,
                                         int N, int K, const int64_t* positions, const qspec_half* cos_sin_cache,
                                         uint8_t* key_cache, uint8_t* value_cache, float k_scale, float v_scale,
                                         const int64_t* slot_mapping, int num_heads, int num_kv_heads, int head_size,
                                         int rot_dim, void* stream) {
    KV_SCALES("qspec_qkv_rope_linear_w4a16_xp32_kv8");
    return qkv_rope_linear_w4a16_xp32("qspec_qkv_rope_linear_w4a16_xp32_kv8", kq, x, wq, ws, qkv, M, N, K, positions,
                                      cos_sin_cache, key_cache, value_cache, slot_mapping, num_heads, num_kv_heads, head_size,
                                      rot_dim, stream);
}
int qspec_ln_qkv_rope_linear_s4s4_kv8(const qspec_half* hidden_in, const qspec_half* delta, qspec_half* hidden_out, float eps,
                                      const int8_t* wq, const qspec_half* ws, qspec_half* qkv, int M, int N, int K,
                                      const int64_t* positions, const qspec_half* cos_sin_cache, uint8_t* key_cache,
                                      uint8_t* value_cache, float k_scale, float v_scale, const int64_t* slot_mapping,
                                      int num_heads, int num_kv_heads, int head_size, int rot_dim, void* sync_workspace,
                                      void* stream) {
    KV_SCALES("qspec_ln_qkv_rope_linear_s4s4_kv8");
    return ln_qkv_rope_linear_s4s4("qspec_ln_qkv_rope_linear_s4s4_kv8", kq, hidden_in, delta, hidden_out, eps, wq, ws, qkv, M,
                                   N, K, positions, cos_sin_cache, key_cache, value_cache, slot_mapping, num_heads,
                                   num_kv_heads, head_size, rot_dim, sync_workspace, stream);
}

// ---- KV block operations (cache_ops.hip)
static int block_op_args(const char* op, const void* layer_ptrs, int num_layers, const void* ids, int n, int64_t block_bytes) {
    if (num_layers < 1) return fail("%s: num_layers = %d < 1", op, num_layers);
    if (n < 0) return fail("%s: negative block count", op);
    if (block_bytes < 16 || block_bytes % 16) return fail("%s: block_bytes = %lld is not a positive multiple of 16", op, (long long)block_bytes);
    if (n > 0 && (!layer_ptrs || !ids)) return fail("%s: a NULL pointer with %d blocks to move", op, n);
    return 0;
}
int qspec_copy_blocks(void* const* layer_ptrs, int num_layers, const int64_t* pairs, int num_pairs, int64_t block_bytes,
                      void* stream) {
    const char* op = "qspec_copy_blocks";
    if (int rc = block_op_args(op, layer_ptrs, num_layers, pairs, num_pairs, block_bytes)) return rc;
    if (num_pairs == 0) return 0;
    return finish(op, qspec::copy_blocks(layer_ptrs, num_layers, pairs, num_pairs, block_bytes, ST));
}
int qspec_gather_blocks(void* const* layer_ptrs, int num_layers, const int64_t* block_ids, int n, int64_t block_bytes,
                        void* staging, void* stream) {
    const char* op = "qspec_gather_blocks";
    if (int rc = block_op_args(op, layer_ptrs, num_layers, block_ids, n, block_bytes)) return rc;
    if (n == 0) return 0;
    NONNULL(op, staging);
    return finish(op, qspec::gather_blocks(layer_ptrs, num_layers, block_ids, n, block_bytes, staging, ST));
}
int qspec_scatter_blocks(void* const* layer_ptrs, int num_layers, const int64_t* block_ids, int n, int64_t block_bytes,
                         const void* staging, void* stream) {
    const char* op = "qspec_scatter_blocks";
    if (int rc = block_op_args(op, layer_ptrs, num_layers, block_ids, n, block_bytes)) return rc;
    if (n == 0) return 0;
    NONNULL(op, staging);
    return finish(op, qspec::scatter_blocks(layer_ptrs, num_layers, block_ids, n, block_bytes, staging, ST));
}

}  // extern "C"
