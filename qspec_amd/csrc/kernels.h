// Internal C++ launch functions behind the C ABI (include/qspec_hip.h).
// Every function enqueues on `st`, never synchronises, returns 0 or a
// negative code for an unsupported shape (the C ABI turns it into an error string).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

// Dev knobs (environment switches for A/B measurements and sweeps) exist only in the EXPERIMENTAL build
// (-DQS_EXPERIMENTAL: `make -C qspec_amd/csrc experimental`); in libqspec_hip.so every knob is its default, a constant.
#ifdef QS_EXPERIMENTAL
#define QS_DEV_KNOB(name, dflt) (getenv(name) ? atoi(getenv(name)) : (dflt))
#else
#define QS_DEV_KNOB(name, dflt) (dflt)
#endif

namespace qspec {
typedef _Float16 f16;

// FP8 (e4m3fn) KV cache, the `_kv8` entries of the C ABI: the cache pointers of the functions below address bytes instead of
// halves (same element positions), a writer stores e4m3_rne(clamp(f(x) * inv, -448, 448)), a reader folds k_scale into the
// softmax scale and multiplies the stored output by v_scale.  Default-constructed = the fp16 cache.
struct KvQuant {
    int fp8 = 0;
    float k_scale = 1.0f, v_scale = 1.0f;   // readers
    float k_inv = 1.0f, v_inv = 1.0f;       // writers: 1.0f / scale, computed once on the host in fp32
};

// norm_quant.hip
int ln_quant_i4(const f16* x, const f16* delta, f16* hidden_out, int8_t* q, f16* scale, f16* isum, float eps, int T,
                int H, hipStream_t st);
int ln_fp16(const f16* x, const f16* delta, f16* hidden_out, f16* out, float eps, int T, int H, hipStream_t st, int xp = 0);
// delta = h((part[0] + ... + part[S-1])[t, :] * f(ws[:])): the K-sliced W4A16 projection finished inside the norm
int ln_ipartial(const f16* x, const int* ipart, const f16* xs, const f16* ws, int S, f16* hidden_out, f16* out, int8_t* q,
                f16* scale, float eps, int T, int H, hipStream_t st);
int ln_fp16_partial(const f16* x, const float* part, const f16* ws, int S, f16* hidden_out, f16* out, float eps, int T,
                    int H, hipStream_t st, int xp = 0);
int rowabsmax_quant(const f16* x, f16* scale, int8_t* q, float clip, int T, int K, hipStream_t st);

// hadamard.hip
int fwht(const f16* x, float scale, f16* out, int64_t rows, int N, hipStream_t st);
int hadk_mix(const f16* y, const f16* hadK, f16* out, int T, int K, int M, hipStream_t st);
int heads_hadamard(const f16* attn, f16* out_f16, int8_t* q, f16* scale, float had_scale, float clip, int T,
                   int heads, int d, hipStream_t st);
int heads_hadamard_mix(const f16* attn, const f16* hadK, f16* out, float had_scale, int T, int heads, int d, int K,
                       hipStream_t st);
int heads_hadamard_merge(const float* ws, int max_tokens, int n_splits, f16* out_f16, int8_t* q, f16* scale,
                         float had_scale, float clip, int T, int heads, int d, hipStream_t st, int xp = 0);
int silu_mul(const f16* gate_up, f16* out, int T, int I, hipStream_t st);
bool mlp_hadamard_xperm_supported(int T, int I, int K);
// 17..32 tokens: two fragment-major 16-row tiles, the two-token-tile streaming kernel (gemm_stream_w4a16.hip: gemm_w4a16_stream2_kernel)
bool gemm_w4a16_stream32_supported(int M, int N, int K);
int gemm_w4a16_stream32_partial_slices(int M, int N, int K);
int gemm_w4a16_stream32_partial(const f16* x, const int8_t* wq, float* part, int M, int N, int K, int S, hipStream_t st);
int gemm_w4a16_stream32(const f16* x, const int8_t* wq, const f16* ws, f16* out, int M, int N, int K, hipStream_t st);
int gemm_w4a16_stream32_qkv_rope(const f16* x, const int8_t* wq, const f16* ws, f16* qkv, int M, int N, int K,
                                 const int64_t* positions, const f16* cos_sin_cache, f16* key_cache, f16* value_cache,
                                 const int64_t* slot_mapping, int nq, int nkv, int d, int rot_dim, hipStream_t st, KvQuant kq = KvQuant());
int gemm_w4a16_stream32_gate_up_silu(const f16* x, const int8_t* wq, const f16* ws, f16* act, int M, int I, int K, hipStream_t st);
int silu_mul_hadamard(const f16* gate_up, const f16* hadK, f16* out_f16, int8_t* q, f16* scale, float had_scale,
                      float clip, int T, int I, int K, int pre_activated, void* xws, hipStream_t st, int xp = 0);
size_t xwg_workspace_bytes();

// gemm.hip
int gemm_w4a4(const int8_t* xq, const f16* xs, const int8_t* wq, const f16* ws, const f16* bias, f16* out, int M,
              int N, int K, hipStream_t st);
size_t gemm_w4a16_ws_bytes();
int gemm_w4a16(const f16* x, const int8_t* wq, const f16* ws, const f16* bias, f16* out, int M, int N, int K,
               void* wsp, hipStream_t st);
int gemm_w4a4_qkv_rope(const int8_t* xq, const f16* xs, const int8_t* wq, const f16* ws, f16* qkv, int M, int N, int K,
                       const int64_t* positions, const f16* cos_sin_cache, f16* key_cache, f16* value_cache,
                       const int64_t* slot_mapping, int nq, int nkv, int d, int rot_dim, hipStream_t st, KvQuant kq = KvQuant());
int gemm_w4a16_qkv_rope(const f16* x, const int8_t* wq, const f16* ws, f16* qkv, int M, int N, int K,
                        const int64_t* positions, const f16* cos_sin_cache, f16* key_cache, f16* value_cache,
                        const int64_t* slot_mapping, int nq, int nkv, int d, int rot_dim, void* wsp, hipStream_t st, KvQuant kq = KvQuant());
int gemm_w4a4_gate_up_silu(const int8_t* xq, const f16* xs, const int8_t* wq, const f16* ws, f16* act, int M, int I,
                           int K, hipStream_t st);
int gemm_w4a16_gate_up_silu(const f16* x, const int8_t* wq, const f16* ws, f16* act, int M, int I, int K, int ch0,
                            int nch, void* wsp, hipStream_t st);
int gemm_w4a16_strided_raw(const f16* x, int64_t ldx, const int8_t* wq, int64_t ldw, float* part, int M, int N, int K,
                           void* wsp, hipStream_t st);
int gemm_w4a16_strided(const f16* x, int64_t ldx, const int8_t* wq, int64_t ldw, const f16* ws, f16* out, int M, int N,
                       int K, void* wsp, hipStream_t st);
int gemm_f16(const f16* x, const f16* w, f16* out, int M, int N, int K, hipStream_t st);
int dequant_w4(const int8_t* wq, const f16* ws, f16* out, int N, int K, hipStream_t st);

// gemm_stream_w4a4.hip: W4A4 for M <= 16 with the activations produced in the prologue.
// Either (xq, xs) -- packed int4 rows + scales -- or (hidden_in, delta, hidden_out, eps): the residual add +
// LN-no-gamma + int4 quant of quarot_llama.py:373-388 fused in front of the GEMM (hidden_out != hidden_in).
struct StreamActs {
    const int8_t* xq = nullptr;
    const f16* xs = nullptr;
    const f16* hidden_in = nullptr;
    const f16* delta = nullptr;
    f16* hidden_out = nullptr;
    float eps = 0.0f;
    int* sync = nullptr;   // gemm_w4a4_stream_sync_bytes() bytes, zero-filled once: LN by producer workgroups + hand-off
};
size_t gemm_w4a4_stream_sync_bytes();
bool gemm_w4a4_stream_supported(int M, int N, int K, bool ln);
int gemm_w4a4_stream(const StreamActs& x, const int8_t* wq, const f16* ws, f16* out, int M, int N, int K,
                     hipStream_t st);
int gemm_w4a4_stream_residual(const StreamActs& x, const int8_t* wq, const f16* ws, const f16* resid_in, f16* resid_out,
                              int M, int N, int K, hipStream_t st);
// the same launch fed with fp16 rows + `nparts` partial row maxima each: row-absmax int4 quantisation (quant.cu:102-167) in the
// prologue (M <= 4, K = 4096, nparts = 8: the spread head-Hadamard's output)
int gemm_w4a4_stream_residual_hq(const f16* x16, const float* part_amax, int nparts, float clip, const int8_t* wq, const f16* ws,
                                 const f16* resid_in, f16* resid_out, int M, int N, int K, hipStream_t st);
bool gemm_w4a4_stream_residual_hq_supported(int M, int N, int K, int nparts);
int gemm_w4a4_stream_partial_slices(int M, int N, int K);
int gemm_w4a4_stream_partial(const int8_t* xq, const int8_t* wq, int* ipart, int M, int N, int K, int S, hipStream_t st);
int heads_hadamard_mix_merge_spread(const float* ws, int max_tokens, int n_splits, const f16* hadK, f16* out_f16,
                                    float* part_amax, float had_scale, int T, int heads, int d, int K, hipStream_t st, int xp = 0);
bool heads_hadamard_mix_merge_spread_supported(int T, int heads, int d, int K);
int heads_hadamard_merge_spread(const float* ws, int max_tokens, int n_splits, f16* out_f16, float* part_amax, float had_scale,
                                int T, int heads, int d, hipStream_t st);
int gemm_w4a4_stream_qkv_rope(const StreamActs& x, const int8_t* wq, const f16* ws, f16* qkv, int M, int N, int K,
                              const int64_t* positions, const f16* cos_sin_cache, f16* key_cache, f16* value_cache,
                              const int64_t* slot_mapping, int nq, int nkv, int d, int rot_dim, hipStream_t st, KvQuant kq = KvQuant());
int gemm_w4a4_stream_gate_up_silu(const StreamActs& x, const int8_t* wq, const f16* ws, f16* act, int M, int I, int K,
                                  hipStream_t st);

// gemm_stream_w4a16.hip: W4A16 on the same streaming skeleton (M <= 16, K = 128 * NW * UB for a built (NW, UB))
bool gemm_w4a16_stream_supported(int M, int N, int K);
bool gemm_w4a16_xperm_supported(int M, int K);
int gemm_w4a16_stream(const f16* x, int64_t ldx, const int8_t* wq, int64_t ldw, const f16* ws, f16* out, int M, int N,
                      int K, hipStream_t st, int xperm = 0);
int gemm_w4a16_stream_partial_slices(int M, int N, int K);
int gemm_w4a16_stream_partial(const f16* x, int64_t ldx, const int8_t* wq, int64_t ldw, float* part, int M, int N, int K,
                              int S, hipStream_t st, int xperm = 0);
int gemm_w4a16_partial_finish(const float* part, const f16* ws, f16* out, int M, int N, int S, hipStream_t st);
int gemm_w4a16_stream_qkv_rope(const f16* x, const int8_t* wq, const f16* ws, f16* qkv, int M, int N, int K,
                               const int64_t* positions, const f16* cos_sin_cache, f16* key_cache, f16* value_cache,
                               const int64_t* slot_mapping, int nq, int nkv, int d, int rot_dim, hipStream_t st, int xperm = 0,
                               KvQuant kq = KvQuant());
int gemm_w4a16_stream_gate_up_silu(const f16* x, const int8_t* wq, const f16* ws, f16* act, int M, int I, int K, int ch0,
                                   int nch, hipStream_t st, int xperm = 0);

// gemm_tiled.hip: W4A16 for prefill-sized M (tiles of 32..128 tokens x 128 weight rows, 32x32x16 MFMA)
bool gemm_w4a16_tiled_supported(int M, int N, int K);
// part (may be NULL): part_bytes of fp32 scratch for the K-sliced plan of narrow layers
int gemm_w4a16_tiled_partial_slices(int M, int N, int K);
int gemm_w4a16_tiled_partial(const f16* x, const int8_t* wq, float* part, int M, int N, int K, int S, hipStream_t st);
int gemm_w4a16_tiled(const f16* x, const int8_t* wq, const f16* ws, f16* out, int M, int N, int K, float* part,
                     size_t part_bytes, hipStream_t st);

bool gemm_f16_tiled_supported(int M, int N, int K);
int gemm_f16_tiled(const f16* x, const f16* w, f16* out, int M, int N, int K, hipStream_t st);

// gemm_stream_f16.hip: the lm_head (fp16 x fp16^T) on the same streaming skeleton
bool gemm_f16_stream_supported(int M, int N, int K);
int gemm_f16_stream(const f16* x, const f16* w, f16* out, int M, int N, int K, void* part_max, hipStream_t st);
int gemm_f16_stream_grid(int N);
#ifdef QS_EXPERIMENTAL
int prefetch_l2(const void* p, size_t bytes, int workgroups, hipStream_t st);
int prefetch_tiles(const void* p, size_t tile_bytes, int first_tile, int ntiles, int workgroups, hipStream_t st);
#endif

// rope_cache.hip
int rope_kv_write(const int64_t* positions, f16* qkv, const f16* cos_sin_cache, void* key_cache, void* value_cache,
                  const int64_t* slot_mapping, int T, int nq, int nkv, int d, int rot_dim, hipStream_t st, KvQuant kq = KvQuant());
int rotary_embedding(const int64_t* positions, f16* q, f16* k, const f16* cos_sin_cache, int T, int nq, int nkv,
                     int d, int rot_dim, int64_t q_stride, int64_t k_stride, hipStream_t st);
int reshape_and_cache_flash(const f16* key, const f16* value, void* key_cache, void* value_cache,
                            const int64_t* slot_mapping, int T, int nkv, int d, int64_t k_stride, int64_t v_stride,
                            hipStream_t st, KvQuant kq = KvQuant());
// attention.hip (host plan; kernels in attention_decode.hip, attention_prefill.hip, attention_generic.hip; the workspace layout
// the consumers of the partials read: attention_common.cuh, attn_ws)
int paged_attention(const f16* q, int64_t q_stride, const void* key_cache, const void* value_cache,
                    const int32_t* block_tables, int max_blocks, const int32_t* ctx_lens, const int32_t* q_start,
                    int n_seqs, int max_q_len, int nq, int nkv, int d, int block_size, float sm_scale, int n_splits,
                    float* ws, f16* out, hipStream_t st, KvQuant kq = KvQuant());
size_t paged_attention_ws_bytes(int T, int nq, int d, int n_splits);
int paged_attention_family(int n_seqs, int max_q_len, int nq, int nkv, int d, int block_size, int max_blocks, int n_splits,
                           bool merged);   // the AttnFamily (attention_common.cuh) of the call's launch plan; no HIP call
int paged_attention_generic_splits(int n_splits);   // head sizes other than 128: the splits actually used for a caller's n_splits

// sampler.hip
int embedding(const int64_t* ids, const f16* table, f16* out, int T, int H, int V, hipStream_t st);
size_t sampler_ws_bytes(int rows);
int softmax_argmax(const f16* logits, float* probs, int64_t* token, int T, int V, void* ws, hipStream_t st);
// sampler front end behind an lm_head launch that left per-workgroup row maxima (gemm_f16_stream, part_max)
size_t head_softmax_ws_bytes(int rows);
void* head_softmax_part_max(void* ws, int rows);
int head_softmax_argmax(const f16* logits, float* probs, int64_t* token, int T, int V, int nparts, void* ws, hipStream_t st);
// Per-sequence seeded draws (sampler.hip, "Per-sequence seeded draws"); seeds == NULL: every row draws from the engine stream
struct SeedRows {
    const int64_t* seeds;      // [nseq]
    const int32_t* seeded;     // [nseq], 0 = the engine stream
    const int32_t* base_pos;   // [nseq]
    int rows_per_seq;          // row t -> sequence t / rows_per_seq, j = j_base + t % rows_per_seq
    int j_base;
    uint32_t stream;           // 1 draft sample, 2 target sample, 3 rejection exponential, 4 rejection uniform
};
struct RejectionArgs {
    const float *target_probs, *draft_probs;
    const int64_t *draft_ids, *bonus_ids;
    const float *uniform, *exponential;
    uint64_t seed, offset;
    uint64_t* rng_state;
    int B, k, V;
    int64_t dp_sb, dp_sk, di_sb, di_sk, bonus_stride;
    int64_t* out_tokens;
    uint8_t* accepted;
    int64_t *recovered, *counters;
    const int32_t* active_lens;
    SeedRows sr;   // sequence b = batch row b: the three arrays are [B]; the kernels map (b, i) and the stream themselves
    void* ws;
};
int rejection_sample(const RejectionArgs& a, hipStream_t st);
size_t sample_ws_bytes(int rows);
struct SampleArgs {
    const f16* logits;
    const float* temperature;
    const int32_t* top_k;
    const float *top_p, *min_p;   // min_p [T] fp32 per row, or NULL: none -- the selection kernel without it, bit for bit
    const float* exponential;
    uint64_t seed, offset;
    uint64_t* rng_state;
    float* probs;
    int64_t* token;
    int64_t token_stride;
    int T, V;
    SeedRows sr;
    int nseq;                     // rows of sr's arrays
    void* ws;
};
int sample_top_k_top_p(const SampleArgs& a, hipStream_t st);
// logit processors (min_tokens, repetition / frequency / presence penalties) and the per-slot token table they read
int logit_table_set_prompt(uint32_t* table, int V, int slot, const int64_t* prompt, int n_prompt, const int64_t* outputs,
                           int n_out, int32_t* counted_len, hipStream_t st);
int logit_table_catch_up(int B, int V, uint32_t* table, int32_t* counted_len, const int32_t* need, const int64_t* gen_tokens,
                         int gen_cap, const int32_t* gen_lens, hipStream_t st);
struct LpArgs {
    const f16* logits;            // [T, V] raw
    f16* out;                     // [T, V] processed (out of place)
    const uint32_t* table;        // [nslots, V]
    const int32_t* slot_ids;      // [nseq] slot of sequence s, or NULL: s itself
    const int32_t* active_lens;   // [nslots] or NULL: a slot with active_lens <= 0 is copied through
    const f16 *rep, *freq, *pres; // [nslots]
    const int32_t* min_tokens;    // [nslots]
    const int32_t* gen_base;      // [nslots] outputs the request had before admission
    const int32_t* gen_lens;      // [nslots] outputs committed since (at the start of the cycle)
    const int32_t* stop_ids;      // [nslots, stop_width]
    const int32_t* n_stop;        // [nslots]
    const int64_t* draft_ids;     // in-flight token i (0-based) of slot b at b * di_sb + i * di_sk; NULL: none
    int64_t di_sb, di_sk;
    int V, rows_per_seq, j_base, nslots, stop_width;   // stop_width <= QS_LP_MAX_STOP: row width of stop_ids
};
// token constraints (logit_bias, allowed_token_ids, bad words) in front of the pipeline above, inside the same launch: the
// per-slot state sampler.hip describes ("Token constraints"); deny == NULL: none
struct LpCons {
    const uint32_t* deny;
    const int32_t* meta;
    const int32_t* bias_ids;
    const float* bias_vals;
    const int32_t* words;
    const int32_t* word_lens;
    const int32_t* tail;
    const int64_t* gen_tokens;    // [nslots, gen_cap] the outputs committed since admission
    int gen_cap, deny_words;
};
struct LpArgsC : LpArgs { LpCons c; };
// token guides (guided decoding: a DFA over token ids per slot) in front of the token constraints, inside the same launch: the
// arena and the per-slot state sampler.hip describes ("Token guides"); allow == NULL: none
struct LpGuide {
    const uint32_t* allow;        // [states, words] bit v of row s: token v is allowed in state s
    const int32_t* rank;          // [states, words] exclusive prefix popcount of the allow row, per word
    const int32_t* off;           // [states] where the state's transitions start in nxt
    const int32_t* nxt;           // next states, ordered by (state, token)
    const int32_t* gslot;         // [nslots, 4] {state, g_len, miss state, guided}
    int words, n_states, n_trans; // row width in words (a multiple of 4, words * 32 >= V); arena sizes (the walk clamps to them)
};
struct LpArgsG : LpArgsC { LpGuide g; };
int process_logits(const LpArgsG& a, int T, hipStream_t st);
int guide_build(uint32_t* allow, int32_t* rank, int32_t* off, int32_t* nxt, int words, int row_stride, int V, int state_base,
                int trans_base, int n_states, const int32_t* row_ptr, const int32_t* tokens, const int32_t* next, int n_trans,
                hipStream_t st);
int guide_catch_up(int B, int V, int32_t* gslot, const LpGuide& g, const int64_t* gen_tokens, int gen_cap,
                   const int32_t* gen_lens, hipStream_t st);
int token_constraints_set(uint32_t* deny, int deny_words, int32_t* meta, int32_t* bias_ids, float* bias_vals, int32_t* words,
                          int32_t* word_lens, int V, int slot, const int64_t* allowed, int n_allowed, const int64_t* banned,
                          int n_banned, const int32_t* src_bias_ids, const float* src_bias_vals, int n_bias,
                          const int32_t* src_words, const int32_t* src_word_lens, int n_words, int bad_words_present,
                          hipStream_t st);
int typical_acceptance_sample(const float* target_probs, const int64_t* draft_ids, const int64_t* bonus_ids,
                              float posterior_threshold, float posterior_alpha, int B, int k, int V, int64_t di_sb,
                              int64_t di_sk, int64_t bonus_stride, int64_t* out_tokens, uint8_t* accepted, int64_t* recovered,
                              int64_t* counters, const int32_t* active_lens, void* ws, hipStream_t st);
int advance_step(int n, int block_size, int64_t* input_tokens, const int64_t* sampled, int64_t* positions,
                 int32_t* seq_lens, int64_t* slot_mapping, const int32_t* block_tables, int64_t bt_stride,
                 hipStream_t st);
int spec_advance_draft(int n, int block_size, int max_blocks, int64_t* input_tokens, const int64_t* sampled,
                       int64_t* positions, int32_t* ctx_lens, int64_t* slot_mapping, const int32_t* block_tables,
                       int64_t bt_stride, hipStream_t st);
int spec_prepare_draft_embed(int B, int block_size, int max_blocks, const int64_t* last_token, const int32_t* seq_lens,
                             const int32_t* step_mask, int32_t* eff_lens, const int32_t* block_tables, int64_t bt_stride,
                             int64_t* input_tokens, int64_t* positions, int64_t* slot_mapping, int32_t* ctx_lens, const f16* table,
                             f16* hidden_out, int H, int V, hipStream_t st);
int spec_advance_draft_embed(int n, int block_size, int max_blocks, int64_t* input_tokens, const int64_t* sampled, int64_t* positions,
                             int32_t* ctx_lens, int64_t* slot_mapping, const int32_t* block_tables, int64_t bt_stride, const f16* table,
                             f16* hidden_out, int H, int V, hipStream_t st);
int spec_prepare_verify_embed(int B, int k, int block_size, int max_blocks, const int64_t* last_token, const int64_t* draft_ids,
                              int64_t di_sb, int64_t di_sk, const int32_t* seq_lens, const int32_t* block_tables, int64_t bt_stride,
                              int64_t* v_tokens, int64_t* v_positions, int64_t* v_slots, int32_t* v_ctx_lens, const f16* table,
                              f16* hidden_out, int H, int V, hipStream_t st);
int spec_prepare_draft(int B, int block_size, int max_blocks, const int64_t* last_token, const int32_t* seq_lens,
                       const int32_t* block_tables, int64_t bt_stride, int64_t* input_tokens, int64_t* positions,
                       int64_t* slot_mapping, int32_t* ctx_lens, hipStream_t st);
int spec_prepare_verify(int B, int k, int block_size, int max_blocks, const int64_t* last_token, const int64_t* draft_ids,
                        int64_t di_sb, int64_t di_sk, const int32_t* seq_lens, const int32_t* block_tables, int64_t bt_stride, int64_t* v_tokens,
                        int64_t* v_positions, int64_t* v_slots, int32_t* v_ctx_lens, hipStream_t st);
int spec_snapshot(int B, int restore, int32_t* seq_lens, int32_t* gen_lens, int64_t* last_token, int64_t* counters,
                  int64_t* rng_state, int32_t* snap_i32, int64_t* snap_i64, hipStream_t st);
int collect_error_words(int32_t* w0, int32_t* w1, int32_t* w2, int32_t* w3, int clear, int64_t* out, hipStream_t st);
int spec_commit(int B, int k, const int64_t* out_tokens, int32_t* seq_lens, int64_t* last_token, int64_t* gen_tokens,
                int32_t* gen_lens, int gen_cap, hipStream_t st);

// logprobs.hip: the selected token's logprob and rank + the num_top best of every row, from the processed probabilities
// (fp32) or from raw logits (fp16); one launch, no workspace
int token_logprobs_from_probs(const float* probs, int64_t row_stride, const int64_t* token_ids, int rows, int vocab, int num_top,
                              float* token_logprob, int32_t* token_rank, int32_t* top_ids, float* top_logprobs, hipStream_t st);
int token_logprobs_from_logits(const f16* logits, int64_t row_stride, const int64_t* token_ids, int rows, int vocab, int num_top,
                               float* token_logprob, int32_t* token_rank, int32_t* top_ids, float* top_logprobs, hipStream_t st);

// cache_ops.hip: whole KV-cache blocks moved as opaque runs of block_bytes bytes (% 16 == 0) across the 2 * num_layers cache
// tensors whose base pointers the device array layer_ptrs holds; one launch each, no workspace
int copy_blocks(void* const* layer_ptrs, int num_layers, const int64_t* pairs, int num_pairs, int64_t block_bytes, hipStream_t st);
int gather_blocks(void* const* layer_ptrs, int num_layers, const int64_t* block_ids, int n, int64_t block_bytes, void* staging,
                  hipStream_t st);
int scatter_blocks(void* const* layer_ptrs, int num_layers, const int64_t* block_ids, int n, int64_t block_bytes,
                   const void* staging, hipStream_t st);
}  // namespace qspec
