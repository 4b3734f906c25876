// What the three streaming-GEMM translation units share (gemm_stream_w4a4.hip: the draft pass's W4A4 kernels,
// gemm_stream_w4a16.hip: the verify pass's W4A16 kernels, gemm_stream_f16.hip: the lm_head): the launch argument block, the
// epilogue / prologue form enums, the tile -> weight-row maps, the fused epilogue tail (RoPE + KV-cache store, silu(gate) * up)
// and the host-side pieces every launcher repeats (grid sizing, dynamic-LDS opt-in, argument fills).
#pragma once
#include <stdlib.h>

#include "common.cuh"
#include "kernels.h"

namespace qspec {

// Weight loads.  Non-temporal loads (`global_load_dwordx4 ... nt`, -DQS_NT_WEIGHTS) were measured on the register
// refill ring of these kernels and lost: cycle 8.66 -> 8.90 ms, gate_up 15.6 -> 16.1 us, down 8.4 -> 8.8 us (round 2;
// the guide's gain is for LDS-DMA loader rings).  Default cache policy it is.
template <typename T>
__device__ __forceinline__ T wload(const void* p) {
#ifdef QS_NT_WEIGHTS
    return __builtin_nontemporal_load(reinterpret_cast<const T*>(p));
#else
    return *reinterpret_cast<const T*>(p);
#endif
}

enum { SEPI_PLAIN = 0, SEPI_QKV = 1, SEPI_GATEUP = 2, SEPI_RESID = 3, SEPI_PARTIAL = 4, SEPI_IPART = 5 };   // RESID: plain + fp16 residual add
// SEPI_IPART (W4A4, (xq, xs) input): blockIdx.y picks one of gridDim.y K slices of length K; the raw int32 sums of the slice
// go to ipart[blockIdx.y][M][N] and whoever consumes them (norm_quant.hip: ln_kernel with ipart) adds the slices -- exact in
// any order -- and applies the epilogue expression.  What it is for: at 17..32 tokens a workgroup with ONE 16-row tile reads
// 2 x as many activation bytes as weight bytes (config 3's down_proj: 229 KB for 115 KB); with two K slices it takes TWO
// tiles of half the K and reads its activation fragments once for both.
enum { PRO_Q = 0, PRO_LN = 1, PRO_LNH = 2, PRO_LN1 = 3, PRO_LNS = 4, PRO_LN1S = 5, PRO_RQ = 6 };   // (see the header)

struct StreamArgs {
    const int8_t* xq;       // PRO_Q : [M, K/2] packed int4 activations
    const f16* xs;          // PRO_Q : [M] activation scales
    const f16* hidden_in;   // PRO_LN: [M, K] residual stream
    const f16* delta;       // PRO_LN: [M, K] output of the previous projection (added first) or nullptr
    f16* hidden_out;        // PRO_LN: [M, K] updated residual stream (written by workgroup 0) or nullptr
    float eps;
    int* sync;              // PRO_LNH: hand-off workspace (gemm_w4a4_stream_sync_bytes(), zero-filled once)
    const f16* x16;         // PRO_RQ: [M, K] fp16 rows
    const float* part_amax; // PRO_RQ: [M, 8] partial maxima of |x16| per row
    float clip;             // PRO_RQ: the quantiser's clip ratio
    const f16* resid_in;    // SEPI_RESID: [M, N] residual stream; resid_out = h(f(resid_in) + f(h(gemm)))
    f16* resid_out;         // SEPI_RESID: [M, N] (may alias resid_in: each element is read and written by one thread)
    const f16* x;           // W4A16: [M, K] fp16 activations, row stride ldx halves
    int64_t ldx, ldw;       // W4A16: activation row stride (halves) / packed weight row stride (bytes); 0 = dense
    int tile0;              // W4A16: first tile of the launch (column-parallel shards)
    float* part;            // W4A16 SEPI_PARTIAL: [gridDim.y][M][N] raw fp32 sums of K slice blockIdx.y (K = slice length)
    int xperm;              // W4A16: x is the 16-row activation tile in fragment-major layout (w4a16_xperm_offset)
    int* ipart;             // W4A4 SEPI_IPART: [gridDim.y][M][N] raw int32 sums of K slice blockIdx.y (ldx / ldw = row strides in BYTES)
    const uint8_t* wq;      // [N, K/2]
    const f16* ws;          // [N]
    f16* out;
    int M, N, K, ntiles;
    const int64_t* positions;
    const f16* cos_sin_cache;
    f16* key_cache;
    f16* value_cache;
    const int64_t* slot_mapping;
    int nq, nkv, I;
    int hdl = 7;   // SEPI_QKV: log2(head size), 7 or 6
    int kv8 = 0;   // SEPI_QKV: the caches hold e4m3 bytes (the `_kv8` entries); k_inv / v_inv = 1.0f / scale
    float k_inv = 1.0f, v_inv = 1.0f;
};

// The cache store of the SEPI_QKV epilogues: the fp16 value, or its e4m3 byte at the same element position (uniform branch:
// one launch form for both cache types; reshape_and_cache_flash(..., "fp8", k_scale, v_scale)).
__device__ __forceinline__ void kv_cache_store(const StreamArgs& a, bool is_k, int64_t idx, f16 res) {
    f16* cache = is_k ? a.key_cache : a.value_cache;
    if (a.kv8) reinterpret_cast<uint8_t*>(cache)[idx] = f2e4m3(h2f(res) * (is_k ? a.k_inv : a.v_inv));
    else cache[idx] = res;
}

__device__ __forceinline__ i32x4 widen16(u32 p0, u32 p1) {
    return i32x4{(int)((p0 << 4) & 0xF0F0F0F0u), (int)(p0 & 0xF0F0F0F0u), (int)((p1 << 4) & 0xF0F0F0F0u),
                 (int)(p1 & 0xF0F0F0F0u)};
}

// Byte offset (inside one batch of NW*UB*64 bytes of a weight row) of step u of `wave`.  Steps are paired so that a
// wave's two consecutive loads cover one 128-byte line of every row (a 16x16 MFMA tile puts only 4 lanes = 64 bytes
// on a row per load instruction); an odd UB leaves one unpaired step at the end of the batch.
template <int NW, int UB>
__device__ __forceinline__ int step_off(int wave, int u) {
    constexpr int UE = UB & ~1;
    if (u < UE) return (u >> 1) * (2 * NW * 64) + wave * 128 + (u & 1) * 64;
    return UE * NW * 64 + wave * 64;
}

// SEPI_QKV tiles.  A tile is eight RoPE pairs (i, i + 64) of one head: rows 0..7 = the pairs' first halves, 8..15 = their
// second halves.  Classic: tile t = pairs 8 (t & 7) .. + 7 of head t >> 3.  LEVELLED (I = L > 0, used where N / 16 tiles
// are 1.5 per workgroup, e.g. Llama-3-8B's 384 on 256 CUs: half the workgroups streamed two tiles, half one): the
// (heads * 64) pairs are dealt twelve to a workgroup (measured slower, off by default: see qkv_level_workgroups) -- "tile" v < L = pairs 12 v .. 12 v + 7 (a full tile), "tile" L + v =
// pairs 12 v + 8 .. 12 v + 11 (a HALF tile: slots j >= 4 repeat slots j - 4, their results are never stored; the wave
// loads coalesce the repeated rows) -- so every workgroup streams 48 KB instead of 64 or 32.
struct QkvPair {
    int head, i;
    bool valid;
};
// hdl = log2(head size): 7 (128: 64 pairs = 8 tiles per head) or 6 (64, e.g. TinyLlama: 32 pairs = 4 tiles per head)
__device__ __forceinline__ QkvPair qkv_pair(int tb, int j, int L, int hdl) {   // j = 0..7: pair slot of the tile
    if (L == 0) return QkvPair{tb >> (hdl - 4), (tb & ((1 << (hdl - 4)) - 1)) * 8 + j, true};
    const bool half = tb >= L;
    const int p = 12 * (half ? tb - L : tb) + (half ? 8 + (j & 3) : j);
    return QkvPair{p >> 6, p & 63, !half || j < 4};
}
template <int EPI>
__device__ __forceinline__ int stile_row(int tb, int r, int I, int hdl) {
    if (EPI == SEPI_QKV) {
        const QkvPair q = qkv_pair(tb, r & 7, I, hdl);
        return (q.head << hdl) + ((r >> 3) << (hdl - 1)) + q.i;
    }
    if (EPI == SEPI_GATEUP) return (r >> 3) * I + tb * 8 + (r & 7);
    return tb * 16 + r;
}

// global_load_lds_dwordx4: 16 bytes per lane from memory straight into LDS (lane-linear image at lds_dst); nt = non-temporal.
template <int NT>
__device__ __forceinline__ void glds16(const void* gsrc, u32 lds_dst) {
    u32 keep;
    if (NT)
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off nt\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
    else
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
template <int N>
__device__ __forceinline__ void vmcnt_le() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// ---- the fused epilogue tail of the SEPI_QKV / SEPI_GATEUP forms, one copy for every streaming kernel.
// cos / sin of (position pos_m, tile column c) of `tile`: prefetched together with the tile's weights
__device__ __forceinline__ void stream_pre_qkv(const StreamArgs& a, int tile, int c, int64_t pos_m, f16& cf, f16& sf) {
    const int o = qkv_pair(tile, c & 7, a.I, a.hdl).i;
    const f16* cs = a.cos_sin_cache + (pos_m << a.hdl);   // rot_dim = head size
    cf = cs[o];
    sf = cs[(1 << (a.hdl - 1)) + o];
}
// Everything behind the exchange of hv with the thread 8 columns away (partner): epilogue thread (token m, tile column c).
// SEPI_GATEUP: columns 0..7 hold up, 8..15 gate.  SEPI_QKV: columns (c, c + 8) are one RoPE pair; rotate, store, and write
// the K / V heads into the paged cache.  cf / sf are read by SEPI_QKV only (references: other forms leave them unset).
// HALF_TILES = false: the caller never sees the levelled tiling's half tiles (qkv_pair: valid is always true), no test.
template <int EPI, bool HALF_TILES = true>
__device__ __forceinline__ void stream_epilogue_pair(const StreamArgs& a, int tile, int m, int c, f16 hv, f16 partner,
                                                     const f16& cf, const f16& sf, int64_t slot_m) {
    static_assert(EPI == SEPI_GATEUP || EPI == SEPI_QKV, "the paired epilogues");
    if (EPI == SEPI_GATEUP) {
        if (c < 8) {  // hv = up, partner = gate
            const float gt = h2f(partner);
            const float act = h2f(f2h(gt / (1.0f + qexpf(-gt))));
            a.out[(size_t)m * a.I + tile * 8 + c] = f2h(act * h2f(hv));
        }
        return;
    }
    const QkvPair qp = qkv_pair(tile, c & 7, a.I, a.hdl);
    if (HALF_TILES && !qp.valid) return;   // a half tile's repeated slots
    const int head = qp.head, o = qp.i;
    const int n = (head << a.hdl) + ((c >> 3) << (a.hdl - 1)) + o;
    f16 res = hv;
    if (head < a.nq + a.nkv) {
        const float cff = h2f(cf), sff = h2f(sf);
        const float xf = h2f(c < 8 ? hv : partner), yf = h2f(c < 8 ? partner : hv);
        res = c < 8 ? f2h(h2f(f2h(xf * cff)) - h2f(f2h(yf * sff))) : f2h(h2f(f2h(yf * cff)) + h2f(f2h(xf * sff)));
    }
    a.out[(size_t)m * a.N + n] = res;
    if (head >= a.nq && slot_m >= 0) {
        const bool is_k = head < a.nq + a.nkv;
        const int kvh = is_k ? head - a.nq : head - a.nq - a.nkv;
        kv_cache_store(a, is_k, ((slot_m * a.nkv + kvh) << a.hdl) + ((c >> 3) << (a.hdl - 1)) + o, res);
    }
}

// ---- host side
// workgroups per launch above which a workgroup loops over several tiles
inline int stream_cap() {
    static const int v = QS_DEV_KNOB("QSPEC_STREAM_CAP", 256);   // one workgroup per CU measured best (bench_stream.py)
    return v < 1 ? 256 : v;
}
// Workgroups for ntiles tiles under a cap: every workgroup gets ceil(ntiles / cap) tiles (the last one maybe fewer), and no
// more workgroups are launched than that needs.
inline int stream_grid(int ntiles, int cap) {
    if (ntiles <= cap) return ntiles;
    const int per = (ntiles + cap - 1) / cap;
    return (ntiles + per - 1) / per;
}
// (the opt-in to more than 64 KiB of dynamic LDS: common.cuh, lds_optin)

// The argument block of an entry function: weights and shape, then the activations, then the QKV epilogue's operands.
inline StreamArgs stream_args(const int8_t* wq, const f16* ws, int M, int N, int K) {
    StreamArgs a{};
    a.wq = reinterpret_cast<const uint8_t*>(wq); a.ws = ws; a.M = M; a.N = N; a.K = K; a.ntiles = N / 16;
    return a;
}
inline StreamArgs with_acts(StreamArgs a, const StreamActs& x) {
    a.xq = x.xq; a.xs = x.xs; a.hidden_in = x.hidden_in; a.delta = x.delta; a.hidden_out = x.hidden_out; a.eps = x.eps; a.sync = x.sync;
    return a;
}
inline StreamArgs with_qkv(StreamArgs a, const int64_t* positions, const f16* cos_sin_cache, f16* key_cache, f16* value_cache,
                           const int64_t* slot_mapping, int nq, int nkv, int d, KvQuant kq) {
    a.kv8 = kq.fp8; a.k_inv = kq.k_inv; a.v_inv = kq.v_inv;
    a.hdl = d == 64 ? 6 : 7;
    a.positions = positions; a.cos_sin_cache = cos_sin_cache; a.key_cache = key_cache; a.value_cache = value_cache;
    a.slot_mapping = slot_mapping; a.nq = nq; a.nkv = nkv;
    return a;
}

// Levelled QKV tiling (qkv_pair): L = workgroups = pairs / 12, or 0 for the classic 16-row tiles.  Only where the classic
// tiling is uneven (more tiles than workgroups, not a multiple of them) and the pairs divide by twelve: Llama-3-8B's
// (32 + 8 + 8) heads x 64 pairs = 3072 = 12 x 256.  OFF by default (QSPEC_QKV_LEVEL=1 switches it on): measured in round 3,
// bit-identical, but the draft qkv launch takes 7.25-7.38 us against 6.89 and the cycle 7.58-7.65 ms against 7.51-7.54 -- two
// tile iterations (reduction, barriers, epilogue) in EVERY workgroup cost more than the 16 KB less that the slowest ones stream.
#ifdef QS_EXPERIMENTAL
inline int qkv_level_workgroups(int nq, int nkv, int N) {
    static const int on = QS_DEV_KNOB("QSPEC_QKV_LEVEL", 0);
    const int pairs = (nq + 2 * nkv) * 64, cap = stream_cap(), classic = N / 16;
    if (!on || pairs % 12 || classic <= cap || classic % cap == 0 || pairs / 12 > cap) return 0;
    return pairs / 12;
}
#endif

}  // namespace qspec
