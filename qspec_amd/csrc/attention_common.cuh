// Paged attention: what the kernel files (attention_decode.hip, attention_prefill.hip, attention_generic.hip), the host
// plan (attention.hip) and the consumers of the partials (hadamard.hip) share -- tile constants, the transposing LDS
// reads, the host-side argument block, launch plan and workspace layout.
#pragma once
#include "common.cuh"
#include "kernels.h"

namespace qspec {

#define QS_ATT_MAXR 16
#define QS_ATT_CHUNK 128
#define QS_ATT_CNT_SLOTS 4096  // ints reserved at the head of the workspace for the ticket counters
#define QS_ATT_VSTRIDE 144     // halves per V row in LDS (288 B): 4 rows x 4 column quads hit 16 distinct bank pairs
#define QS_ATT_MAXSPLIT 64
#define QS_AW_KEYS 32         // keys of a wave's slice (attention_decode.hip: paged_attention_waves_kernel)
#define QS_FA_ROWS 64         // rows / keys of a workgroup's tile (attention_prefill.hip)
#define QS_FA_KEYS 64

// ds_read_b64_tr_b16 as a compiler builtin: the register allocator places the two halves of a B fragment next to each
// other (no v_mov pairs) and the waits are the compiler's (per use, not lgkmcnt(0) behind every read, as the inline-asm
// form of rounds 1-2 had it).
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ s16x4 lds_tr16(uint32_t lds_byte_addr) {
    return __builtin_amdgcn_ds_read_tr16_b64_v4i16(reinterpret_cast<__attribute__((address_space(3))) s16x4*>(lds_byte_addr));
}

// Eight d tiles of one 32-key step at once (the prompt kernel): 16 transposing reads from one base address with
// immediate offsets (d tile: +32 B, second key quad: +4 V rows), ONE wait behind all of them.
__device__ __forceinline__ void lds_read_tr_b16_x16(uint32_t a, u32x2 (&lo)[8], u32x2 (&hi)[8]) {
    static_assert(QS_ATT_VSTRIDE * 8 == 1152, "immediate offsets below assume 288-byte V rows");
    asm volatile(
        "ds_read_b64_tr_b16 %0, %16 offset:0\n\tds_read_b64_tr_b16 %8, %16 offset:1152\n\t"
        "ds_read_b64_tr_b16 %1, %16 offset:32\n\tds_read_b64_tr_b16 %9, %16 offset:1184\n\t"
        "ds_read_b64_tr_b16 %2, %16 offset:64\n\tds_read_b64_tr_b16 %10, %16 offset:1216\n\t"
        "ds_read_b64_tr_b16 %3, %16 offset:96\n\tds_read_b64_tr_b16 %11, %16 offset:1248\n\t"
        "ds_read_b64_tr_b16 %4, %16 offset:128\n\tds_read_b64_tr_b16 %12, %16 offset:1280\n\t"
        "ds_read_b64_tr_b16 %5, %16 offset:160\n\tds_read_b64_tr_b16 %13, %16 offset:1312\n\t"
        "ds_read_b64_tr_b16 %6, %16 offset:192\n\tds_read_b64_tr_b16 %14, %16 offset:1344\n\t"
        "ds_read_b64_tr_b16 %7, %16 offset:224\n\tds_read_b64_tr_b16 %15, %16 offset:1376\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&v"(lo[0]), "=&v"(lo[1]), "=&v"(lo[2]), "=&v"(lo[3]), "=&v"(lo[4]), "=&v"(lo[5]), "=&v"(lo[6]), "=&v"(lo[7]),
          "=&v"(hi[0]), "=&v"(hi[1]), "=&v"(hi[2]), "=&v"(hi[3]), "=&v"(hi[4]), "=&v"(hi[5]), "=&v"(hi[6]), "=&v"(hi[7])
        : "v"(a)
        : "memory");
}

// ---------------------------------------------------------------- shared device pieces (head size 128 kernels)
// Per-sequence metadata through the VECTOR memory path: a uniform address would become an s_load, and a scalar
// cache miss on data the previous kernel has just written costs microseconds, not hundreds of cycles.
struct SeqMeta { int qs, qlen, ctx; };   // first query token, query tokens, context length (the query tokens included)
__device__ __forceinline__ SeqMeta seq_meta(const int32_t* q_start, const int32_t* ctx_lens, int seq, int lane) {
    int meta = 0;
    if (lane < 3) meta = lane < 2 ? q_start[seq + lane] : ctx_lens[seq];
    const int qs = __shfl(meta, 0, 64);
    return SeqMeta{qs, __shfl(meta, 1, 64) - qs, __shfl(meta, 2, 64)};
}

// A sequence's block-table row (<= 128 entries) in two registers per lane: the lookups become lane permutes, or -- for a
// wave-uniform index -- v_readlane + SALU.  Indices are already clamped to the table.
struct BtRow {
    int v0, v1;
    __device__ __forceinline__ int get(int bi) const {
        const int a = __shfl(v0, bi & 63, 64), b = __shfl(v1, bi & 63, 64);
        return bi < 64 ? a : b;
    }
    __device__ __forceinline__ int get_uniform(int bi) const {   // bi in an SGPR
        const int a = __builtin_amdgcn_readlane(v0, bi & 63), b = __builtin_amdgcn_readlane(v1, bi & 63);
        return bi < 64 ? a : b;
    }
};
__device__ __forceinline__ BtRow bt_row_load(const int32_t* block_tables, int seq, int max_blocks, int lane) {
    const int32_t* btr = block_tables + (size_t)seq * max_blocks;
    return BtRow{btr[min(lane, max_blocks - 1)], btr[min(lane + 64, max_blocks - 1)]};
}

// Keys of context split `split`: ceil(ctx / n_splits) rounded up to a 16-key tile, so that a short context still spreads
// over all n_splits workgroups (each CU only draws ~25 GB/s).
struct SplitKeys { int kps, k_begin, k_end; };
__device__ __forceinline__ SplitKeys split_keys(int ctx, int n_splits, int split) {
    const int kps = (((ctx + n_splits - 1) / n_splits) + 15) & ~15;
    const int k_begin = split * kps;
    return SplitKeys{kps, k_begin, min(ctx, k_begin + kps)};
}

// Row rr of a kv head's (query token x GQA head) rows -> token * nq + head, the index of its output / partial row
__device__ __forceinline__ size_t token_head(int rr, int qs, int group_log2, int kvh, int gmask, int nq) {
    return (size_t)(qs + (rr >> group_log2)) * nq + (kvh << group_log2) + (rr & gmask);
}

// Q fragment of lane (row, d slice 8 g4 + 32 j) for the 16x16x32 MFMA: four 16-byte loads.  `r` is already clamped to a
// valid row by the caller.
__device__ __forceinline__ void load_q_frag(u32x4 (&qfrag)[4], const f16* q, int64_t q_stride, int r, int qs,
                                            int group_log2, int kvh, int gmask, int g4) {
    const int tok = qs + (r >> group_log2), head = (kvh << group_log2) + (r & gmask);
    const f16* qp = q + (size_t)tok * q_stride + (size_t)head * 128 + g4 * 8;
#pragma unroll
    for (int j = 0; j < 4; j++) qfrag[j] = *reinterpret_cast<const u32x4*>(qp + 32 * j);
}

// Online softmax of a wave's NT 16-key score tiles in registers: the 16 lanes of a g4 group hold the NT * 16 keys of rows
// 4 g4 + reg.  Folds the tiles into the running (max, sum), leaves the rescale factor of the running output in alpha and
// P in the wave's LDS tile pl ([hi | lo][16 rows][PSTR]) as hi + lo fp16, so that P.V keeps fp32-class accuracy for two
// MFMAs instead of one.  Order: max over the tiles, then lanes ^ 8, 4, 2, 1; the sum over the tiles ascending, then 8, 4, 2, 1.
template <int NT, int PSTR>
__device__ __forceinline__ void online_softmax_tiles(const f32x4 (&sacc)[NT], float (&row_m)[4], float (&row_l)[4],
                                                     float (&alpha)[4], f16* pl, int c16, int g4) {
    static_assert(NT == 2 || NT == 4, "two or four key tiles");
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        float mx = fmaxf(sacc[0][reg], sacc[1][reg]);
        if constexpr (NT == 4) mx = fmaxf(mx, fmaxf(sacc[2][reg], sacc[3][reg]));
        mx = fmaxf(mx, dpp_xor<8>(mx));
        mx = fmaxf(mx, dpp_xor<4>(mx));
        mx = fmaxf(mx, dpp_xor<2>(mx));
        mx = fmaxf(mx, dpp_xor<1>(mx));
        const float m_old = row_m[reg], m_new = fmaxf(m_old, mx);
        float sum = 0.0f;
#pragma unroll
        for (int t = 0; t < NT; t++) {
            const float pv = m_new == -__builtin_inff() ? 0.0f : aexp(sacc[t][reg] - m_new);
            const f16 ph = f2h(pv);
            pl[(4 * g4 + reg) * PSTR + t * 16 + c16] = ph;
            pl[(16 + 4 * g4 + reg) * PSTR + t * 16 + c16] = f2h(pv - h2f(ph));
            sum += pv;
        }
        sum += dpp_xor<8>(sum);
        sum += dpp_xor<4>(sum);
        sum += dpp_xor<2>(sum);
        sum += dpp_xor<1>(sum);
        alpha[reg] = m_old == -__builtin_inff() ? 0.0f : aexp(m_old - m_new);
        row_m[reg] = m_new;
        row_l[reg] = __builtin_fmaf(row_l[reg], alpha[reg], sum);
    }
}

// Weight of a partial with row maximum m in a merge under the overall maximum M: e^(m - M), 0 for an empty partial
// (m = -inf, also when M = -inf).  Every split merge -- in the chunk kernel, the waves combine, the generic merge kernel and
// the head-transform kernels of hadamard.hip -- uses this one expression, so their fp16 rows agree bit for bit.
__device__ __forceinline__ float merge_weight(float m, float M) { return m == -__builtin_inff() ? 0.0f : aexp(m - M); }

// ---------------------------------------------------------------- host side
// The argument block paged_attention() fills once; every launcher takes it.  key / value cache: fp16, or e4m3 bytes (fp8);
// sm_scale carries k_scale already (fp8), v_scale multiplies a row's output where it is stored (1 for fp16);
// out == nullptr: leave the per-split partials (o, m, l) in the workspace for heads_hadamard_merge.
struct AttnArgs {
    const f16* q; int64_t q_stride;
    const void *key_cache, *value_cache;
    const int32_t* block_tables; int max_blocks;
    const int32_t *ctx_lens, *q_start;
    int n_seqs, max_q_len, nq, nkv, d, block_size;
    float sm_scale; int n_splits;
    float* ws; f16* out;
    float v_scale; bool fp8;
    hipStream_t st;
};
// The launch plan attn_form() (attention.hip) decides from the arguments alone.
enum AttnFamily { ATTN_NO_LAUNCH, ATTN_GENERIC, ATTN_GENERIC_VEC, ATTN_PREFILL, ATTN_WAVES, ATTN_CHUNK, ATTN_PREFILL_SPLIT };
struct AttnForm {
    AttnFamily family;
    int rc;                   // ATTN_NO_LAUNCH: what paged_attention() returns (0: nothing to do, < 0: the refusal)
    bool pf, bt, fast;        // template choices of the chunk (PF, BT) and waves (BT, FAST) kernels
    int nw;                   // waves per workgroup of the waves kernel
    int S;                    // context splits of the launch (generic head sizes: paged_attention_generic_splits)
    bool partials, merge;     // (o, m, l) of every split go to the workspace / the splits are merged into `out`: inside the
                              // chunk kernel, by a second launch for the generic head sizes and the context-split prompt kernel
    int bs_log2, group_log2, n_rb;   // n_rb: row blocks per kv head
    dim3 grid; size_t lds;
};
int attn_launch_chunk(const AttnArgs& a, const AttnForm& f);     // attention_decode.hip
int attn_launch_waves(const AttnArgs& a, const AttnForm& f);
int attn_launch_prefill(const AttnArgs& a, const AttnForm& f);   // attention_prefill.hip (ATTN_PREFILL, ATTN_PREFILL_SPLIT)
int attn_launch_generic(const AttnArgs& a, const AttnForm& f);   // attention_generic.hip

// Workspace: [QS_ATT_CNT_SLOTS ticket counters (int) | o partials [Tmax, nq, S, d] | (m, l) partials [Tmax, nq, S, 2]], sized by
// the host for Tmax = n_seqs * max_q_len tokens (paged_attention_ws_bytes).  It must be zero-filled once before its first
// use; every call leaves the counters zero again.  (The readers in hadamard.hip hold it const.)
struct AttnWs { int* cnt; float *o, *ml; };
inline AttnWs attn_ws(const float* ws, size_t Tmax, int nq, int d, int S) {
    float* o = const_cast<float*>(ws) + QS_ATT_CNT_SLOTS;
    return AttnWs{reinterpret_cast<int*>(const_cast<float*>(ws)), o, o + Tmax * nq * S * d};
}
void attn_launch_split_merge(const AttnArgs& a, const AttnForm& f, const AttnWs& w);   // attention_generic.hip: partials -> a.out
// One launch of the plan: the eight arguments every attention kernel starts with, then its own.  LDS beyond 64 KiB is
// opted in to where the plan asks for it.
template <auto KERN, typename KVT, typename... Own>
static int attn_launch(int threads, const AttnArgs& a, const AttnForm& f, Own... own) {
    if (const int rc = lds_optin<KERN>(f.lds)) return rc;
    hipLaunchKernelGGL(KERN, f.grid, dim3(threads), f.lds, a.st, a.q, a.q_stride, (const KVT*)a.key_cache, (const KVT*)a.value_cache,
                       a.block_tables, a.max_blocks, a.ctx_lens, a.q_start, own...);
    return 0;
}

}  // namespace qspec
