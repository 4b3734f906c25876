// Paged causal attention for prompt-sized queries (head size 128), with its launcher.
//
// Replaces (reference, relative to /root/reference):
//   flash_attn_varlen_func (vllm_flash_attn wheel, un-vendored; call sites
//                                        vllm/attention/backends/flash_attn.py:741-830)
#include "attention_common.cuh"

namespace qspec {

// ---------------------------------------------------------------- prompt-sized queries (flash-attn varlen, head 128)
// paged_attention_kernel (attention_decode.hip) keeps 16 rows per workgroup: right for decode (1 .. k+1 query tokens per
// sequence), but a prompt pass would stream K/V once per 4 query tokens.  Here a workgroup holds 64 rows (16 query tokens x the GQA group of one kv
// head), 16 per wave, and walks the visible keys in 64-key chunks (FlashAttention-2 form):
//   * the chunk's K and V go through LDS once per workgroup (K rows XOR-swizzled in 16-byte pieces for the fragment
//     reads, V rows padded for the transposing reads); the next chunk's rows are in flight in registers meanwhile;
//   * a wave's S = Q K^T (16 x 64), its running (max, sum) and its 16 x 128 output live in registers; only P goes
//     through a wave-private LDS tile to change from the accumulator layout to the A-operand layout (as hi + lo fp16,
//     two MFMAs, so that P.V keeps fp32-class accuracy);
//   * SPLIT = false: no context split: one (o, m, l) per row, stored as the single-split partial heads_hadamard_merge
//     expects and/or normalised into `out`.
//   * SPLIT = true (a short suffix behind a long cached context: too few row blocks to fill the chip): grid.z context splits.
//     Split z of a sequence owns the keys [z L, min((z + 1) L, ctx)), L = ceil(ctx / S) rounded up to a whole 64-key chunk, from
//     ctx alone; its walk is the same chunk walk offset by z L and clipped by the workgroup's causal horizon.  It stores the
//     partial (o, m, l) of (token, head, split) in the layout of the chunk kernel and never writes `out`: the merge is a
//     launch of its own (attn_launch_split_merge) or the head transform's.  A row whose position lies in front of the split
//     sees no key at all: its running maximum stays -inf through every chunk.  online_softmax_tiles takes exactly that
//     case (m_new = -inf: p = 0; m_old = -inf: alpha = 0, never e^(-inf + inf)), so such a row ends with the neutral partial
//     (0, -inf, 0) an empty split of the chunk kernel stores; a workgroup whose whole range lies behind its horizon walks
//     no chunk and stores the same.
template <typename KVT, bool SPLIT>   // KVT: see paged_attention_kernel
__global__ __launch_bounds__(256) void paged_attention_prefill_kernel(
    const f16* __restrict__ q, int64_t q_stride, const KVT* __restrict__ key_cache, const KVT* __restrict__ value_cache,
    const int32_t* __restrict__ block_tables, int max_blocks, const int32_t* __restrict__ ctx_lens,
    const int32_t* __restrict__ q_start, int nq, int nkv, int bs_log2, int group_log2, float sm_scale, int n_rb,
    float* __restrict__ ws_o, float* __restrict__ ws_ml, f16* __restrict__ out, float v_scale) {
    constexpr int D = 128;
    constexpr bool FP8 = sizeof(KVT) == 1;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    unsigned char* kl = reinterpret_cast<unsigned char*>(smem_raw);                       // [64 keys][256 B], swizzled
    f16* vl = reinterpret_cast<f16*>(kl + QS_FA_KEYS * 256);                               // [64 keys][QS_ATT_VSTRIDE]
    f16* pl_all = vl + QS_FA_KEYS * QS_ATT_VSTRIDE;                                        // [4 waves][hi, lo][16][72]
    constexpr int PSTR = 72;   // halves per P row (144 B): the 16 rows of an A-fragment read fall on distinct banks
    // the last row blocks see the most keys (causal): dispatch them first so that the tail of the launch is short blocks
    const int seq = blockIdx.x, rb = n_rb - 1 - blockIdx.y / nkv, kvh = blockIdx.y % nkv;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c16 = lane & 15, g4 = lane >> 4;
    const int gmask = (1 << group_log2) - 1, bmask = (1 << bs_log2) - 1;
    const SeqMeta sm = seq_meta(q_start, ctx_lens, seq, lane);
    const int qs = sm.qs, qlen = sm.qlen, ctx = sm.ctx;
    const int total_rows = qlen << group_log2;
    if (rb * QS_FA_ROWS >= total_rows) return;   // uniform
    const int rbase = rb * QS_FA_ROWS + wave * 16;
    f16* pl = pl_all + wave * 2 * 16 * PSTR;
    const int32_t* bt = block_tables + (size_t)seq * max_blocks;

    // causal horizon of the workgroup: the last valid row's token sees keys 0 .. pos
    const int last_row = min(rb * QS_FA_ROWS + QS_FA_ROWS - 1, total_rows - 1);
    const int n_keys = min(ctx, ctx - qlen + (last_row >> group_log2) + 1);
    // keys [k0, k1) of this workgroup: all visible ones, or the split's share of them
    int k0 = 0, k1 = n_keys;
    int n_chunks = (n_keys + QS_FA_KEYS - 1) / QS_FA_KEYS;
    if constexpr (SPLIT) {
        const int S = gridDim.z;
        const int L = (((ctx + S - 1) / S) + QS_FA_KEYS - 1) & ~(QS_FA_KEYS - 1);
        k0 = blockIdx.z * L;
        k1 = min(k0 + L, n_keys);
        n_chunks = max(k1 - k0 + QS_FA_KEYS - 1, 0) / QS_FA_KEYS;   // 0: the range lies behind the horizon
    }

    // Q fragments: lane (row c16, d slice 8 g4 + 32 j); rows past the end repeat the last valid row (never stored)
    u32x4 qfrag[4];
    load_q_frag(qfrag, q, q_stride, min(rbase + c16, total_rows - 1), qs, group_log2, kvh, gmask, g4);
    // positions of this lane's accumulator rows (4 g4 + reg)
    int pos[4];
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        const int rr = rbase + 4 * g4 + reg;
        pos[reg] = rr < total_rows ? ctx - qlen + (rr >> group_log2) : -1;
    }
    float row_m[4], row_l[4];
    f32x4 o[8];
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        row_m[reg] = -__builtin_inff();
        row_l[reg] = 0.0f;
    }
#pragma unroll
    for (int dt = 0; dt < 8; dt++) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};

    // staging: thread (key = tid / 4, quarter = tid % 4) moves 64 B of the key's K row and of its V row
    const int skey = tid >> 2, spart = tid & 3;
    typename KvRaw<KVT>::type kreg[4], vreg[4];
    auto stage_load = [&](int kb) {   // unconditional, clamped (no load behind a branch)
        const int p = min(kb + skey, ctx - 1);
        const int64_t slot = ((int64_t)bt[min(p >> bs_log2, max_blocks - 1)] << bs_log2) + (p & bmask);
        const KVT* kp = key_cache + (slot * nkv + kvh) * D + spart * 32;
        const KVT* vp = value_cache + (slot * nkv + kvh) * D + spart * 32;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            kreg[i] = kv_load8<KVT>(kp + 8 * i);
            vreg[i] = kv_load8<KVT>(vp + 8 * i);
        }
    };
    stage_load(k0);
    for (int c = 0; c < n_chunks; c++) {
        const int kb = k0 + c * QS_FA_KEYS;
        const int nk = min(k1 - kb, QS_FA_KEYS);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int ci = spart * 4 + i;
            *reinterpret_cast<u32x4*>(kl + skey * 256 + ((ci ^ (skey & 15)) << 4)) = kv_f16x8(kreg[i]);
            const u32x4 vz = skey < nk ? kv_f16x8(vreg[i]) : u32x4{0, 0, 0, 0};   // zero rows keep the MFMA clean
            *reinterpret_cast<u32x4*>(vl + skey * QS_ATT_VSTRIDE + ci * 8) = vz;
        }
        __syncthreads();
        stage_load(kb + QS_FA_KEYS);   // next chunk underneath this one (clamped re-read behind the last chunk)

        // ---- S = Q K^T for the wave's 16 rows x 64 keys: lane holds rows 4 g4 + reg, key column t * 16 + c16
        f32x4 sacc[4];
#pragma unroll
        for (int t = 0; t < 4; t++) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            const int row = t * 16 + c16;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const u32x4 kf = *reinterpret_cast<const u32x4*>(kl + row * 256 + (((g4 + 4 * j) ^ (row & 15)) << 4));
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, qfrag[j]),
                                                             __builtin_bit_cast(f16x8, kf), acc, 0, 0, 0);
            }
            const int p = kb + t * 16 + c16;
#pragma unroll
            for (int reg = 0; reg < 4; reg++) sacc[t][reg] = p <= pos[reg] ? acc[reg] * sm_scale : -__builtin_inff();
        }
        // ---- online softmax per row: the 16 lanes of a g4 group hold the 64 keys of rows 4 g4 + reg
        float alpha[4];
        online_softmax_tiles<4, PSTR>(sacc, row_m, row_l, alpha, pl, c16, g4);
#pragma unroll
        for (int dt = 0; dt < 8; dt++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) o[dt][reg] *= alpha[reg];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the wave's own P tile: LDS is in order per wave
        // ---- O += P V: A = P (row c16, keys st * 32 + 8 g4 ..), B = V[keys][d0 + c16] through the transposing read
        {
            const uint32_t vl_base = (uint32_t)(uintptr_t)vl;
            const int qd = c16 >> 2, pq = c16 & 3;
#pragma unroll
            for (int st = 0; st < 2; st++) {
                const f16x8 pa = *reinterpret_cast<const f16x8*>(pl + c16 * PSTR + st * 32 + g4 * 8);
                const f16x8 pb = *reinterpret_cast<const f16x8*>(pl + (16 + c16) * PSTR + st * 32 + g4 * 8);
                const int krow = st * 32 + g4 * 8 + qd;
                u32x2 lo[8], hi[8];
                lds_read_tr_b16_x16(vl_base + (uint32_t)((krow * QS_ATT_VSTRIDE + 4 * pq) * 2), lo, hi);
#pragma unroll
                for (int dt = 0; dt < 8; dt++) {
                    const u32x4 bw = {lo[dt][0], lo[dt][1], hi[dt][0], hi[dt][1]};
                    o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pb, __builtin_bit_cast(f16x8, bw), o[dt], 0, 0, 0);
                    o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pa, __builtin_bit_cast(f16x8, bw), o[dt], 0, 0, 0);
                }
            }
        }
        __syncthreads();   // kl / vl are rewritten by the next chunk
    }
    // ---- results: lane holds rows 4 g4 + reg, columns dt * 16 + c16
    if constexpr (FP8) {
#pragma unroll
        for (int dt = 0; dt < 8; dt++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) o[dt][reg] *= v_scale;
    }
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        const int rr = rbase + 4 * g4 + reg;
        if (rr < total_rows) {
            size_t th = token_head(rr, qs, group_log2, kvh, gmask, nq);
            if constexpr (SPLIT) th = th * gridDim.z + blockIdx.z;   // [T, nq, S, ..]
            if (ws_o) {
#pragma unroll
                for (int dt = 0; dt < 8; dt++) ws_o[th * D + dt * 16 + c16] = o[dt][reg];
                if (c16 == 0) {
                    ws_ml[th * 2] = row_m[reg];
                    ws_ml[th * 2 + 1] = row_l[reg];
                }
            }
            if (!SPLIT && out) {
#pragma unroll
                for (int dt = 0; dt < 8; dt++) out[th * D + dt * 16 + c16] = f2h(o[dt][reg] / row_l[reg]);
            }
        }
    }
}

template <typename KVT, bool SPLIT>
static int launch_prefill(const AttnArgs& a, const AttnForm& f) {
    const AttnWs w = attn_ws(a.ws, (size_t)a.n_seqs * a.max_q_len, a.nq, a.d, f.S);
    if (const int rc = attn_launch<paged_attention_prefill_kernel<KVT, SPLIT>, KVT>(256, a, f, a.nq, a.nkv, f.bs_log2, f.group_log2,
                                                                                    a.sm_scale, f.n_rb, w.o, w.ml, a.out, a.v_scale))
        return rc;
    if (f.merge) attn_launch_split_merge(a, f, w);   // SPLIT, out != NULL: no ticket counters, the launch boundary is the hand-off
    return 0;
}
int attn_launch_prefill(const AttnArgs& a, const AttnForm& f) {
    if (f.family == ATTN_PREFILL_SPLIT) return a.fp8 ? launch_prefill<uint8_t, true>(a, f) : launch_prefill<f16, true>(a, f);
    return a.fp8 ? launch_prefill<uint8_t, false>(a, f) : launch_prefill<f16, false>(a, f);
}

}  // namespace qspec
