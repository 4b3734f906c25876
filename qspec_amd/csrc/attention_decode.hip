// Paged causal attention for the two QSpec query shapes (draft q_len = 1, verify q_len = k+1), head size 128: the chunk
// kernel and the keys-over-waves kernel, with their launchers.  attention.hip decides which one runs.
//
// Replaces (reference, relative to /root/reference):
//   flash_attn_with_kvcache / flash_attn_varlen_func (vllm_flash_attn wheel, un-vendored; call sites
//                                        vllm/attention/backends/flash_attn.py:741-830)
#include "attention_common.cuh"

namespace qspec {

// ---------------------------------------------------------------- attention
// Split-context ("flash-decoding") paged attention, one launch, both products on the matrix cores.
//   grid (n_seqs, n_kv_heads * n_rb, n_splits), 256 threads = 4 waves.  A workgroup takes the keys
//   [split*128, split*128+128) of one sequence and one kv head, and up to 16 query rows (row = query token x
//   GQA head of that kv head: 4 rows for the draft pass, 16 for verify k=3; longer queries use n_rb row blocks).
//
//   At these sizes a wave's INSTRUCTION COUNT is the cost (one wave per SIMD issues ~1 instruction / 4 cycles),
//   so the kernel is shaped to need few of them:
//     * S = Q K^T: Q and K are both d-contiguous, so MFMA fragments are plain 16-byte global loads
//       (wave w owns key tiles 2w, 2w+1); 8 v_mfma_f32_16x16x32_f16 per wave.
//     * softmax: S (fp32) sits in LDS as [row][key]; 16 lanes share a row, reduce with 4 shuffles, P goes back
//       as fp16 [row][key] = exactly the A fragment layout of the second product.
//     * O = P V: V rows are staged once in LDS ([key][d], 288-byte row stride) and read back TRANSPOSED with
//       ds_read_b64_tr_b16, so B fragments cost 2 LDS reads instead of 8 gathers; wave w owns output columns
//       32w..32w+31 (no cross-wave reduction); 8 MFMAs per wave.
//     * block_size and the GQA group are powers of two: no integer division anywhere.
//   Every global load of the workgroup is issued before the first use (one dependent chain:
//   block table -> K/V).  The partial (o, m, l) of a split goes to the workspace; the LAST workgroup to
//   arrive for a (sequence, kv head, row block) merges the splits in split order (deterministic) and writes
//   fp16 -- agent-scope release / acquire around a relaxed ticket counter (reset for the next call).
// d = 128 only.

// PF: the loads of chunk i+1 fly underneath chunk i (64 more VGPRs: one workgroup per CU -- the decode shape at small
// batch, where the launch is 256 workgroups of dependent round trips).  PF = false halves the register footprint so that
// two workgroups share a CU: large batches, where occupancy hides the same latency.
// BT: the sequence's block-table row (<= 128 entries) is fetched into two registers per lane together with the
// per-sequence metadata, and the chunk lookups become lane permutes: the dependent chain metadata -> table entry -> K / V
// loses one memory round trip.
// (A wave-uniform form of the table lookup -- a K tile / the 16-key group of a V row lies in ONE block when block_size >= 16,
// so v_readlane + SALU instead of 20 ds_bpermute -- is what paged_attention_waves_kernel<.., FAST> uses; HERE it measured
// slower, 6.16 against 6.05 us per launch and 7.57 against 7.53 ms per cycle: the serial SALU chain is longer than the
// pipelined permutes.)
// KVT = uint8_t (fp8 KV cache): a K / V piece of eight elements is an 8-byte load of e4m3 bytes, held as loaded and widened to
// the eight halves of the fp16 form at its first use (exact); LDS, MFMAs and softmax see the same fp16 operands either way.
// sm_scale arrives with k_scale folded in; v_scale multiplies the split's output where the partial is stored.
template <bool PF, bool BT, typename KVT>
__global__ __launch_bounds__(256) void paged_attention_kernel(
    const f16* __restrict__ q, int64_t q_stride, const KVT* __restrict__ key_cache, const KVT* __restrict__ value_cache,
    const int32_t* __restrict__ block_tables, int max_blocks, const int32_t* __restrict__ ctx_lens,
    const int32_t* __restrict__ q_start, int nq, int nkv, int bs_log2, int group_log2, float sm_scale, int n_splits,
    int n_rb, int* cnt, float* ws_o, float* ws_ml, f16* __restrict__ out, int merge, float v_scale) {
    constexpr bool FP8 = sizeof(KVT) == 1;
    constexpr int D = 128;
#ifdef QS_ATT_STAMPS
    long long stamp[10];
#define QS_STAMP(i) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(stamp[i])::"memory")
#else
#define QS_STAMP(i)
#endif
    QS_STAMP(9);   // entry
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* sc = reinterpret_cast<float*>(smem_raw);                          // [16 rows][128 keys] fp32 scores
    f16* pl = reinterpret_cast<f16*>(sc + QS_ATT_MAXR * QS_ATT_CHUNK);       // [16 rows][128 keys] fp16 probabilities
    f16* pl2 = pl + QS_ATT_MAXR * QS_ATT_CHUNK;                              // low half of the fp32 probability (p - fp16(p))
    f16* vl = pl2 + QS_ATT_MAXR * QS_ATT_CHUNK;                              // [128 keys][QS_ATT_VSTRIDE]
    float* row_m = reinterpret_cast<float*>(vl + QS_ATT_CHUNK * QS_ATT_VSTRIDE);  // [16]
    float* row_l = row_m + QS_ATT_MAXR;                                      // [16]
    float* wgt = row_l + QS_ATT_MAXR;                                        // [16][QS_ATT_MAXSPLIT] merge weights
    int* flag = reinterpret_cast<int*>(wgt + QS_ATT_MAXR * QS_ATT_MAXSPLIT); // [1]
    const int seq = blockIdx.x, kvh = blockIdx.y / n_rb, rb = blockIdx.y % n_rb, split = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int gmask = (1 << group_log2) - 1, bmask = (1 << bs_log2) - 1;
    BtRow btrow{0, 0};
    if constexpr (BT) btrow = bt_row_load(block_tables, seq, max_blocks, lane);   // in the same round trip as the metadata (the early return below depends on it)
    const SeqMeta sm = seq_meta(q_start, ctx_lens, seq, lane);
    const int qs = sm.qs, qlen = sm.qlen, ctx = sm.ctx;
    const int r0 = rb * QS_ATT_MAXR;
    const int R = min(QS_ATT_MAXR, (qlen << group_log2) - r0);
    if (R <= 0) return;  // uniform for the whole workgroup
    // Keys per split adapt to the sequence (split_keys).  A split longer than 128 keys is walked
    // in 128-key chunks with a running (max, sum, output) -- flash-decoding with an inner loop -- so the number of
    // splits (and of partials to merge) stays put while the context grows; the loads of chunk i+1 are issued before
    // chunk i is consumed.  One chunk per split is the same arithmetic as before the loop existed.
    const SplitKeys sk = split_keys(ctx, n_splits, split);
    const int kps = sk.kps, k_begin = sk.k_begin, k_end = sk.k_end;
    const int n_it = max(1, (min(kps, max(k_end - k_begin, 0)) + QS_ATT_CHUNK - 1) / QS_ATT_CHUNK);
    const int c16 = lane & 15, g4 = lane >> 4;
    const int32_t* bt = block_tables + (size_t)seq * max_blocks;
    auto bt_get = [&](int bi) -> int {   // bi already clamped to the table
        if constexpr (BT) return btrow.get(bi);
        else return bt[bi];
    };
    QS_STAMP(0);

    // No load below sits behind a branch (hipcc answers control flow around a load with s_waitcnt vmcnt(0), which
    // would serialise the prefetch): block-table indices and key rows are clamped, out-of-range keys are masked
    // after the load (scores -> -inf, V rows -> 0).
    struct Slots {
        int64_t k[2], v[8];
    };
    struct KV {
        typename KvRaw<KVT>::type kfrag[2][4], vraw[8];
    };
    // Keys past the split's end are masked after the load; their ADDRESSES are those of the split's last key, so that a
    // 64-key split does not pull the neighbouring split's 64 keys through this CU as well (a chunk is 128 keys: twice the
    // bytes in flight, i.e. a second round trip of the CU's ~32 KB window -- 6.7 us per launch at 8 splits of a 512-key
    // context).  Lanes with equal addresses coalesce inside the wave instruction.
    const int k_last = max(k_end - 1, 0);
    // Slots hold ELEMENT offsets of the rows' first element of this kv head: (slot * nkv + kvh) * D
    auto lookup = [&](Slots& sl, int kb) {   // block-table entries of the chunk starting at key kb
#pragma unroll
        for (int t2 = 0; t2 < 2; t2++) {
            const int p = min(kb + (wave * 2 + t2) * 16 + c16, k_last);
            sl.k[t2] = ((((int64_t)bt_get(min(p >> bs_log2, max_blocks - 1)) << bs_log2) + (p & bmask)) * nkv + kvh) * D;
        }
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int p = min(kb + wave * 4 + g4 + 16 * i, k_last);
            sl.v[i] = ((((int64_t)bt_get(min(p >> bs_log2, max_blocks - 1)) << bs_log2) + (p & bmask)) * nkv + kvh) * D;
        }
    };
    auto fetch = [&](KV& kv, const Slots& sl) {
#pragma unroll
        for (int t2 = 0; t2 < 2; t2++) {  // lane (key c16 of tile 2w+t2, d slice 8*g4 + 32j)
            const KVT* kp = key_cache + sl.k[t2] + g4 * 8;
#pragma unroll
            for (int j = 0; j < 4; j++) kv.kfrag[t2][j] = kv_load8<KVT>(kp + 32 * j);
        }
#pragma unroll
        for (int i = 0; i < 8; i++)  // 16 lanes cover one V row (256 bytes of fp16); wave w, group g4 -> keys 4w+g4 + 16i
            kv.vraw[i] = kv_load8<KVT>(value_cache + sl.v[i] + c16 * 8);
    };
    Slots sl_cur, sl_nxt;
    lookup(sl_cur, k_begin);
    if constexpr (PF) lookup(sl_nxt, k_begin + (n_it > 1 ? QS_ATT_CHUNK : 0));
    u32x4 qfrag[4];
    {  // lane (row c16, d slice 8*g4 + 32j); rows >= R repeat row 0 (their outputs are never stored)
       // (load_q_frag's text kept here: through the helper the PF = true fp8 instantiation takes two more VGPRs)
        const int r = r0 + (c16 < R ? c16 : 0);
        const int tok = qs + (r >> group_log2), head = (kvh << group_log2) + (r & gmask);
        const f16* qp = q + (size_t)tok * q_stride + (size_t)head * D + g4 * 8;
#pragma unroll
        for (int j = 0; j < 4; j++) qfrag[j] = *reinterpret_cast<const u32x4*>(qp + 32 * j);
    }
    KV cur, nxt;
    fetch(cur, sl_cur);
    if (tid < QS_ATT_MAXR) {
        row_m[tid] = -__builtin_inff();
        row_l[tid] = 0.0f;
    }
    float* row_a = wgt;   // [16] rescale factors of the running output (wgt is free until the merge)
    f32x4 o0 = {0.f, 0.f, 0.f, 0.f}, o1 = {0.f, 0.f, 0.f, 0.f};
    QS_STAMP(1);

    int qpos[4];   // absolute position of the query token of this lane's score rows 4 g4 + reg
#pragma unroll
    for (int reg = 0; reg < 4; reg++) qpos[reg] = ctx - qlen + ((r0 + 4 * g4 + reg) >> group_log2);
    auto process = [&](const KV& kv, int kb, bool last) {
        const int nkeys = __builtin_amdgcn_readfirstlane(max(0, min(k_end - kb, QS_ATT_CHUNK)));   // uniform: scalar branches below
        // ---- S = Q K^T (fp32 accumulate) -> sc[row][key], masked and scaled
#pragma unroll
        for (int t2 = 0; t2 < 2; t2++) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; j++)
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, qfrag[j]),
                                                             __builtin_bit_cast(f16x8, kv_f16x8(kv.kfrag[t2][j])), acc, 0, 0, 0);
            const int kk = (wave * 2 + t2) * 16 + c16;  // lane holds rows 4*g4 + reg of key column kk
            const int p = kb + kk;
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {   // one compare-and-select per score: no short-circuit branches
                const bool ok = (kk < nkeys) & (p <= qpos[reg]);
                sc[(4 * g4 + reg) * QS_ATT_CHUNK + kk] = ok ? acc[reg] * sm_scale : -__builtin_inff();
            }
        }
        // V rows -> LDS: only the 32-key steps P.V walks (st * 32 < nkeys), zeros beyond nkeys inside the last of them
        // (uniform branches around LDS stores; no global load sits behind them)
        if ((nkeys & 31) == 0) {
#pragma unroll
            for (int i = 0; i < 8; i++)
                if (16 * i < nkeys)
                    *reinterpret_cast<u32x4*>(vl + (wave * 4 + g4 + 16 * i) * QS_ATT_VSTRIDE + c16 * 8) = kv_f16x8(kv.vraw[i]);
        } else {
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int kk = wave * 4 + g4 + 16 * i;
                const u32x4 vz = kk < nkeys ? kv_f16x8(kv.vraw[i]) : u32x4{0, 0, 0, 0};
                if (16 * i < ((nkeys + 31) & ~31)) *reinterpret_cast<u32x4*>(vl + kk * QS_ATT_VSTRIDE + c16 * 8) = vz;
            }
        }
        if (last) QS_STAMP(3);
        __syncthreads();
        // ---- softmax over the 128 keys of a row, folded into the running (max, sum): thread (row = tid>>4, 8 keys)
        {
            const int r = tid >> 4, ks = tid & 15;
            const float4 a = *reinterpret_cast<const float4*>(sc + r * QS_ATT_CHUNK + ks * 8);
            const float4 b = *reinterpret_cast<const float4*>(sc + r * QS_ATT_CHUNK + ks * 8 + 4);
            float s8[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            float mx = s8[0];
#pragma unroll
            for (int i = 1; i < 8; i++) mx = fmaxf(mx, s8[i]);
            // the 16 lanes of a row exchange through DPP (max: order independent)
            mx = fmaxf(mx, dpp_xor<8>(mx));
            mx = fmaxf(mx, dpp_xor<4>(mx));
            mx = fmaxf(mx, dpp_xor<2>(mx));
            mx = fmaxf(mx, dpp_xor<1>(mx));
            const float m_old = row_m[r];              // the row's 16 lanes sit in one wave: read before lane 0 writes
            const float m_new = fmaxf(m_old, mx);
            float sum = 0.0f;
            f16x8 p8, p8lo;
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const float pv = m_new == -__builtin_inff() ? 0.0f : aexp(s8[i] - m_new);
                // the matrix core takes fp16 operands: carry the fp32 probability as hi + lo so that P.V keeps
                // fp32-class accuracy (22 bits) for two MFMAs instead of one
                const f16 ph = f2h(pv);
                p8[i] = ph;
                p8lo[i] = f2h(pv - h2f(ph));
                sum += pv;
            }
            sum += dpp_xor<8>(sum);   // same pairing order as the xor butterfly it replaces (8, 4, 2, 1)
            sum += dpp_xor<4>(sum);
            sum += dpp_xor<2>(sum);
            sum += dpp_xor<1>(sum);
            *reinterpret_cast<f16x8*>(pl + r * QS_ATT_CHUNK + ks * 8) = p8;
            *reinterpret_cast<f16x8*>(pl2 + r * QS_ATT_CHUNK + ks * 8) = p8lo;
            if (ks == 0) {
                const float alpha = m_old == -__builtin_inff() ? 0.0f : aexp(m_old - m_new);   // e^0 = 1 exactly
                row_a[r] = alpha;
                row_m[r] = m_new;
                row_l[r] = __builtin_fmaf(row_l[r], alpha, sum);   // first chunk: 0 * 0 + sum
            }
        }
        if (last) QS_STAMP(7);
        __syncthreads();
        if (last) QS_STAMP(8);
        // ---- O = O * alpha + P V: wave w owns d columns 32w..32w+31 (two 16-wide tiles), k over the 128 keys in 4 steps
        {
#pragma unroll
            for (int reg = 0; reg < 4; reg++) {
                const float al = row_a[4 * g4 + reg];
                o0[reg] *= al;
                o1[reg] *= al;
            }
            const uint32_t vl_base = (uint32_t)(uintptr_t)vl;  // LDS byte address (low 32 bits of the shared pointer)
            const int qd = c16 >> 2, pq = c16 & 3;              // lane 4q+p of its 16-lane group
#pragma unroll
            for (int st = 0; st < 4; st++) {
                if (st * 32 >= nkeys) continue;   // uniform: P is all zero there (short splits: 64 keys = two of the four steps)
                const f16x8 pa = *reinterpret_cast<const f16x8*>(pl + c16 * QS_ATT_CHUNK + st * 32 + g4 * 8);
                const f16x8 pb = *reinterpret_cast<const f16x8*>(pl2 + c16 * QS_ATT_CHUNK + st * 32 + g4 * 8);
                // B fragment of lane (col c16, group g4) = V[key st*32 + 8*g4 + j][d0 + c16], j = 0..7
                const int krow = st * 32 + g4 * 8 + qd;
#pragma unroll
                for (int dt = 0; dt < 2; dt++) {
                    const int d0 = wave * 32 + dt * 16;
                    const uint32_t a0 = vl_base + (uint32_t)((krow * QS_ATT_VSTRIDE + d0 + 4 * pq) * 2);
                    const s16x8 bw = __builtin_shufflevector(lds_tr16(a0), lds_tr16(a0 + 4 * QS_ATT_VSTRIDE * 2), 0, 1, 2, 3, 4, 5, 6, 7);
                    if (dt == 0) {
                        o0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(pb, __builtin_bit_cast(f16x8, bw), o0, 0, 0, 0);
                        o0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(pa, __builtin_bit_cast(f16x8, bw), o0, 0, 0, 0);
                    } else {
                        o1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(pb, __builtin_bit_cast(f16x8, bw), o1, 0, 0, 0);
                        o1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(pa, __builtin_bit_cast(f16x8, bw), o1, 0, 0, 0);
                    }
                }
            }
        }
        if (!last) __syncthreads();   // sc / pl / vl / row_a are rewritten by the next chunk
    };

    int kb = k_begin;
    for (int it = 0; it < n_it - 1; it++) {
        if constexpr (PF) {
            fetch(nxt, sl_nxt);                                     // chunk it+1: in flight underneath chunk it
            lookup(sl_nxt, kb + 2 * QS_ATT_CHUNK);                  // table entries of chunk it+2 (clamped)
            process(cur, kb, false);
            cur = nxt;
        } else {
            lookup(sl_nxt, kb + QS_ATT_CHUNK);                      // the next chunk's table entries under this chunk
            process(cur, kb, false);
            fetch(cur, sl_nxt);
        }
        kb += QS_ATT_CHUNK;
    }
#ifdef QS_ATT_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    QS_STAMP(2);   // the (last) chunk's K / V are here
#endif
    process(cur, kb, true);
    QS_STAMP(4);
    // ---- partial of this split -> workspace: ws_o [T, nq, n_splits, D], ws_ml [T, nq, n_splits, 2]
    // lane holds rows 4*g4 + reg, columns wave*32 + {0,16} + c16
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        const int r = 4 * g4 + reg;
        if (r < R) {
            float* dst = ws_o + (token_head(r0 + r, qs, group_log2, kvh, gmask, nq) * n_splits + split) * D + wave * 32 + c16;
            if constexpr (FP8) {
                dst[0] = o0[reg] * v_scale;
                dst[16] = o1[reg] * v_scale;
            } else {
                dst[0] = o0[reg];
                dst[16] = o1[reg];
            }
        }
    }
    if (tid < R) {
        const size_t o = (token_head(r0 + tid, qs, group_log2, kvh, gmask, nq) * n_splits + split) * 2;
        ws_ml[o] = row_m[tid];
        ws_ml[o + 1] = row_l[tid];
    }
    QS_STAMP(5);
    // merge == 0: the consumer kernel (heads_hadamard_merge) combines the splits; the launch boundary is the hand-off
#ifdef QS_ATT_STAMPS
    if (!merge && tid == 0 && seq == 0 && kvh == 0 && rb == 0 && split == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        QS_STAMP(6);
        long long* sb = reinterpret_cast<long long*>(cnt + 2048);
        for (int i = 0; i < 10; i++) sb[i] = stamp[i];
    }
#endif
    if (!merge) return;
    // ---- hand-off: every storing wave drains, one lane releases and takes a ticket
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int* my_cnt = cnt + (seq * nkv + kvh) * n_rb + rb;
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const int ticket = __hip_atomic_fetch_add(my_cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *flag = ticket == n_splits - 1;
    }
    __syncthreads();
    QS_STAMP(6);
    if (!*flag) return;
    if (tid == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(my_cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // ready for the next call
    }
    __syncthreads();
    QS_STAMP(7);
    // ---- merge: out = sum_s w_s o_s / sum_s w_s l_s, w_s = e^(m_s - M), splits in order.
    // Thread i owns 4 output columns of one row; its o loads (up to 8 splits at a time) go out first, the
    // per-row weights are computed meanwhile by 16 threads and passed through LDS.
    const int NV = R * (D / 4);
    for (int i0 = 0; i0 < NV; i0 += 256) {
        const int i = i0 + tid;
        const bool act = i < NV;
        const int r = act ? i / (D / 4) : 0, e4 = act ? (i % (D / 4)) * 4 : 0;
        const size_t th = token_head(r0 + r, qs, group_log2, kvh, gmask, nq);
        float4 o8[8];
#pragma unroll
        for (int s2 = 0; s2 < 8; s2++) {
            o8[s2] = float4{0.f, 0.f, 0.f, 0.f};
            if (act && s2 < n_splits) o8[s2] = *reinterpret_cast<const float4*>(ws_o + (th * n_splits + s2) * D + e4);
        }
        if (i0 == 0) {
            if (tid < R) {
                const size_t t2 = token_head(r0 + tid, qs, group_log2, kvh, gmask, nq);
                float M = -__builtin_inff();
                for (int s2 = 0; s2 < n_splits; s2++) M = fmaxf(M, ws_ml[(t2 * n_splits + s2) * 2]);
                float den = 0.0f;
                for (int s2 = 0; s2 < n_splits; s2++) {
                    const float m = ws_ml[(t2 * n_splits + s2) * 2];
                    const float w = merge_weight(m, M);
                    wgt[tid * QS_ATT_MAXSPLIT + s2] = w;
                    den = __builtin_fmaf(w, ws_ml[(t2 * n_splits + s2) * 2 + 1], den);
                }
                row_l[tid] = den;
            }
            __syncthreads();
        }
        if (act) {
            float4 num = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s2 = 0; s2 < 8; s2++) {
                if (s2 < n_splits) {
                    const float w = wgt[r * QS_ATT_MAXSPLIT + s2];
                    num.x = __builtin_fmaf(w, o8[s2].x, num.x);
                    num.y = __builtin_fmaf(w, o8[s2].y, num.y);
                    num.z = __builtin_fmaf(w, o8[s2].z, num.z);
                    num.w = __builtin_fmaf(w, o8[s2].w, num.w);
                }
            }
            for (int s2 = 8; s2 < n_splits; s2++) {
                const float w = wgt[r * QS_ATT_MAXSPLIT + s2];
                const float4 o4 = *reinterpret_cast<const float4*>(ws_o + (th * n_splits + s2) * D + e4);
                num.x = __builtin_fmaf(w, o4.x, num.x);
                num.y = __builtin_fmaf(w, o4.y, num.y);
                num.z = __builtin_fmaf(w, o4.z, num.z);
                num.w = __builtin_fmaf(w, o4.w, num.w);
            }
            const float den = row_l[r];
            f16x4 o = {f2h(num.x / den), f2h(num.y / den), f2h(num.z / den), f2h(num.w / den)};
            *reinterpret_cast<f16x4*>(out + th * D + e4) = o;
        }
    }
#ifdef QS_ATT_STAMPS
    QS_STAMP(8);
    if (tid == 0 && seq == 0 && kvh == 0 && rb == 0) {
        long long* sb = reinterpret_cast<long long*>(cnt + 2048);
        for (int i = 0; i < 9; i++) sb[i] = stamp[i];
    }
#endif
}

// ---------------------------------------------------------------- decode, the keys of a workgroup split over its WAVES
// Same grid, same partials as paged_attention_kernel (16 rows per workgroup, context splits on blockIdx.z), but no
// workgroup-wide phase inside the key loop: wave w walks the 32-key slices w, w+4, ... of the split on its own -- K
// fragments straight from the cache into registers, V through a wave-private LDS tile for the transposing reads,
// S / softmax / P.V and a running (max, sum, output) per wave -- and the four waves' results are combined once at
// the end (wave order: deterministic).  The next slice's loads fly underneath the current one.  Where the 128-key
// chunk loop of paged_attention_kernel spends 2.7 us in barrier-separated phases per chunk, the waves here overlap
// each other: large batches and long contexts (more than one chunk per workgroup).  Partials only (out == NULL form).
// NW waves per workgroup (4; 8 behind QSPEC_ATTN_NW): a wave has ONE slice (16 KB of K + V) in flight beside the one it
// works on.  A pure read of config 3's 67 MB with 32 KB per CU in flight takes 21.8 us, 13-14 us with twice that
// (scripts/micro/kvread.hip) -- but eight waves = two per SIMD are SLOWER here (21.6 against 19.1 us): in-kernel stamps
// (-DQS_ATT_STAMPS, scripts/bench_attn_cold.py) show a wave stuck 0.5-1.8 us per slice at the ISSUE of its refill loads
// (the CU's request window is full) with its softmax + P.V (1.35 us per slice) behind that.
// FAST (needs BT, block_size >= 16; a split starts on a 16-key boundary): a 32-key slice is two 16-key halves of ONE
// block each, so a slice needs two table entries, not ten -- wave-uniform, taken with v_readlane from the table row in
// registers -- and every K / V address is a uniform 64-bit base (SALU) plus a lane offset that never changes.  The
// general form spends ~250 of its ~700 loop instructions on lane permutes and 64-bit address arithmetic per slice and
// needs AGPR copies (291 VGPRs); at one wave per SIMD the instruction count IS the slice time.
template <bool BT, int NW, bool FAST, typename KVT>   // BT: block-table row in registers, lookups as lane permutes; KVT: see paged_attention_kernel
__global__ __launch_bounds__(64 * NW, NW == 4 ? 2 : 1) void paged_attention_waves_kernel(
    const f16* __restrict__ q, int64_t q_stride, const KVT* __restrict__ key_cache, const KVT* __restrict__ value_cache,
    const int32_t* __restrict__ block_tables, int max_blocks, const int32_t* __restrict__ ctx_lens,
    const int32_t* __restrict__ q_start, int nq, int nkv, int bs_log2, int group_log2, float sm_scale, int n_splits,
    int n_rb, float* __restrict__ ws_o, float* __restrict__ ws_ml, float v_scale) {
    constexpr bool FP8 = sizeof(KVT) == 1;
    constexpr int D = 128, PSTR = 40;   // P row stride in halves (80 B)
    constexpr int WAVE_LDS = QS_AW_KEYS * QS_ATT_VSTRIDE * 2 + 2 * 16 * PSTR * 2;   // V tile + P hi/lo tile, bytes
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    const int seq = blockIdx.x, kvh = blockIdx.y / n_rb, rb = blockIdx.y % n_rb, split = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c16 = lane & 15, g4 = lane >> 4;
    const int gmask = (1 << group_log2) - 1, bmask = (1 << bs_log2) - 1;
    f16* vl = reinterpret_cast<f16*>(smem_raw + wave * WAVE_LDS);
    f16* pl = vl + QS_AW_KEYS * QS_ATT_VSTRIDE;
    BtRow btrow{0, 0};
    if constexpr (BT) btrow = bt_row_load(block_tables, seq, max_blocks, lane);
    const SeqMeta sm = seq_meta(q_start, ctx_lens, seq, lane);
    const int qs = sm.qs, qlen = sm.qlen, ctx = sm.ctx;
    const int r0 = rb * QS_ATT_MAXR;
    const int R = min(QS_ATT_MAXR, (qlen << group_log2) - r0);
    if (R <= 0) return;  // uniform for the whole workgroup
    const SplitKeys sk = split_keys(ctx, n_splits, split);
    const int k_begin = sk.k_begin, k_end = sk.k_end;
    const int n_sl = (max(k_end - k_begin, 0) + QS_AW_KEYS - 1) / QS_AW_KEYS;
    const int32_t* bt = block_tables + (size_t)seq * max_blocks;

    auto bt_get = [&](int bi) -> int {   // bi already clamped to the table
        if constexpr (BT) return btrow.get(bi);
        else return bt[bi];
    };
    struct Slots {
        int64_t k[2], v[8];
    };
    struct KV {
        typename KvRaw<KVT>::type kf[2][4], vr[8];
    };
    auto lookup = [&](Slots& sl, int sb) {   // clamped: no load behind a branch
#pragma unroll
        for (int t2 = 0; t2 < 2; t2++) {
            const int p = sb + t2 * 16 + c16;
            sl.k[t2] = ((int64_t)bt_get(min(p >> bs_log2, max_blocks - 1)) << bs_log2) + (p & bmask);
        }
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int p = sb + i * 4 + g4;
            sl.v[i] = ((int64_t)bt_get(min(p >> bs_log2, max_blocks - 1)) << bs_log2) + (p & bmask);
        }
    };
    // FAST: uniform element offsets of the slice's two 16-key halves, ((slot * nkv) + kvh) * D
    static_assert(!FAST || BT, "the fast lookup reads the table row from registers");
    auto ublock = [&](int bi) -> int {   // bi wave-uniform
        return btrow.get_uniform(__builtin_amdgcn_readfirstlane(min(bi, max_blocks - 1)));
    };
    auto lookup_u = [&](int64_t (&base)[2], int sbu) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int p = sbu + 16 * h;
            const int64_t slot = ((int64_t)ublock(p >> bs_log2) << bs_log2) + (p & bmask);
            base[h] = (slot * nkv + kvh) * D;
        }
    };
    const int k_lane = (c16 * nkv) * D + g4 * 8, v_lane = (g4 * nkv) * D + c16 * 8;   // elements; < 2^31 (nkv * 16 * 128)
    const int v_step = 4 * nkv * D;                                                   // four rows further
    auto fetch_k_u = [&](KV& kv, const int64_t (&base)[2]) {
#pragma unroll
        for (int t2 = 0; t2 < 2; t2++) {
            const KVT* kp = key_cache + base[t2] + k_lane;
#pragma unroll
            for (int j = 0; j < 4; j++) kv.kf[t2][j] = kv_load8<KVT>(kp + 32 * j);
        }
    };
    auto fetch_v_u = [&](KV& kv, const int64_t (&base)[2]) {
#pragma unroll
        for (int i = 0; i < 8; i++)
            kv.vr[i] = kv_load8<KVT>(value_cache + base[i >> 2] + (int64_t)((i & 3) * v_step) + v_lane);
    };
    auto fetch = [&](KV& kv, const Slots& sl) {
#pragma unroll
        for (int t2 = 0; t2 < 2; t2++) {   // lane (key c16 of tile t2, d slice 8 g4 + 32 j)
            const KVT* kp = key_cache + (sl.k[t2] * nkv + kvh) * D + g4 * 8;
#pragma unroll
            for (int j = 0; j < 4; j++) kv.kf[t2][j] = kv_load8<KVT>(kp + 32 * j);
        }
#pragma unroll
        for (int i = 0; i < 8; i++)   // 16 lanes cover one V row: key 4 i + g4 of the slice
            kv.vr[i] = kv_load8<KVT>(value_cache + (sl.v[i] * nkv + kvh) * D + c16 * 8);
    };
#ifdef QS_ATT_STAMPS
    long long awst[24];
    int awn = 0;
#define QS_AWST() do { if (awn < 24) { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(awst[awn])::"memory"); awn++; } } while (0)
#define QS_AWST_NW() do { if (awn < 24) { asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(awst[awn])::"memory"); awn++; } } while (0)
#else
#define QS_AWST()
#define QS_AWST_NW()
#endif
    QS_AWST_NW();   // 0: metadata here
    int sb = (FAST ? __builtin_amdgcn_readfirstlane(k_begin) : k_begin) + wave * QS_AW_KEYS;
    Slots sl_cur, sl_nxt;
    int64_t ub[2];
    if constexpr (FAST) {
        lookup_u(ub, sb);
    } else {
        lookup(sl_cur, sb);
        lookup(sl_nxt, sb + NW * QS_AW_KEYS);
    }
    u32x4 qfrag[4];
    load_q_frag(qfrag, q, q_stride, r0 + (c16 < R ? c16 : 0), qs, group_log2, kvh, gmask, g4);   // rows >= R repeat row 0
    KV cur;
    if constexpr (FAST) {
        fetch_k_u(cur, ub);
        fetch_v_u(cur, ub);
    } else {
        fetch(cur, sl_cur);
    }
    int pos[4];
    float row_m[4], row_l[4];
    f32x4 o[8];
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        pos[reg] = ctx - qlen + ((r0 + 4 * g4 + reg) >> group_log2);
        row_m[reg] = -__builtin_inff();
        row_l[reg] = 0.0f;
    }
#pragma unroll
    for (int dt = 0; dt < 8; dt++) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    const uint32_t vl_base = (uint32_t)(uintptr_t)vl;
    const int qd = c16 >> 2, pq = c16 & 3;
    QS_AWST_NW();   // 1: first slice requested

    for (int s2 = wave; s2 < n_sl; s2 += NW) {
        QS_AWST();  // loop top: the slice's K and V have arrived (stamp build only: waits for everything)
        const int nkeys = max(0, min(k_end - sb, QS_AW_KEYS));
        // ---- S = Q K^T: lane holds rows 4 g4 + reg, key column t2 * 16 + c16.  Each K register is refilled with the
        // wave's NEXT slice right behind its last use (as the weight ring of gemm_stream_w4a4.hip): the loads never stop.
        f32x4 sacc[2];
#pragma unroll
        for (int t2 = 0; t2 < 2; t2++) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < 4; j++)
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, qfrag[j]),
                                                             __builtin_bit_cast(f16x8, kv_f16x8(cur.kf[t2][j])), acc, 0, 0, 0);
            const int kk = t2 * 16 + c16, p = sb + kk;
#pragma unroll
            for (int reg = 0; reg < 4; reg++)
                sacc[t2][reg] = (kk < nkeys && p <= pos[reg]) ? acc[reg] * sm_scale : -__builtin_inff();
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (FAST) {
            lookup_u(ub, sb + NW * QS_AW_KEYS);   // the wave's next slice (clamped to the table: no load behind a branch)
            fetch_k_u(cur, ub);
        } else {
#pragma unroll
            for (int t2 = 0; t2 < 2; t2++) {
                const KVT* kp = key_cache + (sl_nxt.k[t2] * nkv + kvh) * D + g4 * 8;
#pragma unroll
                for (int j = 0; j < 4; j++) cur.kf[t2][j] = kv_load8<KVT>(kp + 32 * j);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // V rows -> the wave's LDS tile (zeros past the end keep the MFMA clean), registers refilled the same way
        if (nkeys == QS_AW_KEYS) {   // uniform; LDS stores only (no global load sits behind this branch)
#pragma unroll
            for (int i = 0; i < 8; i++)
                *reinterpret_cast<u32x4*>(vl + (i * 4 + g4) * QS_ATT_VSTRIDE + c16 * 8) = kv_f16x8(cur.vr[i]);
        } else {
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int kk = i * 4 + g4;
                const u32x4 vz = kk < nkeys ? kv_f16x8(cur.vr[i]) : u32x4{0, 0, 0, 0};
                *reinterpret_cast<u32x4*>(vl + kk * QS_ATT_VSTRIDE + c16 * 8) = vz;
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (FAST) {
            fetch_v_u(cur, ub);
        } else {
#pragma unroll
            for (int i = 0; i < 8; i++)
                cur.vr[i] = kv_load8<KVT>(value_cache + (sl_nxt.v[i] * nkv + kvh) * D + c16 * 8);
        }
        __builtin_amdgcn_sched_barrier(0);
        QS_AWST_NW();   // QK + refills issued + V in LDS
        if constexpr (!FAST) lookup(sl_nxt, sb + 2 * NW * QS_AW_KEYS);           // table entries of the slice after the next (clamped)
        // ---- running softmax: the 16 lanes of a g4 group hold the 32 keys of rows 4 g4 + reg
        float alpha[4];
        online_softmax_tiles<2, PSTR>(sacc, row_m, row_l, alpha, pl, c16, g4);
#pragma unroll
        for (int dt = 0; dt < 8; dt++)
#pragma unroll
            for (int reg = 0; reg < 4; reg++) o[dt][reg] *= alpha[reg];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the wave's own tiles: LDS is in order per wave
        // ---- O += P V (one 32-key step): A = P (row c16, keys 8 g4 ..), B = V through the transposing reads
        {
            const f16x8 pa = *reinterpret_cast<const f16x8*>(pl + c16 * PSTR + g4 * 8);
            const f16x8 pb = *reinterpret_cast<const f16x8*>(pl + (16 + c16) * PSTR + g4 * 8);
            const uint32_t va = vl_base + (uint32_t)(((g4 * 8 + qd) * QS_ATT_VSTRIDE + 4 * pq) * 2);
            s16x8 bw[8];   // d tile dt: +32 B; the fragment's second key quad: +4 V rows
#pragma unroll
            for (int dt = 0; dt < 8; dt++)
                bw[dt] = __builtin_shufflevector(lds_tr16(va + 32 * dt), lds_tr16(va + 32 * dt + 4 * QS_ATT_VSTRIDE * 2), 0, 1, 2,
                                                 3, 4, 5, 6, 7);
#pragma unroll
            for (int dt = 0; dt < 8; dt++) {
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pb, __builtin_bit_cast(f16x8, bw[dt]), o[dt], 0, 0, 0);
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(pa, __builtin_bit_cast(f16x8, bw[dt]), o[dt], 0, 0, 0);
            }
        }
        sb += NW * QS_AW_KEYS;
        QS_AWST_NW();   // slice done (softmax + P.V)
    }
    QS_AWST_NW();
    // ---- combine the four waves (wave order), store the split's partial: ws_o [T, nq, n_splits, D], ws_ml [.., 2]
    __syncthreads();   // every wave is done with its private tiles: the same LDS now carries the exchange
    float* co = reinterpret_cast<float*>(smem_raw);          // [NW][16][128]
    float* cml = co + NW * 16 * D;                            // [NW][16][2]
#pragma unroll
    for (int reg = 0; reg < 4; reg++) {
        const int r = 4 * g4 + reg;
#pragma unroll
        for (int dt = 0; dt < 8; dt++) co[(wave * 16 + r) * D + dt * 16 + c16] = o[dt][reg];
        if (c16 == 0) {
            cml[(wave * 16 + r) * 2] = row_m[reg];
            cml[(wave * 16 + r) * 2 + 1] = row_l[reg];
        }
    }
    __syncthreads();
    {
        const int r = tid >> 4, c8 = (tid & 15) * 8;
        if (r < R) {   // R <= 16: the first 256 threads
            float M = -__builtin_inff();
#pragma unroll
            for (int w = 0; w < NW; w++) M = fmaxf(M, cml[(w * 16 + r) * 2]);
            float l = 0.0f, acc8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int w = 0; w < NW; w++) {
                const float m = cml[(w * 16 + r) * 2];
                const float wg = merge_weight(m, M);
                l = __builtin_fmaf(wg, cml[(w * 16 + r) * 2 + 1], l);
                const float4 a = *reinterpret_cast<const float4*>(co + (w * 16 + r) * D + c8);
                const float4 b = *reinterpret_cast<const float4*>(co + (w * 16 + r) * D + c8 + 4);
                acc8[0] = __builtin_fmaf(wg, a.x, acc8[0]); acc8[1] = __builtin_fmaf(wg, a.y, acc8[1]);
                acc8[2] = __builtin_fmaf(wg, a.z, acc8[2]); acc8[3] = __builtin_fmaf(wg, a.w, acc8[3]);
                acc8[4] = __builtin_fmaf(wg, b.x, acc8[4]); acc8[5] = __builtin_fmaf(wg, b.y, acc8[5]);
                acc8[6] = __builtin_fmaf(wg, b.z, acc8[6]); acc8[7] = __builtin_fmaf(wg, b.w, acc8[7]);
            }
            const size_t th = token_head(r0 + r, qs, group_log2, kvh, gmask, nq);
            float* dst = ws_o + (th * n_splits + split) * D + c8;
            if constexpr (FP8) {
#pragma unroll
                for (int e = 0; e < 8; e++) acc8[e] *= v_scale;
            }
            *reinterpret_cast<float4*>(dst) = float4{acc8[0], acc8[1], acc8[2], acc8[3]};
            *reinterpret_cast<float4*>(dst + 4) = float4{acc8[4], acc8[5], acc8[6], acc8[7]};
            if ((tid & 15) == 0) {
                ws_ml[(th * n_splits + split) * 2] = M;
                ws_ml[(th * n_splits + split) * 2 + 1] = l;
            }
        }
    }
#ifdef QS_ATT_STAMPS
    QS_AWST_NW();
    if (tid == 0 && blockIdx.x == 1 && blockIdx.y == 1 && blockIdx.z == 0) {
        long long* sbp = reinterpret_cast<long long*>(ws_o) - (QS_ATT_CNT_SLOTS / 2) + 1024;   // int slot 2048 of the counters
        sbp[0] = awn;
        for (int i = 0; i < awn; i++) sbp[1 + i] = awst[i];
    }
#endif
}

// ---------------------------------------------------------------- launchers: one table of instantiations each
// X(PF, BT)
#define QS_ATT_CHUNK_FORMS(X) X(true, true) X(true, false) X(false, true) X(false, false)
template <typename KVT>
static int launch_chunk(const AttnArgs& a, const AttnForm& f) {
    const AttnWs w = attn_ws(a.ws, (size_t)a.n_seqs * a.max_q_len, a.nq, a.d, f.S);
#define X(PFV, BTV)                                                                                                      \
    if (f.pf == PFV && f.bt == BTV)                                                                                      \
        return attn_launch<paged_attention_kernel<PFV, BTV, KVT>, KVT>(256, a, f, a.nq, a.nkv, f.bs_log2, f.group_log2,  \
                                                                       a.sm_scale, f.S, f.n_rb, w.cnt, w.o, w.ml, a.out, \
                                                                       f.merge ? 1 : 0, a.v_scale);
    QS_ATT_CHUNK_FORMS(X)
#undef X
    return -1;
}
int attn_launch_chunk(const AttnArgs& a, const AttnForm& f) {
    return a.fp8 ? launch_chunk<uint8_t>(a, f) : launch_chunk<f16>(a, f);
}

// X(BT, NW, FAST); eight waves (QSPEC_ATTN_NW=8) exist in the experimental library only
#ifdef QS_EXPERIMENTAL
#define QS_AW_FORMS_NW8(X) X(true, 8, true) X(true, 8, false) X(false, 8, false)
#else
#define QS_AW_FORMS_NW8(X)
#endif
#define QS_AW_FORMS(X) X(true, 4, true) X(true, 4, false) X(false, 4, false) QS_AW_FORMS_NW8(X)
template <typename KVT>
static int launch_waves(const AttnArgs& a, const AttnForm& f) {
    const AttnWs w = attn_ws(a.ws, (size_t)a.n_seqs * a.max_q_len, a.nq, a.d, f.S);
#define X(BTV, NWV, FV)                                                                                                  \
    if (f.bt == BTV && f.nw == NWV && f.fast == FV)                                                                      \
        return attn_launch<paged_attention_waves_kernel<BTV, NWV, FV, KVT>, KVT>(64 * NWV, a, f, a.nq, a.nkv, f.bs_log2, \
                                                                                 f.group_log2, a.sm_scale, f.S, f.n_rb,  \
                                                                                 w.o, w.ml, a.v_scale);
    QS_AW_FORMS(X)
#undef X
    return -1;
}
int attn_launch_waves(const AttnArgs& a, const AttnForm& f) {
    return a.fp8 ? launch_waves<uint8_t>(a, f) : launch_waves<f16>(a, f);
}

}  // namespace qspec
