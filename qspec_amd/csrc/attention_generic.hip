// Paged causal attention for head sizes other than 128 (the plumbing path), the split merge behind it, and their launcher.
#include "attention_common.cuh"

namespace qspec {

// ---------------------------------------------------------------- generic head size (plumbing path)
// Any head_size <= 256 (TinyLlama: 64).  One 128-thread workgroup per (query token, head): scores of all visible keys
// into LDS (fp32 dot products), one softmax over them, then thread j accumulates output dimension j over the keys in
// order (fp32, deterministic).  No context split, no matrix cores: correctness path for configurations the MFMA
// kernel (head_size 128) does not cover, not a tuned one.
__global__ __launch_bounds__(128) void paged_attention_generic_kernel(
    const f16* __restrict__ q, int64_t q_stride, const f16* __restrict__ key_cache, const f16* __restrict__ value_cache,
    const int32_t* __restrict__ block_tables, int max_blocks, const int32_t* __restrict__ ctx_lens,
    const int32_t* __restrict__ q_start, int n_seqs, int nq, int nkv, int d, int block_size, float sm_scale,
    f16* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* sc = reinterpret_cast<float*>(smem_raw);   // [ctx]
    __shared__ float red[4];
    const int t = blockIdx.x, h = blockIdx.y, tid = threadIdx.x;
    int seq = 0;
    while (seq + 1 < n_seqs && q_start[seq + 1] <= t) seq++;
    const int qs = q_start[seq], qlen = q_start[seq + 1] - qs, ctx = ctx_lens[seq];
    if (t - qs >= qlen) return;
    const int pos = ctx - qlen + (t - qs);            // absolute position of this query token
    const int nvis = pos + 1;                          // causal: keys 0..pos
    const int kvh = h / (nq / nkv);
    const f16* qp = q + (size_t)t * q_stride + (size_t)h * d;
    const int32_t* bt = block_tables + (size_t)seq * max_blocks;
    float mx = -__builtin_inff();
    for (int k = tid; k < nvis; k += 128) {
        const int64_t slot = (int64_t)bt[k / block_size] * block_size + k % block_size;
        const f16* kp = key_cache + (slot * nkv + kvh) * d;
        float acc = 0.0f;
        for (int e = 0; e < d; e++) acc = __builtin_fmaf(h2f(qp[e]), h2f(kp[e]), acc);
        acc *= sm_scale;
        sc[k] = acc;
        mx = fmaxf(mx, acc);
    }
    mx = wave_max_f(mx);
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(red[0], red[1]);
    __syncthreads();
    float sum = 0.0f;
    for (int k = tid; k < nvis; k += 128) {
        const float p = qexpf(sc[k] - mx);
        sc[k] = p;
        sum += p;
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) sum += shfl_xor_f(sum, m);
    if ((tid & 63) == 0) red[2 + (tid >> 6)] = sum;
    __syncthreads();
    const float den = red[2] + red[3];
    for (int e = tid; e < d; e += 128) {
        float acc = 0.0f;
        for (int k = 0; k < nvis; k++) {
            const int64_t slot = (int64_t)bt[k / block_size] * block_size + k % block_size;
            acc = __builtin_fmaf(sc[k], h2f(value_cache[(slot * nkv + kvh) * d + e]), acc);
        }
        out[((size_t)t * nq + h) * d + e] = f2h(acc / den);
    }
}

// The same arithmetic with vector loads (head_size a multiple of 8; round 3: TinyLlama's bs = 1 cycle spent 47 % of its time
// in the kernel above, 51 us per launch: its P.V phase ran head_size threads through one DEPENDENT 2-byte load per key).
// 256 threads: a thread's score is the same e-ascending fma chain over 16-byte pieces of the key row (all pieces of a row
// in flight together); P.V stages chunks of 256 / (head_size / 8) V rows through LDS with one 16-byte piece per thread
// (next chunk in flight in registers while the current one is accumulated) and thread e then adds the chunk's keys in
// ascending order: the output sums are those of the kernel above bit for bit; the softmax denominator is summed in a
// different (fixed) grouping.
template <typename KVT>   // see paged_attention_kernel ("16-byte piece" below = eight elements: 8 bytes of an fp8 cache)
__global__ __launch_bounds__(256) void paged_attention_generic_vec_kernel(
    const f16* __restrict__ q, int64_t q_stride, const KVT* __restrict__ key_cache, const KVT* __restrict__ value_cache,
    const int32_t* __restrict__ block_tables, int max_blocks, const int32_t* __restrict__ ctx_lens,
    const int32_t* __restrict__ q_start, int n_seqs, int nq, int nkv, int d, int block_size, float sm_scale,
    f16* __restrict__ out, float* __restrict__ ws_o, float* __restrict__ ws_ml, float v_scale) {
    constexpr bool FP8 = sizeof(KVT) == 1;
    typedef typename KvRaw<KVT>::type raw_t;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    __shared__ float red[8];
    __shared__ __attribute__((aligned(16))) f16 qrow[256];
    const int t = blockIdx.x, h = blockIdx.y, tid = threadIdx.x;
    int seq = 0;
    while (seq + 1 < n_seqs && q_start[seq + 1] <= t) seq++;
    const int qs = q_start[seq], qlen = q_start[seq + 1] - qs, ctx = ctx_lens[seq];
    if (t - qs >= qlen) return;   // (uniform)
    const int pos = ctx - qlen + (t - qs);            // absolute position of this query token
    const int nall = pos + 1;                          // causal: keys 0..pos
    // context splits (gridDim.z = S > 1, or partials wanted): split sp takes keys [kbase, kbase + nvis) -- whole 16-key groups,
    // the same length for every split of a token; an empty split leaves (m, l, o) = (-inf, 0, 0)
    const int S = gridDim.z, sp = blockIdx.z;
    const int per = S > 1 ? ((((nall + S - 1) / S) + 15) & ~15) : nall;
    const int kbase = min(nall, sp * per);
    const int nvis = min(nall - kbase, per);           // keys of this workgroup (0: an empty split)
    const int kvh = h / (nq / nkv);
    const int32_t* bt = block_tables + (size_t)seq * max_blocks;
    const int pieces = d >> 3;                         // 16-byte pieces per row
    const int RG = 256 / pieces;                       // row groups of the P.V pass (threads beyond RG * pieces idle there)
    float* sc = reinterpret_cast<float*>(smem_raw);   // [nvis rounded up to 4]
    float* pvr = reinterpret_cast<float*>(smem_raw + (((size_t)nvis * 4 + 15) & ~(size_t)15));   // [RG][d] partial output rows
    if (tid < pieces)
        *reinterpret_cast<u32x4*>(qrow + tid * 8) = *reinterpret_cast<const u32x4*>(q + (size_t)t * q_stride + (size_t)h * d + tid * 8);
    // the V rows do not depend on the scores: this thread's first PRE of them are requested here, in front of the K rows
    constexpr int PRE = 8;
    const int rg = tid / pieces, vp = tid - rg * pieces;
    const bool pv_on = rg < RG;
    auto vaddr = [&](int k) -> const KVT* {
        const int kc = min(kbase + min(k, nvis - 1), nall - 1);   // clamped: no branch around a load (rows past the end are not used)
        const int64_t slot = (int64_t)bt[kc / block_size] * block_size + kc % block_size;
        return value_cache + (slot * nkv + kvh) * d + vp * 8;
    };
    raw_t vpre[PRE];
#pragma unroll
    for (int j = 0; j < PRE; j++) vpre[j] = kv_load8<KVT>(vaddr(rg + RG * j));
    __syncthreads();
    // scores: NK keys per thread and trip -- their table entries first, then every K piece in flight, then the dot products
    // (one key per trip was two dependent round trips per key: 512 keys = four of them per thread)
    constexpr int NK = 4;
    float mx = -__builtin_inff();
    for (int kb = tid; kb < nvis; kb += 256 * NK) {
        const KVT* kp[NK];
#pragma unroll
        for (int i = 0; i < NK; i++) {
            const int kc = min(kbase + min(kb + 256 * i, nvis - 1), nall - 1);   // clamped: rows past the end are loaded, not used
            const int64_t slot = (int64_t)bt[kc / block_size] * block_size + kc % block_size;
            kp[i] = key_cache + (slot * nkv + kvh) * d;
        }
        float acc[NK];
#pragma unroll
        for (int i = 0; i < NK; i++) acc[i] = 0.0f;
        for (int p0 = 0; p0 < pieces; p0 += 8) {      // up to 8 pieces of each row in flight
            raw_t kr[NK][8];
#pragma unroll
            for (int i = 0; i < NK; i++)
#pragma unroll
                for (int j = 0; j < 8; j++) kr[i][j] = kv_load8<KVT>(kp[i] + min(p0 + j, pieces - 1) * 8);
#pragma unroll
            for (int j = 0; j < 8; j++) {
                if (p0 + j < pieces) {
                    const f16x8 q8 = *reinterpret_cast<const f16x8*>(qrow + (p0 + j) * 8);
#pragma unroll
                    for (int i = 0; i < NK; i++) {
                        const f16x8 k8 = __builtin_bit_cast(f16x8, kv_f16x8(kr[i][j]));
#pragma unroll
                        for (int e = 0; e < 8; e++) acc[i] = __builtin_fmaf(h2f(q8[e]), h2f(k8[e]), acc[i]);
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < NK; i++) {
            const int k = kb + 256 * i;
            if (k < nvis) {
                const float a = acc[i] * sm_scale;
                sc[k] = a;
                mx = fmaxf(mx, a);
            }
        }
    }
    mx = wave_max_f(mx);
    if ((tid & 63) == 0) red[tid >> 6] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float sum = 0.0f;
    for (int k = tid; k < nvis; k += 256) {
        const float pv = qexpf(sc[k] - mx);
        sc[k] = pv;
        sum += pv;
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) sum += shfl_xor_f(sum, m);
    if ((tid & 63) == 0) red[4 + (tid >> 6)] = sum;
    __syncthreads();
    const float den = (red[4] + red[5]) + (red[6] + red[7]);
    // ---- P.V: thread (row group rg, 16-byte piece vp) sums p_k * V[k][8 vp .. 8 vp + 8) over the keys rg, rg + RG, ...
    // (the first eight of its rows were requested in front of the scores), then the RG partial rows are added in order.
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; e++) acc[e] = 0.0f;
    auto fma8 = [&](float pk, raw_t raw) {
        const f16x8 v8 = __builtin_bit_cast(f16x8, kv_f16x8(raw));
#pragma unroll
        for (int e = 0; e < 8; e++) acc[e] = __builtin_fmaf(pk, h2f(v8[e]), acc[e]);
    };
    const int pv_rows = min(RG, nvis);   // row groups that saw a key (the others wrote nothing)
    if (pv_on && rg < nvis) {
#pragma unroll
        for (int j = 0; j < PRE; j++) {
            const int k = rg + RG * j;
            if (k < nvis) fma8(sc[k], vpre[j]);
        }
        for (int k0 = rg + RG * PRE; k0 < nvis; k0 += RG * PRE) {   // long contexts: eight more rows in flight per trip
            raw_t vb[PRE];
#pragma unroll
            for (int j = 0; j < PRE; j++) vb[j] = kv_load8<KVT>(vaddr(k0 + RG * j));
#pragma unroll
            for (int j = 0; j < PRE; j++) {
                const int k = k0 + RG * j;
                if (k < nvis) fma8(sc[k], vb[j]);
            }
        }
#pragma unroll
        for (int e = 0; e < 8; e++) pvr[(size_t)rg * d + vp * 8 + e] = acc[e];
    }
    __syncthreads();
    if (tid < d) {
        float o = pv_rows > 0 ? pvr[tid] : 0.0f;
        for (int r2 = 1; r2 < pv_rows; r2++) o += pvr[(size_t)r2 * d + tid];
        if constexpr (FP8) o *= v_scale;
        if (ws_o) {   // partials of split sp: unnormalised output, (row maximum, sum of exponentials)
            const size_t ths = ((size_t)t * nq + h) * S + sp;
            ws_o[ths * d + tid] = o;
            if (tid == 0) *reinterpret_cast<float2*>(ws_ml + ths * 2) = float2{mx, den};
        } else {
            out[((size_t)t * nq + h) * d + tid] = f2h(o / den);
        }
    }
}

// Split merge for the generic head sizes and for the context-split prompt kernel (attention_prefill.hip) when the caller wants fp16 rows (the reference-order path; the engine merges in
// the head-transform launch, hadamard.hip: heads_hadamard_merge_cols_kernel -- same expression, same bits):
// out = h( sum_s w_s o_s / sum_s w_s l_s ), w_s = e^(m_s - M), splits in order.
__global__ __launch_bounds__(256) void paged_attention_generic_merge_kernel(const float* __restrict__ ws_o,
                                                                            const float* __restrict__ ws_ml, int S, int d,
                                                                            f16* __restrict__ out, const int32_t* __restrict__ q_start,
                                                                            int n_seqs, int nq) {
    const size_t th = blockIdx.x;   // token * nq + head
    if ((int)(th / nq) >= q_start[n_seqs]) return;   // the grid covers n_seqs * max_q_len tokens, `out` the real ones
    const float* mlb = ws_ml + th * S * 2;
    float M = -__builtin_inff();
    for (int s2 = 0; s2 < S; s2++) M = fmaxf(M, mlb[s2 * 2]);
    for (int c = threadIdx.x; c < d; c += 256) {
        float num = 0.0f, den = 0.0f;
        for (int s2 = 0; s2 < S; s2++) {
            const float m = mlb[s2 * 2];
            const float w = merge_weight(m, M);
            den = __builtin_fmaf(w, mlb[s2 * 2 + 1], den);
            num = __builtin_fmaf(w, ws_o[(th * S + s2) * d + c], num);
        }
        out[th * d + c] = f2h(num / den);
    }
}

void attn_launch_split_merge(const AttnArgs& a, const AttnForm& f, const AttnWs& w) {
    const size_t Tm = (size_t)a.n_seqs * a.max_q_len;
    hipLaunchKernelGGL(paged_attention_generic_merge_kernel, dim3((unsigned)(Tm * a.nq)), dim3(256), 0, a.st, w.o, w.ml, f.S, a.d,
                       a.out, a.q_start, a.n_seqs, a.nq);
}

template <typename KVT>
static int launch_generic_vec(const AttnArgs& a, const AttnForm& f) {
    const size_t Tm = (size_t)a.n_seqs * a.max_q_len;
    const AttnWs w = f.partials ? attn_ws(a.ws, Tm, a.nq, a.d, f.S) : AttnWs{nullptr, nullptr, nullptr};
    if (const int rc = attn_launch<paged_attention_generic_vec_kernel<KVT>, KVT>(256, a, f, a.n_seqs, a.nq, a.nkv, a.d, a.block_size,
                                                                                 a.sm_scale, a.out, w.o, w.ml, a.v_scale))
        return rc;
    if (f.merge) attn_launch_split_merge(a, f, w);
    return 0;
}
int attn_launch_generic(const AttnArgs& a, const AttnForm& f) {
    if (f.family == ATTN_GENERIC_VEC) return a.fp8 ? launch_generic_vec<uint8_t>(a, f) : launch_generic_vec<f16>(a, f);
    return attn_launch<paged_attention_generic_kernel, f16>(128, a, f, a.n_seqs, a.nq, a.nkv, a.d, a.block_size, a.sm_scale, a.out);
}

}  // namespace qspec
