// Token-side kernels: embedding gather, greedy sampler front end, rejection
// sampler (accept/reject + recovered token + output assembly + counters) and
// the on-GPU advance step of the draft loop.
//
// Replaces (reference, relative to /root/reference):
//   Sampler.forward greedy path            vllm/model_executor/layers/sampler.py:216-316 (modify_greedy_probs=False :293)
//   RejectionSampler.forward & helpers     vllm/model_executor/layers/rejection_sampler.py:60-399
//   SpecDecodeBaseSampler._create_output   vllm/model_executor/layers/spec_decode_base_sampler.py:69-131
//   advance_step_flashattn_kernel          csrc/prepare_inputs/advance_step.cu:14-64
// The reference runs ~15 small torch kernels over [B,k,V] fp32 per step; here it is two.
#include "common.cuh"
#include "kernels.h"

namespace qspec {

__global__ __launch_bounds__(256) void embedding_kernel(const int64_t* __restrict__ ids, const f16* __restrict__ table,
                                                        f16* __restrict__ out, int H, int V) {
    const int t = blockIdx.x;
    int64_t id = ids[t];
    if (id < 0 || id >= V) id = 0;  // padded slot
    const f16* src = table + id * H;
    for (int i = threadIdx.x; i < H / 8; i += blockDim.x)
        *reinterpret_cast<f16x8*>(out + (size_t)t * H + 8 * i) = *reinterpret_cast<const f16x8*>(src + 8 * i);
}
int embedding(const int64_t* ids, const f16* table, f16* out, int T, int H, int V, hipStream_t st) {
    if (T == 0) return 0;
    if (H % 8) return -1;
    hipLaunchKernelGGL(embedding_kernel, dim3(T), dim3(256), 0, st, ids, table, out, H, V);
    return 0;
}

// block-wide helpers (1024 threads = 16 waves)
struct ArgMax {
    float v;
    int i;
};
__device__ __forceinline__ ArgMax argmax_combine(ArgMax a, ArgMax b) {
    // larger value wins; on ties the smaller index (first occurrence) wins; NaN never wins
    if (b.v > a.v || (b.v == a.v && b.i < a.i)) return b;
    return a;
}
__device__ __forceinline__ ArgMax block_argmax(ArgMax a, ArgMax* red) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        ArgMax o;
        o.v = __shfl_xor(a.v, m, 64);
        o.i = __shfl_xor(a.i, m, 64);
        a = argmax_combine(a, o);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = a;
    __syncthreads();
    ArgMax r = red[0];
    for (int w = 1; w < nw; w++) r = argmax_combine(r, red[w]);
    return r;
}
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    double r = red[0];
    for (int w = 1; w < nw; w++) r += red[w];
    return r;
}

// probs = softmax_fp32(float(logits)); token = argmax (first index on ties).
// exp via qexpf, denominator accumulated in fp64 and rounded once (the oracle does the same), so the fp32
// probabilities are the oracle's bit for bit up to a ~2^-29 chance per row.
// A row of 128256 logits is ~1.8 MB of traffic; one workgroup per row would sit on one CU's ~25 GB/s share
// (150 us).  The row is cut into QS_SM_CHUNKS chunks, three small launches:
//   1. per chunk max / argmax            -> part_a[row][chunk]
//   2. row max from the partials, e = qexpf(l - M) -> probs, per chunk sum (fp64) -> part_s[row][chunk]
//   3. total in chunk order (deterministic), p = e / float(total); chunk 0 writes the token
#define QS_SM_CHUNKS 64
struct SmPartA {
    float v;
    int i;
};
__device__ __forceinline__ void sm_chunk_range(int V, int c, int& lo, int& hi) {
    const int len = (((V + QS_SM_CHUNKS - 1) / QS_SM_CHUNKS) + 7) & ~7;
    lo = min(V, c * len);
    hi = min(V, lo + len);
}
__global__ __launch_bounds__(256) void softmax_max_kernel(const f16* __restrict__ logits, SmPartA* __restrict__ part_a,
                                                          int V) {
    __shared__ ArgMax red_a[4];
    const int c = blockIdx.x, t = blockIdx.y;
    int lo, hi;
    sm_chunk_range(V, c, lo, hi);
    const f16* l = logits + (size_t)t * V;
    ArgMax am{-__builtin_inff(), 0x7fffffff};
    for (int v = lo + threadIdx.x; v < hi; v += 256) {
        float f = h2f(l[v]);
        if (f > am.v) {
            am.v = f;
            am.i = v;
        }
    }
    am = block_argmax(am, red_a);
    if (threadIdx.x == 0) part_a[t * QS_SM_CHUNKS + c] = SmPartA{am.v, am.i};
}
__device__ __forceinline__ ArgMax sm_row_max(const SmPartA* part_a, int t) {
    ArgMax am{-__builtin_inff(), 0x7fffffff};
    for (int c = 0; c < QS_SM_CHUNKS; c++) {
        SmPartA pa = part_a[t * QS_SM_CHUNKS + c];
        am = argmax_combine(am, ArgMax{pa.v, pa.i});
    }
    return am;
}
// np <= 256 partial maxima per row (QS_SM_CHUNKS from softmax_max_kernel, or one per workgroup of the lm_head
// launch): one load per thread, then a block reduction (call from all 256 threads of the workgroup)
__device__ __forceinline__ ArgMax sm_row_max_n(const SmPartA* part_a, int t, int np, ArgMax* red_a) {
    ArgMax am{-__builtin_inff(), 0x7fffffff};
    if ((int)threadIdx.x < np) {
        const SmPartA pa = part_a[(size_t)t * np + threadIdx.x];
        am = ArgMax{pa.v, pa.i};
    }
    return block_argmax(am, red_a);
}
// pass 2: the chunk's share of the denominator, sum of qexpf(l - M) in fp64.  Nothing is written to probs here: the
// fp16 logits (2 B per element, cache resident) are cheaper to read twice than an fp32 e-array is to write and re-read
// (the reference's softmax + log_softmax make two passes over T x V x 4 B, sampler.py:270-287).
__global__ __launch_bounds__(256) void softmax_sum_kernel(const f16* __restrict__ logits, const SmPartA* part_a, int np,
                                                          double* __restrict__ part_s, int V) {
    __shared__ double red_d[4];
    __shared__ ArgMax red_a[4];
    const int c = blockIdx.x, t = blockIdx.y;
    int lo, hi;
    sm_chunk_range(V, c, lo, hi);
    const float mx = sm_row_max_n(part_a, t, np, red_a).v;
    const f16* l = logits + (size_t)t * V;
    double den = 0.0;
    for (int v = lo + threadIdx.x; v < hi; v += 256) den += (double)qexpf(h2f(l[v]) - mx);
    den = block_sum_f64(den, red_d);
    if (threadIdx.x == 0) part_s[t * QS_SM_CHUNKS + c] = den;
}
// pass 3: p = qexpf(l - M) / float(total) written ONCE; chunk 0 writes the token
__global__ __launch_bounds__(256) void softmax_write_kernel(const f16* __restrict__ logits, const SmPartA* part_a,
                                                            int np, const double* part_s, float* __restrict__ probs,
                                                            int64_t* __restrict__ token, int64_t token_stride, int V) {
    __shared__ ArgMax red_a[4];
    const int c = blockIdx.x, t = blockIdx.y;
    int lo, hi;
    sm_chunk_range(V, c, lo, hi);
    double den = 0.0;
    for (int cc = 0; cc < QS_SM_CHUNKS; cc++) den += part_s[t * QS_SM_CHUNKS + cc];
    const float inv = (float)den;
    const ArgMax am = sm_row_max_n(part_a, t, np, red_a);
    const f16* l = logits + (size_t)t * V;
    float* p = probs + (size_t)t * V;
    for (int v = lo + threadIdx.x; v < hi; v += 256) p[v] = qexpf(h2f(l[v]) - am.v) / inv;
    if (c == 0 && threadIdx.x == 0) token[t * token_stride] = am.i == 0x7fffffff ? 0 : am.i;
}
size_t sampler_ws_bytes(int rows) { return (size_t)rows * QS_SM_CHUNKS * 16; }
int softmax_argmax(const f16* logits, float* probs, int64_t* token, int T, int V, void* ws, hipStream_t st) {
    if (T == 0) return 0;
    SmPartA* part_a = reinterpret_cast<SmPartA*>(ws);
    double* part_s = reinterpret_cast<double*>(reinterpret_cast<char*>(ws) + (size_t)T * QS_SM_CHUNKS * 8);
    hipLaunchKernelGGL(softmax_max_kernel, dim3(QS_SM_CHUNKS, T), dim3(256), 0, st, logits, part_a, V);
    hipLaunchKernelGGL(softmax_sum_kernel, dim3(QS_SM_CHUNKS, T), dim3(256), 0, st, logits, part_a, QS_SM_CHUNKS, part_s, V);
    hipLaunchKernelGGL(softmax_write_kernel, dim3(QS_SM_CHUNKS, T), dim3(256), 0, st, logits, part_a, QS_SM_CHUNKS,
                       part_s, probs, token, (int64_t)1, V);
    return 0;
}
// Behind an lm_head launch that left nparts <= 256 partial maxima per row: two launches, the logits are read twice
// (fp16) and probs written once.  ws: [rows][256] SmPartA, then [rows][QS_SM_CHUNKS] double.
size_t head_softmax_ws_bytes(int rows) { return (size_t)rows * (256 * 8 + QS_SM_CHUNKS * 8); }
void* head_softmax_part_max(void* ws, int rows) { return ws; }
int head_softmax_argmax(const f16* logits, float* probs, int64_t* token, int T, int V, int nparts, void* ws,
                        hipStream_t st) {
    if (T == 0) return 0;
    if (nparts < 1 || nparts > 256) return -1;
    SmPartA* part_a = reinterpret_cast<SmPartA*>(ws);
    double* part_s = reinterpret_cast<double*>(reinterpret_cast<char*>(ws) + (size_t)T * 256 * 8);
    hipLaunchKernelGGL(softmax_sum_kernel, dim3(QS_SM_CHUNKS, T), dim3(256), 0, st, logits, part_a, nparts, part_s, V);
    hipLaunchKernelGGL(softmax_write_kernel, dim3(QS_SM_CHUNKS, T), dim3(256), 0, st, logits, part_a, nparts, part_s,
                       probs, token, (int64_t)1, V);
    return 0;
}

// Philox4x32-10 (counter-based; the product's own stream -- CUDA's torch.rand stream is not reproducible here)
__device__ __forceinline__ void philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                           uint32_t out[4]) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
        uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
__device__ __forceinline__ float u01_open(uint32_t x) { return ((float)(x >> 8) + 0.5f) * (1.0f / 16777216.0f); }

// Per-sequence seeded draws (SamplingParams.seed; the reference's seeded_seqs, rejection_sampler.py:60-67,229-250,387-399).
// A row of a seeded sequence keys its Philox by the request alone (include/qspec_hip.h, "seeded draws"):
//   key = (seed lo, seed hi), counter = (c0, 0x80000000 | stream << 16 | j, base_pos, 0)
// c0 = v (per-token noise) or 0xFFFFFFFF (accept uniform).  Rows of unseeded sequences keep the engine stream's
// (seed, offset) key and counter bit for bit.  Every pointer is read at replay (captured graphs serve changing seeds).
// SeedRows (kernels.h) carries the per-sequence arrays.
struct PhiloxKey {
    uint32_t k0, k1, c1, c2, c3;
};
__device__ __forceinline__ PhiloxKey engine_key(uint64_t seed, uint64_t offset, uint32_t c1) {
    return PhiloxKey{(uint32_t)seed, (uint32_t)(seed >> 32), c1, (uint32_t)offset, (uint32_t)(offset >> 32)};
}
// the key of a row of sequence s at sub-index j: the sequence's own when it is seeded, else `fallback`
__device__ __forceinline__ PhiloxKey seeded_key(const SeedRows& sr, int s, uint32_t stream, int j, PhiloxKey fallback) {
    if (!sr.seeded[s]) return fallback;
    const uint64_t sd = (uint64_t)sr.seeds[s];
    return PhiloxKey{(uint32_t)sd, (uint32_t)(sd >> 32), 0x80000000u | (stream << 16) | ((uint32_t)j & 0xFFFFu),
                     (uint32_t)sr.base_pos[s], 0u};
}

// accepted[b,i] = U < min(1, q[x]/p[x]);
// recovered[b,i] = argmax_v ( max(q_v - p_v, FLT_MIN) / S ) / E_v ,  S = sum_v max(q_v - p_v, FLT_MIN)
// target_probs [B, k+1, V], draft_probs (b,i,v) at b*dp_sb + i*dp_sk + v.  uniform [B,k] / exponential [B,k,V] may
// be injected (tests); when null they come from Philox keyed by (seed, offset).
// Same shape as the softmax: each (b,i) row is cut into QS_SM_CHUNKS chunks over the chip.
//   1. per chunk sum of max(q-p, tiny) in fp64                       -> part_s
//   2. S = float(total in chunk order); per chunk argmax of (f/S)/E  -> part_a
//   3. one workgroup: final argmax per (b,i), accept test, output assembly + counters
__global__ __launch_bounds__(256) void rejection_sum_kernel(const float* __restrict__ target_probs,
                                                            const float* __restrict__ draft_probs, int k, int V,
                                                            int64_t dp_sb, int64_t dp_sk,
                                                            double* __restrict__ part_s) {
    __shared__ double red_d[4];
    const int c = blockIdx.x, bk = blockIdx.y, b = bk / k, i = bk % k;
    int lo, hi;
    sm_chunk_range(V, c, lo, hi);
    const float* q = target_probs + ((size_t)b * (k + 1) + i) * V;
    const float* p = draft_probs + b * dp_sb + i * dp_sk;
    const float tiny = 1.17549435e-38f;
    double s = 0.0;
    for (int v = lo + threadIdx.x; v < hi; v += 256) s += (double)fmaxf(q[v] - p[v], tiny);
    s = block_sum_f64(s, red_d);
    if (threadIdx.x == 0) part_s[bk * QS_SM_CHUNKS + c] = s;
}
// SEEDED: sequence b of a seeded row draws from its own key (stream 3, j = i); the unseeded instantiation is the
// engine-stream kernel as it always was
template <bool SEEDED>
__global__ __launch_bounds__(256) void rejection_argmax_kernel(const float* __restrict__ target_probs,
                                                               const float* __restrict__ draft_probs,
                                                               const float* __restrict__ exponential, uint64_t seed,
                                                               uint64_t offset, const uint64_t* __restrict__ rng_state,
                                                               int k, int V, int64_t dp_sb, int64_t dp_sk,
                                                               const double* part_s, SmPartA* __restrict__ part_a,
                                                               SeedRows sr) {
    __shared__ ArgMax red_a[4];
    const int c = blockIdx.x, bk = blockIdx.y, b = bk / k, i = bk % k;
    int lo, hi;
    sm_chunk_range(V, c, lo, hi);
    const float* q = target_probs + ((size_t)b * (k + 1) + i) * V;
    const float* p = draft_probs + b * dp_sb + i * dp_sk;
    if (rng_state) {  // device-resident (seed, offset): lets a captured graph draw fresh numbers every replay
        seed = rng_state[0];
        offset = rng_state[1];
    }
    PhiloxKey pk = engine_key(seed, offset, (uint32_t)bk);
    if (SEEDED) pk = seeded_key(sr, b, 3u, i, pk);
    const float tiny = 1.17549435e-38f;
    double tot = 0.0;
    for (int cc = 0; cc < QS_SM_CHUNKS; cc++) tot += part_s[bk * QS_SM_CHUNKS + cc];
    const float S = (float)tot;
    ArgMax am{-__builtin_inff(), 0x7fffffff};
    for (int v = lo + threadIdx.x; v < hi; v += 256) {
        float f = fmaxf(q[v] - p[v], tiny) / S;
        float e;
        if (exponential) {
            e = exponential[(size_t)bk * V + v];
        } else {
            uint32_t r[4];
            philox4x32((uint32_t)v, pk.c1, pk.c2, pk.c3, pk.k0, pk.k1, r);
            e = -__logf(u01_open(r[0]));
        }
        float val = f / e;
        if (val > am.v) {
            am.v = val;
            am.i = v;
        }
    }
    am = block_argmax(am, red_a);
    if (threadIdx.x == 0) part_a[bk * QS_SM_CHUNKS + c] = SmPartA{am.v, am.i};
}
// SpecDecodeBaseSampler._create_output + the counters (spec_decode_base_sampler.py:69-131), shared by the rejection and the
// typical-acceptance sampler: out[b, i] = draft token (i < limit) | recovered (i == limit) | -1; out[b, k] = bonus iff every
// draft token was accepted; counters[0] += accepted.sum() (non-causal), counters[1] += #(out != -1), counters[2] += B*k.
// Call from every thread of ONE workgroup, behind the barrier that made accepted / recovered visible.
__device__ __forceinline__ void create_output(int B, int k, const int64_t* __restrict__ draft_ids, int64_t di_sb, int64_t di_sk,
                                              const int64_t* __restrict__ bonus_ids, int64_t bonus_stride,
                                              const uint8_t* accepted, const int64_t* recovered, int64_t* __restrict__ out,
                                              int64_t* __restrict__ counters, const int32_t* __restrict__ active_lens) {
    int acc_cnt = 0, emit_cnt = 0, rows_on = 0;
    for (int b = threadIdx.x; b < B; b += blockDim.x) {
        if (active_lens && active_lens[b] <= 0) {
            for (int i = 0; i <= k; i++) out[b * (k + 1) + i] = -1;
            continue;
        }
        rows_on++;
        int limit = k;
        for (int i = 0; i < k; i++) {
            if (accepted[b * k + i]) acc_cnt++;
            else if (limit == k) limit = i;
        }
        for (int i = 0; i < k; i++) {
            int64_t v = i < limit ? draft_ids[b * di_sb + i * di_sk] : (i == limit ? recovered[b * k + i] : -1);
            out[b * (k + 1) + i] = v;
            emit_cnt += v != -1;
        }
        int64_t last = limit == k ? bonus_ids[b * bonus_stride] : -1;
        out[b * (k + 1) + k] = last;
        emit_cnt += last != -1;
    }
    if (counters) {
        if (acc_cnt) atomicAdd(reinterpret_cast<unsigned long long*>(counters), (unsigned long long)acc_cnt);
        if (emit_cnt) atomicAdd(reinterpret_cast<unsigned long long*>(counters + 1), (unsigned long long)emit_cnt);
        if (rows_on) atomicAdd(reinterpret_cast<unsigned long long*>(counters + 2), (unsigned long long)rows_on * k);
    }
}

// Final step + output assembly + counters; one workgroup.  SEEDED: the accept uniform of a seeded sequence b comes
// from its own key (stream 4, j = i).
template <bool SEEDED>
__global__ __launch_bounds__(1024) void rejection_output_kernel(
    const float* __restrict__ target_probs, const float* __restrict__ draft_probs,
    const int64_t* __restrict__ draft_ids, const int64_t* __restrict__ bonus_ids, const float* __restrict__ uniform,
    uint64_t seed, uint64_t offset, uint64_t* __restrict__ rng_state, const SmPartA* part_a, int B, int k, int V,
    int64_t dp_sb, int64_t dp_sk, int64_t di_sb, int64_t di_sk, int64_t bonus_stride, uint8_t* __restrict__ accepted,
    int64_t* __restrict__ recovered, int64_t* __restrict__ out, int64_t* __restrict__ counters,
    const int32_t* __restrict__ active_lens, SeedRows sr) {
    // active_lens (may be NULL): row b takes part iff active_lens[b] > 0 (an empty batch slot of the engine emits
    // nothing and is not counted: the reference only ever sees the sequences that are scheduled)
    if (rng_state) {
        seed = rng_state[0];
        offset = rng_state[1];
    }
    for (int bk = threadIdx.x; bk < B * k; bk += blockDim.x) {
        const int b = bk / k, i = bk % k;
        ArgMax am{-__builtin_inff(), 0x7fffffff};
        for (int c = 0; c < QS_SM_CHUNKS; c++) {
            SmPartA pa = part_a[bk * QS_SM_CHUNKS + c];
            am = argmax_combine(am, ArgMax{pa.v, pa.i});
        }
        const int64_t x = draft_ids[b * di_sb + i * di_sk];
        float u;
        if (uniform) {
            u = uniform[bk];
        } else {
            PhiloxKey pk = engine_key(seed, offset, (uint32_t)bk);
            if (SEEDED) pk = seeded_key(sr, b, 4u, i, pk);
            uint32_t r[4];
            philox4x32(0xFFFFFFFFu, pk.c1, pk.c2, pk.c3, pk.k0, pk.k1, r);
            u = (float)(r[0] >> 8) * (1.0f / 16777216.0f);  // [0,1) like torch.rand
        }
        const float qx = target_probs[((size_t)b * (k + 1) + i) * V + x];
        const float px = draft_probs[b * dp_sb + i * dp_sk + x];
        const float rq = qx / px;
        // torch.minimum propagates NaN (0/0) and `u < NaN` is false: such a token is rejected
        const bool row_on = !active_lens || active_lens[b] > 0;
        accepted[bk] = (row_on && (rq == rq) && (u < fminf(rq, 1.0f))) ? 1 : 0;
        recovered[bk] = am.i == 0x7fffffff ? 0 : am.i;
    }
    __syncthreads();
    create_output(B, k, draft_ids, di_sb, di_sk, bonus_ids, bonus_stride, accepted, recovered, out, counters, active_lens);
    if (rng_state && threadIdx.x == 0) rng_state[1] = offset + 1;  // after every draw of this call
}

int rejection_sample(const RejectionArgs& a, hipStream_t st) {
    auto argmax_kernel = rejection_argmax_kernel<false>;
    auto output_kernel = rejection_output_kernel<false>;
    if (a.sr.seeds) {   // the SEEDED instantiations follow the presence of the seed arrays
        if (!a.sr.seeded || !a.sr.base_pos) return -1;
        argmax_kernel = rejection_argmax_kernel<true>;
        output_kernel = rejection_output_kernel<true>;
    }
    if (a.B == 0) return 0;
    if (a.k < 1) return -1;
    SmPartA* part_a = reinterpret_cast<SmPartA*>(a.ws);
    double* part_s = reinterpret_cast<double*>(reinterpret_cast<char*>(a.ws) + (size_t)a.B * a.k * QS_SM_CHUNKS * 8);
    hipLaunchKernelGGL(rejection_sum_kernel, dim3(QS_SM_CHUNKS, a.B * a.k), dim3(256), 0, st, a.target_probs, a.draft_probs, a.k,
                       a.V, a.dp_sb, a.dp_sk, part_s);
    hipLaunchKernelGGL(argmax_kernel, dim3(QS_SM_CHUNKS, a.B * a.k), dim3(256), 0, st, a.target_probs, a.draft_probs,
                       a.exponential, a.seed, a.offset, a.rng_state, a.k, a.V, a.dp_sb, a.dp_sk, part_s, part_a, a.sr);
    hipLaunchKernelGGL(output_kernel, dim3(1), dim3(1024), 0, st, a.target_probs, a.draft_probs, a.draft_ids, a.bonus_ids,
                       a.uniform, a.seed, a.offset, a.rng_state, part_a, a.B, a.k, a.V, a.dp_sb, a.dp_sk, a.di_sb, a.di_sk,
                       a.bonus_stride, a.accepted, a.recovered, a.out_tokens, a.counters, a.active_lens, a.sr);
    return 0;
}

// ---------------------------------------------------------------- typical acceptance (MEDUSA 3.3.1)
// TypicalAcceptanceSampler.forward (vllm/model_executor/layers/typical_acceptance_sampler.py:37-172), deterministic:
//   accepted[b,i]  = q[b,i,x] > min(posterior_threshold, posterior_alpha * exp(-H)),  H = -sum_v q_v log(q_v + 1e-5)
//   recovered[b,i] = argmax_v q[b,i,v]           (first index on ties, as torch.argmax)
// then the shared _create_output.  q = target_with_bonus_probs[:, :-1].  Same launch shape as the rejection sampler: each
// (b, i) row in QS_SM_CHUNKS chunks over the chip -- the entropy terms in fp32 as the reference forms them (add, log,
// multiply), summed in fp64 in chunk order and rounded once -- then one workgroup for the decision and the output.
__global__ __launch_bounds__(256) void typical_entropy_kernel(const float* __restrict__ target_probs, int k, int V,
                                                              double* __restrict__ part_s, SmPartA* __restrict__ part_a) {
    __shared__ double red_d[4];
    __shared__ ArgMax red_a[4];
    const int c = blockIdx.x, bk = blockIdx.y, b = bk / k, i = bk % k;
    int lo, hi;
    sm_chunk_range(V, c, lo, hi);
    const float* q = target_probs + ((size_t)b * (k + 1) + i) * V;
    double s = 0.0;
    ArgMax am{-__builtin_inff(), 0x7fffffff};
    for (int v = lo + threadIdx.x; v < hi; v += 256) {
        const float qv = q[v];
        s += (double)(qv * logf(qv + 1e-5f));
        if (qv > am.v) {
            am.v = qv;
            am.i = v;
        }
    }
    s = block_sum_f64(s, red_d);
    am = block_argmax(am, red_a);
    if (threadIdx.x == 0) {
        part_s[bk * QS_SM_CHUNKS + c] = s;
        part_a[bk * QS_SM_CHUNKS + c] = SmPartA{am.v, am.i};
    }
}
__global__ __launch_bounds__(1024) void typical_output_kernel(
    const float* __restrict__ target_probs, const int64_t* __restrict__ draft_ids, const int64_t* __restrict__ bonus_ids,
    float posterior_threshold, float posterior_alpha, const double* part_s, const SmPartA* part_a, int B, int k, int V,
    int64_t di_sb, int64_t di_sk, int64_t bonus_stride, uint8_t* __restrict__ accepted, int64_t* __restrict__ recovered,
    int64_t* __restrict__ out, int64_t* __restrict__ counters, const int32_t* __restrict__ active_lens) {
    for (int bk = threadIdx.x; bk < B * k; bk += blockDim.x) {
        const int b = bk / k, i = bk % k;
        double tot = 0.0;
        ArgMax am{-__builtin_inff(), 0x7fffffff};
        for (int c = 0; c < QS_SM_CHUNKS; c++) {
            tot += part_s[bk * QS_SM_CHUNKS + c];
            SmPartA pa = part_a[bk * QS_SM_CHUNKS + c];
            am = argmax_combine(am, ArgMax{pa.v, pa.i});
        }
        const float H = -(float)tot;
        const float thr = fminf(posterior_threshold, qexpf(-H) * posterior_alpha);
        const int64_t x = draft_ids[b * di_sb + i * di_sk];
        const float cand = target_probs[((size_t)b * (k + 1) + i) * V + x];
        const bool row_on = !active_lens || active_lens[b] > 0;
        accepted[bk] = (row_on && cand > thr) ? 1 : 0;
        recovered[bk] = am.i == 0x7fffffff ? 0 : am.i;
    }
    __syncthreads();
    create_output(B, k, draft_ids, di_sb, di_sk, bonus_ids, bonus_stride, accepted, recovered, out, counters, active_lens);
}
int typical_acceptance_sample(const float* target_probs, const int64_t* draft_ids, const int64_t* bonus_ids,
                              float posterior_threshold, float posterior_alpha, int B, int k, int V, int64_t di_sb,
                              int64_t di_sk, int64_t bonus_stride, int64_t* out_tokens, uint8_t* accepted, int64_t* recovered,
                              int64_t* counters, const int32_t* active_lens, void* ws, hipStream_t st) {
    if (B == 0) return 0;
    if (k < 1) return -1;
    SmPartA* part_a = reinterpret_cast<SmPartA*>(ws);
    double* part_s = reinterpret_cast<double*>(reinterpret_cast<char*>(ws) + (size_t)B * k * QS_SM_CHUNKS * 8);
    hipLaunchKernelGGL(typical_entropy_kernel, dim3(QS_SM_CHUNKS, B * k), dim3(256), 0, st, target_probs, k, V, part_s, part_a);
    hipLaunchKernelGGL(typical_output_kernel, dim3(1), dim3(1024), 0, st, target_probs, draft_ids, bonus_ids, posterior_threshold,
                       posterior_alpha, part_s, part_a, B, k, V, di_sb, di_sk, bonus_stride, accepted, recovered, out_tokens,
                       counters, active_lens);
    return 0;
}

// ---------------------------------------------------------------- Sampler.forward, the non-greedy rows
// vllm/model_executor/layers/sampler.py:216-316: l = float(logits) / temperature; _apply_top_k_top_p (:387-413: ascending
// sort; keep the top_k largest -- ties at the k-th value kept --; softmax of what is left; mask where the ASCENDING cumulative
// probability is <= 1 - top_p, never the last); probs = softmax(masked l); token = argmax(probs / Exp(1)) (_multinomial
// :585-604) or, for rows with temperature < 1e-5 (greedy requests of a mixed batch: scaled by 1.0, sampling_metadata.py:413-417),
// argmax(probs).
//
// No sort.  The logits are fp16 and l is monotonic in the logit for a positive temperature, so the ORDER of a row is the
// order of 65536 possible keys: (1) a histogram of the row's keys (integer atomics: deterministic); (2) one workgroup per row
// walks the keys in descending order -- 64 per thread, exclusive block scans of the counts and of the probability mass
// count x exp(l - max) in fp64 -- and finds the top-k key (the k-th largest value), the mass Z_k of what top-k keeps, the
// top-p key (the lowest key whose strictly-larger keys hold less than top_p x Z_k of the mass: the reference's ascending-
// cumsum rule evaluated per group of EQUAL logits -- inside such a group the reference masks whichever members its unstable
// sort happened to put first; here a boundary group stays whole, deterministic) and the final denominator; (3) an
// elementwise pass writes probs ONCE and leaves per-chunk argmax partials of probs / noise; (4) a last small launch
// combines them.  The histogram is left zeroed for the next call.
#define QS_TK_KEYS 65536
__device__ __forceinline__ uint32_t tk_key(f16 h) {   // order-preserving: larger logit -> larger key
    // -0.0 takes the key of +0.0: the two are EQUAL logits (a negative penalty produces -0.0), and a group of equal logits
    // is one key, kept or masked as a whole
    const uint16_t raw = __builtin_bit_cast(uint16_t, h);
    const uint16_t b = raw == 0x8000u ? (uint16_t)0u : raw;
    return (b & 0x8000u) ? (uint32_t)(uint16_t)~b : (uint32_t)(b | 0x8000u);
}
__device__ __forceinline__ float tk_val(uint32_t key) {   // the logit of a key
    const uint16_t b = (key & 0x8000u) ? (uint16_t)(key & 0x7FFFu) : (uint16_t)~key;
    return h2f(__builtin_bit_cast(f16, b));
}
struct TkRow {      // what pass 3 needs of a row
    uint32_t tau;   // keys >= tau are kept
    float temp;     // the divisor (1.0 for greedy rows)
    float mx;       // max l
    float z;        // float(sum of exp(l - mx) over the kept tokens)
    int greedy;
    int pad[3];
};
// One workgroup per (row, eighth of the vocabulary): a PRIVATE histogram of all 65536 keys in LDS -- 16-bit counters packed two
// to a dword (an eighth of a 128 K vocabulary cannot overflow one; larger vocabularies take more chunks) -- then only the non-zero
// counters go to the row's histogram in memory: a few thousand integer atomics per workgroup instead of one per logit (the first
// form: 38.6 us per launch at 4 rows, 79 at 16).  Integer adds: the histogram does not depend on the order.
#define QS_TK_HCHUNK 16384   // logits per workgroup (< 65536)
__global__ __launch_bounds__(1024) void topk_hist_kernel(const f16* __restrict__ logits, uint32_t* __restrict__ hist, int V) {
    extern __shared__ __attribute__((aligned(16))) uint32_t lh[];   // [32768] = 65536 16-bit counters
    const int c = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    uint4* lz = reinterpret_cast<uint4*>(lh);
#pragma unroll
    for (int i = 0; i < 8; i++) lz[tid + 1024 * i] = uint4{0u, 0u, 0u, 0u};
    __syncthreads();
    const int lo = c * QS_TK_HCHUNK, hi = min(V, lo + QS_TK_HCHUNK);
    const f16* l = logits + (size_t)t * V;
    for (int v = lo + tid; v < hi; v += 1024) {
        const f16 x = l[v];
        if (x == x) {   // (a NaN logit takes no part)
            const uint32_t key = tk_key(x);
            atomicAdd(lh + (key >> 1), (key & 1u) ? 65536u : 1u);
        }
    }
    __syncthreads();
    uint32_t* h = hist + (size_t)t * QS_TK_KEYS;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int q = tid + 1024 * i;
        const uint4 v = lz[q];
        const uint32_t w4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; e++) {
            if (w4[e] & 0xFFFFu) atomicAdd(h + 8 * q + 2 * e, w4[e] & 0xFFFFu);
            if (w4[e] >> 16) atomicAdd(h + 8 * q + 2 * e + 1, w4[e] >> 16);
        }
    }
}
// MINP (_apply_min_p, sampler.py:416-430, which runs behind top-k / top-p): a token whose probability is below min_p x the row's
// largest is masked.  p_v / p_max = exp(l_v - max) whatever the denominator and whatever top-k / top-p masked, so it is one more
// boundary in key order: the first position (descending) whose qexpf(l - max) < min_p, and everything below it.  The <false>
// instantiation is the kernel as it always was.
template <bool MINP>
__global__ __launch_bounds__(1024) void topk_select_kernel(uint32_t* __restrict__ hist, const float* __restrict__ temperature,
                                                            const int32_t* __restrict__ top_k, const float* __restrict__ top_p,
                                                            const float* __restrict__ min_p, TkRow* __restrict__ rows, int V) {
    __shared__ uint32_t s_cnt[16];
    __shared__ double s_mass[16];
    __shared__ uint32_t s_u[4];
    __shared__ double s_zk, s_z;
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t* h = hist + (size_t)t * QS_TK_KEYS;
    const float traw = temperature ? temperature[t] : 1.0f;
    const bool greedy = traw < 1e-5f;
    const float temp = greedy ? 1.0f : traw;
    int kk = top_k ? top_k[t] : -1;
    if (kk <= 0 || kk > V) kk = V;
    const double pp = top_p ? (double)top_p[t] : 1.0;
    // thread tid owns keys 65535 - 64 tid - j, j = 0 .. 63 (descending).  Its 64 counts are read ONCE, as sixteen 16-byte loads
    // of its 256 contiguous bytes, and stay in registers: every loop over them is fully unrolled (static indices; a dynamic index
    // spills them), and the three boundary searches below are walked only by the thread that holds the boundary -- the other
    // 1023 answer from their block-scan prefixes.  (Round 4: the kernel re-read the histogram five times with 4-byte loads at a
    // 256-byte lane stride: 149 us per launch, 0.6 ms of a sampled cycle.)
    const uint32_t k_hi = 65535u - 64u * tid;
    uint32_t cnt[64];
    {
        const uint4* hv = reinterpret_cast<const uint4*>(h + (k_hi - 63u));   // key k_hi - 63 + 4 q + e  <->  j = 63 - 4 q - e
#pragma unroll
        for (int q = 0; q < 16; q++) {
            const uint4 v = hv[q];
            cnt[63 - 4 * q] = v.x;
            cnt[62 - 4 * q] = v.y;
            cnt[61 - 4 * q] = v.z;
            cnt[60 - 4 * q] = v.w;
        }
    }
    uint32_t c_loc = 0, first = 0xFFFFFFFFu;
#pragma unroll
    for (int j = 0; j < 64; j++) {
        const uint32_t cj = cnt[j];
        c_loc += cj;
        if (cj && first == 0xFFFFFFFFu) first = 64u * tid + j;   // descending position of this thread's largest key
    }
    // the row maximum = the first non-empty key in descending order
    uint32_t fm = first;
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) fm = min(fm, (uint32_t)__shfl_xor((int)fm, m, 64));
    if (lane == 0) s_cnt[wave] = fm;
    __syncthreads();
    uint32_t pos_max = s_cnt[0];
    for (int w2 = 1; w2 < 16; w2++) pos_max = min(pos_max, s_cnt[w2]);
    __syncthreads();
    const float mx = pos_max == 0xFFFFFFFFu ? 0.0f : tk_val(65535u - pos_max) / temp;
    auto wgt = [&](int j) -> double { return (double)cnt[j] * (double)qexpf(tk_val(k_hi - j) / temp - mx); };
    double m_loc = 0.0;
    if (c_loc) {
#pragma unroll
        for (int j = 0; j < 64; j++)
            if (cnt[j]) m_loc += wgt(j);
    }
    // exclusive block scans (thread order = descending keys): counts and mass
    uint32_t c_inc = c_loc;
    double m_inc = m_loc;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t oc = (uint32_t)__shfl_up((int)c_inc, d, 64);
        const double om = __shfl_up(m_inc, d, 64);
        if (lane >= d) {
            c_inc += oc;
            m_inc += om;
        }
    }
    if (lane == 63) {
        s_cnt[wave] = c_inc;
        s_mass[wave] = m_inc;
    }
    __syncthreads();
    uint32_t c_ex = c_inc - c_loc;
    double m_ex = m_inc - m_loc;
    for (int w2 = 0; w2 < wave; w2++) {
        c_ex += s_cnt[w2];
        m_ex += s_mass[w2];
    }
    if (tid == 0) {
        s_u[0] = 0xFFFFFFFFu;   // descending position of the top-k key
        s_u[1] = 0xFFFFFFFFu;   // descending position of the first key top-p masks
        s_u[2] = 0xFFFFFFFFu;   // descending position of the first key min_p masks
    }
    __syncthreads();
    // (a) top-k: the key at which the descending cumulative count reaches k; Z_k = the mass down to and including it.
    // Exactly one thread's count range (c_ex, c_ex + c_loc] contains k: it walks its keys.
    if (c_ex < (uint32_t)kk && c_ex + c_loc >= (uint32_t)kk) {
        uint32_t run = c_ex;
        double mrun = m_ex;
#pragma unroll
        for (int j = 0; j < 64; j++) {
            const uint32_t cj = cnt[j];
            if (cj) {
                const double w = wgt(j);
                if (run < (uint32_t)kk && run + cj >= (uint32_t)kk) {
                    s_u[0] = 64u * tid + j;
                    s_zk = mrun + w;
                }
                run += cj;
                mrun += w;
            }
        }
    }
    if (tid == 1023 && c_ex + c_loc < (uint32_t)kk) {   // fewer than k finite logits: everything is kept
        s_u[0] = 65535u;
        s_zk = m_ex + m_loc;
    }
    __syncthreads();
    const uint32_t pos_k = s_u[0];
    const double zk = s_zk;
    // (b) top-p: the first key (descending) whose strictly-larger keys already hold >= p Z_k of the mass is masked, and
    // everything below it; a group of equal logits is kept or masked as a whole.  The mass above a key never decreases along
    // the positions, so the answer lies in the thread where it crosses p Z_k -- or, if it crosses behind that thread's last
    // key, it is the first key of a later thread: those offer theirs without a walk, the smallest position wins.
    // top_p >= 1 (the default) masks nothing and is not searched: with thr = Z_k the groups whose weight is below half an ulp
    // of the fp64 mass above them (~37 nats under the maximum) would satisfy mass_above >= thr and be masked, tokens whose
    // fp32 probability is not 0 -- the reference's `cumsum <= 1 - p` masks none of them
    if (pp < 1.0) {
        const double thr = pp * zk;
        uint32_t best = 0xFFFFFFFFu;
        if (c_loc && m_ex + m_loc >= thr && 64u * tid <= pos_k) {
            if (m_ex >= thr && first != pos_max) {
                if (first <= pos_k) best = first;
            } else {
                double mrun = m_ex;
#pragma unroll
                for (int j = 0; j < 64; j++) {
                    const uint32_t cj = cnt[j];
                    if (cj) {
                        const uint32_t pos = 64u * tid + j;
                        if (best == 0xFFFFFFFFu && pos <= pos_k && pos != pos_max && mrun >= thr) best = pos;
                        mrun += wgt(j);
                    }
                }
            }
        }
        if (best != 0xFFFFFFFFu) atomicMin(&s_u[1], best);
    }
    if (MINP) {
        // (b') min_p: every thread offers its first non-empty key with qexpf(l - max) < min_p (the row maximum has 1.0 and
        // min_p <= 1: it is never masked); greedy rows have none (SamplingParams resets min_p for them, sampling_params.py:344)
        const float mp = (min_p && !greedy) ? min_p[t] : 0.0f;
        if (mp > 0.0f && c_loc) {
            uint32_t best = 0xFFFFFFFFu;
#pragma unroll
            for (int j = 0; j < 64; j++)
                if (cnt[j] && best == 0xFFFFFFFFu && 64u * tid + j != pos_max && qexpf(tk_val(k_hi - j) / temp - mx) < mp)
                    best = 64u * tid + j;
            if (best != 0xFFFFFFFFu) atomicMin(&s_u[2], best);
        }
    }
    __syncthreads();
    const uint32_t pos_p = s_u[1];                                       // first masked position, or none
    uint32_t pos_last = pos_p == 0xFFFFFFFFu ? pos_k : min(pos_k, pos_p - 1);   // last kept position (descending)
    if (MINP && s_u[2] != 0xFFFFFFFFu) pos_last = min(pos_last, s_u[2] - 1);
    // (c) the final denominator: the mass of positions <= pos_last (pos_last itself may be an empty key: the position just
    // above the first masked one); the thread whose 64 positions contain pos_last walks and publishes it
    if ((pos_last >> 6) == (uint32_t)tid) {
        double mrun = m_ex;
#pragma unroll
        for (int j = 0; j < 64; j++)
            if (cnt[j] && 64u * tid + j <= pos_last) mrun += wgt(j);
        s_z = mrun;
    }
    if (c_loc) {   // leave the histogram zeroed for the next call
        uint4* hz = reinterpret_cast<uint4*>(h + (k_hi - 63u));
#pragma unroll
        for (int q = 0; q < 16; q++) hz[q] = uint4{0u, 0u, 0u, 0u};
    }
    __syncthreads();
    if (tid == 0) {
        TkRow r;
        r.tau = 65535u - pos_last;
        // (between pos_last and the next non-empty key nothing lives, so "key >= tau" keeps exactly positions <= pos_last)
        r.temp = temp;
        r.mx = mx;
        r.z = (float)s_z;
        r.greedy = greedy ? 1 : 0;
        r.pad[0] = r.pad[1] = r.pad[2] = 0;
        rows[t] = r;
    }
}
// SEEDED: row t of a seeded sequence t / rows_per_seq draws from its own key (sr.stream, j = j_base + t % rows_per_seq)
template <bool SEEDED>
__global__ __launch_bounds__(256) void topk_write_kernel(const f16* __restrict__ logits, const TkRow* __restrict__ rows,
                                                         const float* __restrict__ exponential, uint64_t seed, uint64_t offset,
                                                         const uint64_t* __restrict__ rng_state, float* __restrict__ probs,
                                                         SmPartA* __restrict__ part_a, int V, SeedRows sr) {
    __shared__ ArgMax red_a[4];
    const int c = blockIdx.x, t = blockIdx.y;
    int lo, hi;
    sm_chunk_range(V, c, lo, hi);
    const TkRow r = rows[t];
    if (rng_state) {
        seed = rng_state[0];
        offset = rng_state[1];
    }
    PhiloxKey pk = engine_key(seed, offset, 0x40000000u | (uint32_t)t);
    if (SEEDED) pk = seeded_key(sr, t / sr.rows_per_seq, sr.stream, sr.j_base + t % sr.rows_per_seq, pk);
    const f16* l = logits + (size_t)t * V;
    float* p = probs + (size_t)t * V;
    ArgMax am{-__builtin_inff(), 0x7fffffff};
    for (int v = lo + threadIdx.x; v < hi; v += 256) {
        const f16 x = l[v];
        float pv = 0.0f;
        if (x == x && tk_key(x) >= r.tau) pv = qexpf(h2f(x) / r.temp - r.mx) / r.z;
        p[v] = pv;
        float val = pv;
        if (!r.greedy) {
            float e;
            if (exponential) {
                e = exponential[(size_t)t * V + v];
            } else {
                uint32_t rr[4];
                philox4x32((uint32_t)v, pk.c1, pk.c2, pk.c3, pk.k0, pk.k1, rr);
                e = -__logf(u01_open(rr[0]));
            }
            val = pv / e;
        }
        if (val > am.v) {
            am.v = val;
            am.i = v;
        }
    }
    am = block_argmax(am, red_a);
    if (threadIdx.x == 0) part_a[t * QS_SM_CHUNKS + c] = SmPartA{am.v, am.i};
}
__global__ __launch_bounds__(256) void topk_token_kernel(const SmPartA* __restrict__ part_a, int64_t* __restrict__ token,
                                                         int64_t token_stride, uint64_t* __restrict__ rng_state, int T) {
    for (int t = threadIdx.x; t < T; t += 256) {
        const ArgMax am = sm_row_max(part_a, t);
        token[t * token_stride] = am.i == 0x7fffffff ? 0 : am.i;
    }
    if (rng_state && threadIdx.x == 0) rng_state[1] = rng_state[1] + 1;   // after every draw of this call
}
// ws: [rows][65536] u32 histogram (zero-filled ONCE by the caller, left zeroed by every call) | [rows] TkRow | [rows][CHUNKS] SmPartA
size_t sample_ws_bytes(int rows) {
    return (size_t)rows * QS_TK_KEYS * 4 + (size_t)rows * sizeof(TkRow) + (size_t)rows * QS_SM_CHUNKS * sizeof(SmPartA);
}
static bool g_tk_hist_attr = false;   // topk_hist_kernel's LDS attribute is set
int sample_top_k_top_p(const SampleArgs& a, hipStream_t st) {
    // the instantiations follow the presence of the optional parts: MINP of a.min_p, SEEDED of the seed arrays
    const auto select_kernel = a.min_p ? topk_select_kernel<true> : topk_select_kernel<false>;
    auto write_kernel = topk_write_kernel<false>;
    const SeedRows& sr = a.sr;
    if (sr.seeds) {
        if (!sr.seeded || !sr.base_pos || sr.rows_per_seq < 1 || (int64_t)a.nseq * sr.rows_per_seq < a.T || sr.j_base < 0 ||
            sr.j_base + sr.rows_per_seq > 65536 || sr.stream < 1 || sr.stream > 0x7FFF)
            return -1;
        write_kernel = topk_write_kernel<true>;
    }
    const int T = a.T, V = a.V;
    if (T == 0) return 0;
    uint32_t* hist = reinterpret_cast<uint32_t*>(a.ws);
    TkRow* rows = reinterpret_cast<TkRow*>(reinterpret_cast<char*>(a.ws) + (size_t)T * QS_TK_KEYS * 4);
    SmPartA* part_a = reinterpret_cast<SmPartA*>(reinterpret_cast<char*>(rows) + (size_t)T * sizeof(TkRow));
    if (!g_tk_hist_attr) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(topk_hist_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                QS_TK_KEYS * 2) != hipSuccess)
            return -8;
        g_tk_hist_attr = true;
    }
    hipLaunchKernelGGL(topk_hist_kernel, dim3((V + QS_TK_HCHUNK - 1) / QS_TK_HCHUNK, T), dim3(1024), QS_TK_KEYS * 2, st, a.logits, hist, V);
    hipLaunchKernelGGL(select_kernel, dim3(T), dim3(1024), 0, st, hist, a.temperature, a.top_k, a.top_p, a.min_p, rows, V);
    hipLaunchKernelGGL(write_kernel, dim3(QS_SM_CHUNKS, T), dim3(256), 0, st, a.logits, rows, a.exponential, a.seed, a.offset,
                       a.rng_state, a.probs, part_a, V, sr);
    hipLaunchKernelGGL(topk_token_kernel, dim3(1), dim3(256), 0, st, part_a, a.token, a.token_stride, a.rng_state, T);
    return 0;
}

// ---------------------------------------------------------------- logit processors
// Sampler.forward's steps in front of the temperature (vllm/model_executor/layers/sampler.py:258-266): _apply_min_tokens_penalty
// (:338-384) and apply_penalties (vllm/model_executor/layers/utils.py:24-57), per ROW of a speculative cycle: row j of a sequence
// is processed exactly as the non-speculative sampler would process that position given the same prefix -- prompt tokens, the
// outputs committed before the cycle, the in-flight draft tokens d_1 .. d_j, generated length = committed + j.
//
// tok_table[slot][V], one u32 per (slot, token): bit 31 = the token occurs in the prompt, low 31 bits = how often it occurs in
// the outputs counted so far.  counted_len[slot] = how many of the slot's committed tokens gen_tokens[slot][0 .. gen_lens) are in
// the table (outputs a re-admitted request had before its admission are counted by logit_table_set_prompt and live in the table
// only).
// INVARIANT: catch-up is driven by gen_lens alone -- it adds gen_tokens[slot][counted_len .. gen_len) and sets counted_len =
// gen_len -- so it is idempotent, and a cycle re-run by recover() needs no rollback: the failed cycle's catch-up left counted_len
// = gen_len at the START of that cycle, spec_snapshot(restore) brings gen_lens back to exactly that value, and the re-run's
// catch-up finds nothing to add.  (The tokens the failed cycle committed were never counted: counting happens at the head of the
// NEXT cycle.)
#define QS_LP_MAX_STOP 16      // QS_MAX_STOP_IDS of include/qspec_hip.h
#define QS_LP_MAX_INFLIGHT 64  // in-flight draft tokens a row can see (j_base + rows_per_seq - 1)
#define QS_LP_CHUNK 2048       // logits per workgroup: 256 threads x 8
__global__ __launch_bounds__(1024) void logit_table_set_prompt_kernel(uint32_t* __restrict__ row, int V,
                                                                       const int64_t* __restrict__ prompt, int n_prompt,
                                                                       const int64_t* __restrict__ outputs, int n_out,
                                                                       int32_t* __restrict__ counted_len) {
    // ONE workgroup: clear the row, then mark / count (integer atomics: the result does not depend on the order)
    for (int v = threadIdx.x; v < V; v += blockDim.x) row[v] = 0u;
    __syncthreads();
    for (int i = threadIdx.x; i < n_prompt; i += blockDim.x) {
        const int64_t t = prompt[i];
        if (t >= 0 && t < V) atomicOr(row + t, 0x80000000u);
    }
    for (int i = threadIdx.x; i < n_out; i += blockDim.x) {
        const int64_t t = outputs[i];
        if (t >= 0 && t < V) atomicAdd(row + t, 1u);
    }
    if (threadIdx.x == 0) *counted_len = 0;
}
int logit_table_set_prompt(uint32_t* table, int V, int slot, const int64_t* prompt, int n_prompt, const int64_t* outputs,
                           int n_out, int32_t* counted_len, hipStream_t st) {
    hipLaunchKernelGGL(logit_table_set_prompt_kernel, dim3(1), dim3(1024), 0, st, table + (size_t)slot * V, V, prompt, n_prompt,
                       outputs, n_out, counted_len + slot);
    return 0;
}
// One thread per slot walks its new tokens in order (k + 1 at most in the steady state): plain loads and stores, no atomics,
// deterministic.  need[slot] == 0: the slot keeps no counts (its penalties are neutral) and is left alone.
__global__ void logit_table_catch_up_kernel(int B, int V, uint32_t* __restrict__ table, int32_t* __restrict__ counted_len,
                                            const int32_t* __restrict__ need, const int64_t* __restrict__ gen_tokens, int gen_cap,
                                            const int32_t* __restrict__ gen_lens) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B || !need[b]) return;
    const int hi = min(gen_lens[b], gen_cap);
    int lo = counted_len[b];
    if (lo < 0) lo = 0;
    if (hi <= lo) return;   // nothing new (or gen_lens went back: a freed slot; admission rebuilds the row)
    uint32_t* row = table + (size_t)b * V;
    for (int i = lo; i < hi; i++) {
        const int64_t t = gen_tokens[(size_t)b * gen_cap + i];
        if (t >= 0 && t < V) row[t] = row[t] + 1u;
    }
    counted_len[b] = hi;
}
int logit_table_catch_up(int B, int V, uint32_t* table, int32_t* counted_len, const int32_t* need, const int64_t* gen_tokens,
                         int gen_cap, const int32_t* gen_lens, hipStream_t st) {
    if (B == 0) return 0;
    hipLaunchKernelGGL(logit_table_catch_up_kernel, dim3((B + 63) / 64), dim3(64), 0, st, B, V, table, counted_len, need,
                       gen_tokens, gen_cap, gen_lens);
    return 0;
}
// One element, the reference's steps in the reference's order with the reference's roundings (every fp16 op of torch is the
// fp32 op on the fp16 operands rounded to fp16; f2h keeps hipcc from folding two roundings into one):
//   min_tokens: stop ids -> -inf;  repetition: x > 0 ? x / r : x * r where the token is in prompt or outputs (x <= 0 is evaluated
//   AFTER the division, as the reference's second masked assignment is; NaN takes neither);  x -= f * fp16(count);
//   x -= p * (count > 0) -- the products are formed even where the count is 0: a negative penalty gives -0.0 there and
//   (-0.0) - (-0.0) = +0.0, as in the reference.
struct LpRow {
    f16 rep, freq, pres;
    bool table, stop;     // the slot keeps counts / the row masks its stop ids
    int n_inflight, n_stop;
};
__device__ __forceinline__ f16 lp_element(f16 x, int v, uint32_t w, const LpRow& r, const int64_t* s_inflight, const int32_t* s_stop) {
    if (r.stop) {
        for (int i = 0; i < r.n_stop; i++)
            if (s_stop[i] == v) x = f2h(-__builtin_inff());
    }
    if (!r.table) return x;
    uint32_t cnt = w & 0x7FFFFFFFu;
    for (int i = 0; i < r.n_inflight; i++) cnt += (s_inflight[i] == (int64_t)v) ? 1u : 0u;
    const bool seen = (w >> 31) || cnt > 0u;
    if (seen) {
        const float rr = h2f(r.rep);
        if (h2f(x) > 0.0f) x = f2h(h2f(x) / rr);
        if (h2f(x) <= 0.0f) x = f2h(h2f(x) * rr);
    }
    const f16 cnt_h = f2h((float)cnt);
    x = f2h(h2f(x) - h2f(f2h(h2f(r.freq) * h2f(cnt_h))));
    x = f2h(h2f(x) - h2f(f2h(h2f(r.pres) * (cnt > 0u ? 1.0f : 0.0f))));
    return x;
}
// LpArgs (kernels.h): the launch arguments of the pass
// Token constraints (logit_bias, allowed_token_ids, bad words): the reference's engine lowers them to logits processors
// (vllm/engine/llm_engine.py:1950-2009; vllm/entrypoints/openai/logits_processors.py:10-50; vllm/logits_process.py:48-119) that
// run on the fp16 row in front of Sampler.forward (vllm/model_executor/layers/logits_processor.py:134-170).  Per-slot state:
//   deny [nslots, deny_words] u32: bit v = token v is outside allowed_token_ids or is a single-token bad word;
//   meta [nslots, 4] i32: flags (bit 0: the deny row is in use, bit 1: the request has bad words), number of biases, number of
//     multi-token bad words, length of the tail;
//   bias_ids / bias_vals [nslots, 512]: logit_bias, sorted by id;  words [nslots, 32, 8] / word_lens [nslots, 32];
//   tail [nslots, 7] i32, right-aligned: the last outputs the request had BEFORE its admission (gen_tokens starts empty then).
#define QS_TC_MAX_BIAS 512     // QS_MAX_LOGIT_BIAS of include/qspec_hip.h
#define QS_TC_MAX_WORDS 32     // QS_MAX_BAD_WORDS
#define QS_TC_WORD_LEN 8       // QS_MAX_BAD_WORD_LEN
// LpCons, LpArgsC (kernels.h): that per-slot state, behind the arguments of the plain pass
template <bool C, bool G = false> struct LpArgsOf { typedef LpArgs type; };
template <> struct LpArgsOf<true, false> { typedef LpArgsC type; };
template <> struct LpArgsOf<true, true> { typedef LpArgsG type; };
// Token guides (guided decoding): the reference's engine lowers guided_decoding (regex, JSON schema, choice) to an Outlines
// processor at index 0 of logits_processors (vllm/engine/llm_engine.py:1950-2009) whose call
// (vllm/model_executor/guided_decoding/outlines_logits_processors.py:34-93) advances a finite automaton over the sequence's OUTPUT
// tokens and adds an fp32 mask, 0 at the state's allowed ids and -inf elsewhere, to the fp16 row.  Here the automaton lives on
// the device, because row j's state depends on the in-flight draft tokens d_1 .. d_j.  The guide arena, per resident state s:
//   allow [states, words] u32: bit v = token v is allowed in s (the geometry of deny; words a multiple of 4);
//   rank  [states, words] i32: the exclusive prefix popcount of the allow row, per word;
//   off   [states] i32 and nxt[] i32: the next states of s's allowed tokens, ascending by token, start at nxt[off[s]];
//   next(s, t) = allow[s][t >> 5] bit (t & 31) ? nxt[off[s] + rank[s][t >> 5] + popc(allow[s][t >> 5] & ((1 << (t & 31)) - 1))] : miss
// -- two dependent round trips per token (allow, rank and off are independent loads), no search, no dense [S, V] table.  States
// are arena rows: a guide's states are contiguous and its nxt entries are stored as arena rows, so a walk needs no base.
//   gslot [nslots, 4] i32: {state after the outputs counted so far, g_len, the guide's miss state, 1 = the slot is guided}.
// INVARIANT (the twin of counted_len's above): catch-up is driven by gen_lens alone -- it advances state over
// gen_tokens[slot][g_len .. gen_len) and sets g_len = gen_len -- so it is idempotent, and a cycle re-run by recover() needs no
// rollback: spec_snapshot(restore) brings gen_lens back to g_len and the re-run's catch-up finds nothing to walk.  Outputs a
// re-admitted request had before its admission are walked on the host at admission (g_len = 0 then).
__device__ __forceinline__ int guide_next(const LpGuide& g, int V, int s, int64_t t, int miss) {
    if (t < 0 || t >= V || s < 0 || s >= g.n_states) return miss;
    const size_t wi = (size_t)s * g.words + (size_t)(t >> 5);
    const uint32_t aw = g.allow[wi];      // first round trip: three independent loads
    const int r = g.rank[wi];
    const int o = g.off[s];
    const uint32_t bit = 1u << (t & 31);
    if (!(aw & bit)) return miss;
    const int i = o + r + __builtin_popcount(aw & (bit - 1u));
    if (i < 0 || i >= g.n_trans) return miss;
    return g.nxt[i];                      // second round trip
}
template <bool G> __device__ __forceinline__ int* guide_state_word() {   // (LDS of the guided instantiation alone)
    __shared__ int s_gstate;
    return &s_gstate;
}
// grid (chunks of 2048 logits, rows): 16-byte loads of the logits and of the table words, 16-byte stores; a row is wave-uniform
// in everything but the element itself.  About 8 B of traffic per element (2 + 4 read, 2 written).
// C (token constraints, in front of the pipeline above): x[id] = fp16(x[id] + bias); deny bits and matched multi-token bad words
// -> -inf; a request with bad words adds the reference's fp32 zero to every element (-0.0 becomes +0.0).  All -inf assignments
// commute with a finite bias, so the order among them is free; all of them land before lp_element, whose repetition rule looks
// at the sign.  One byte of the deny row covers a thread's 8 logits.  Biases and banned last tokens that fall into the
// workgroup's chunk are applied to the chunk staged in LDS (no workgroup stages anything when none does: __syncthreads_or).
// Every workgroup of a row resolves the bad-word matches itself: threads 0..6 fetch the row's last 7 tokens (in-flight, then
// committed, then the pre-admission tail), threads 0..31 compare one word each.  Nothing is written but `out`.
// G (token guides, in front of C; its own instantiation: <false> and <true> are the kernels they were): a guided row's workgroup
// resolves its state itself -- one lane of the second wave walks the row's j in-flight tokens from gslot[slot].state (at most
// QS_LP_MAX_INFLIGHT steps of two round trips, issued behind the element loads, so they overlap) and broadcasts it through LDS;
// then every thread reads one byte of allow[state] beside its deny byte: deny |= ~allow.  Every element of a guided row gets
// the fp32 zero the reference's scores.add_(mask) adds at allowed ids (-0.0 becomes +0.0), on the element as loaded.  The
// reference's order is guide, bias, allowed, bad words: the zero is added in front of the bias as there, and the guide's -inf
// assignments commute with a finite bias like the others, so they land with the deny bits.  Rows of unguided slots get the bits
// of the <true> instantiation.
template <bool C, bool G = false>
__global__ __launch_bounds__(256) void process_logits_kernel(typename LpArgsOf<C, G>::type a) {
    __shared__ int64_t s_inflight[QS_LP_MAX_INFLIGHT];
    __shared__ int32_t s_stop[QS_LP_MAX_STOP];
    const int t = blockIdx.y, seq = t / a.rows_per_seq, j = a.j_base + t % a.rows_per_seq;
    int slot = a.slot_ids ? a.slot_ids[seq] : seq;
    const bool slot_ok = slot >= 0 && slot < a.nslots;   // (a row outside the slot arrays is copied through)
    if (!slot_ok) slot = 0;
    const int V = a.V;
    const f16* l = a.logits + (size_t)t * V;
    f16* o = a.out + (size_t)t * V;
    LpRow r;
    r.rep = a.rep[slot]; r.freq = a.freq[slot]; r.pres = a.pres[slot];
    const bool on = slot_ok && (!a.active_lens || a.active_lens[slot] > 0);
    r.table = on && !(h2f(r.rep) == 1.0f && h2f(r.freq) == 0.0f && h2f(r.pres) == 0.0f);
    r.n_stop = min(max(a.n_stop[slot], 0), a.stop_width);
    r.stop = on && r.n_stop > 0 && a.gen_base[slot] + a.gen_lens[slot] + j < a.min_tokens[slot];
    r.n_inflight = (r.table && a.draft_ids) ? min(j, QS_LP_MAX_INFLIGHT) : 0;
    if ((int)threadIdx.x < r.n_inflight) s_inflight[threadIdx.x] = a.draft_ids[slot * a.di_sb + threadIdx.x * a.di_sk];
    if ((int)threadIdx.x < r.n_stop) s_stop[threadIdx.x] = a.stop_ids[slot * a.stop_width + threadIdx.x];
    const int lo = blockIdx.x * QS_LP_CHUNK, v0 = lo + 8 * (int)threadIdx.x;
    if constexpr (C) {
        __shared__ int64_t s_last[QS_TC_WORD_LEN - 1];   // s_last[p - 1]: the p-th token from the end of outputs + in-flight
        __shared__ f16 s_x[QS_LP_CHUNK];
        const int tid = threadIdx.x;
        const int4 meta = *reinterpret_cast<const int4*>(a.c.meta + 4 * slot);
        const bool deny_on = on && (meta.x & 1);
        const bool zero_add = on && (meta.x & 2);
        int4 gs = int4{0, 0, 0, 0};
        if constexpr (G) gs = *reinterpret_cast<const int4*>(a.g.gslot + 4 * slot);
        const bool guided = G && on && gs.w != 0;
        const int n_bias = on ? min(max(meta.y, 0), QS_TC_MAX_BIAS) : 0;
        const int n_words = on ? min(max(meta.z, 0), QS_TC_MAX_WORDS) : 0;
        const bool vec = V % 8 == 0;
        // the element loads first: everything below overlaps them
        f16x8 x = f16x8{0, 0, 0, 0, 0, 0, 0, 0};
        u32x4 w0 = u32x4{0u, 0u, 0u, 0u}, w1 = w0;
        const uint32_t* w = a.table + (size_t)slot * V;
        uint32_t deny = 0u;
        if (v0 < V) {
            if (vec) {
                x = *reinterpret_cast<const f16x8*>(l + v0);
                if (r.table) {
                    w0 = *reinterpret_cast<const u32x4*>(w + v0);
                    w1 = *reinterpret_cast<const u32x4*>(w + v0 + 4);
                }
            } else {
                for (int e = 0; e < 8; e++)
                    if (v0 + e < V) {
                        x[e] = l[v0 + e];
                        const uint32_t we = r.table ? w[v0 + e] : 0u;
                        if (e < 4) w0[e] = we; else w1[e - 4] = we;
                    }
            }
            deny = reinterpret_cast<const uint8_t*>(a.c.deny + (size_t)slot * a.c.deny_words)[v0 >> 3];
        }
        if (!deny_on) deny = 0u;
        if constexpr (G) {   // the row's state: gslot's, advanced over the in-flight tokens d_1 .. d_j
            if (guided && tid == 64) {
                int s = gs.x;
                const int n = a.draft_ids ? min(j, QS_LP_MAX_INFLIGHT) : 0;
                for (int i = 0; i < n; i++) s = guide_next(a.g, V, s, a.draft_ids[slot * a.di_sb + i * a.di_sk], gs.z);
                *guide_state_word<G>() = min(max(s, 0), a.g.n_states - 1);
            }
        }
        // logit_bias entries of this thread (two at most) that fall into the chunk
        int bid[2]; float bval[2];
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const int i = tid + 256 * e;
            bid[e] = i < n_bias ? a.c.bias_ids[slot * QS_TC_MAX_BIAS + i] - lo : -1;
            bval[e] = i < n_bias ? a.c.bias_vals[slot * QS_TC_MAX_BIAS + i] : 0.0f;
            if (bid[e] < 0 || bid[e] >= QS_LP_CHUNK || bid[e] + lo >= V) bid[e] = -1;
        }
        // multi-token bad words: the last 7 tokens of the row's prefix, then one word per thread
        if (n_words > 0 && tid < QS_TC_WORD_LEN - 1) {
            const int p = tid + 1;
            int64_t tok = -1;
            const int gl = min(max(a.gen_lens[slot], 0), a.c.gen_cap);
            const int tl = min(max(meta.w, 0), QS_TC_WORD_LEN - 1);
            if (p <= j) {
                if (a.draft_ids) tok = a.draft_ids[slot * a.di_sb + (int64_t)(j - p) * a.di_sk];
            } else if (p - j <= gl) {
                tok = a.c.gen_tokens[(size_t)slot * a.c.gen_cap + (gl - (p - j))];
            } else if (p - j - gl <= tl) {
                tok = a.c.tail[slot * (QS_TC_WORD_LEN - 1) + (QS_TC_WORD_LEN - 1) - (p - j - gl)];
            }
            s_last[tid] = tok;
        }
        int4 wa = int4{-1, -1, -1, -1}, wb = wa;
        int wl = 0;
        if (tid < n_words) {
            const int32_t* wp = a.c.words + ((size_t)slot * QS_TC_MAX_WORDS + tid) * QS_TC_WORD_LEN;
            wa = *reinterpret_cast<const int4*>(wp);
            wb = *reinterpret_cast<const int4*>(wp + 4);
            wl = min(max(a.c.word_lens[slot * QS_TC_MAX_WORDS + tid], 2), QS_TC_WORD_LEN);
        }
        __syncthreads();
        if constexpr (G) {
            if (guided && v0 < V) {
                const uint32_t* arow = a.g.allow + (size_t)(*guide_state_word<G>()) * a.g.words;
                deny |= ~(uint32_t)reinterpret_cast<const uint8_t*>(arow)[v0 >> 3] & 0xFFu;
            }
            if (guided) {   // the mask's zeros, on the element as loaded: in front of the bias, as the reference orders them
#pragma unroll
                for (int e = 0; e < 8; e++) x[e] = f2h(h2f(x[e]) + 0.0f);
            }
        }
        int ban = -1;
        if (tid < n_words) {
            const int ws[QS_TC_WORD_LEN] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
            bool match = true;
            int last = -1;
#pragma unroll
            for (int i = 0; i < QS_TC_WORD_LEN; i++) {
                if (i < wl - 1) match = match && (int64_t)ws[i] == s_last[wl - 2 - i];
                if (i == wl - 1) last = ws[i];
            }
            if (match && last >= lo && last < lo + QS_LP_CHUNK && last < V) ban = last - lo;
        }
        bool staged = false;
        if (n_bias > 0 || n_words > 0) staged = __syncthreads_or(bid[0] >= 0 || bid[1] >= 0 || ban >= 0);
        if (staged) {   // (workgroup-uniform)
            *reinterpret_cast<f16x8*>(s_x + 8 * tid) = x;
            __syncthreads();
#pragma unroll
            for (int e = 0; e < 2; e++)   // ids are distinct: one writer per element
                if (bid[e] >= 0) s_x[bid[e]] = f2h(h2f(s_x[bid[e]]) + bval[e]);
            __syncthreads();
            if (ban >= 0) s_x[ban] = f2h(-__builtin_inff());   // (two words may ban the same token: the same value)
            __syncthreads();
            x = *reinterpret_cast<const f16x8*>(s_x + 8 * tid);
        }
        if (v0 >= V) return;
        const bool lp = r.table || r.stop;
#pragma unroll
        for (int e = 0; e < 8; e++) {
            f16 xe = x[e];
            if ((deny >> e) & 1u) xe = f2h(-__builtin_inff());
            if (zero_add) xe = f2h(h2f(xe) + 0.0f);
            if (lp) xe = lp_element(xe, v0 + e, e < 4 ? w0[e] : w1[e - 4], r, s_inflight, s_stop);
            x[e] = xe;
        }
        if (vec) {
            *reinterpret_cast<f16x8*>(o + v0) = x;
        } else {
            for (int e = 0; e < 8; e++)
                if (v0 + e < V) o[v0 + e] = x[e];
        }
        return;
    }
    __syncthreads();
    const uint32_t* w = a.table + (size_t)slot * V;
    if (v0 >= V) return;
    if (V % 8 == 0) {   // rows are 16-byte aligned: one f16x8 per thread (v0 + 8 <= V follows from V % 8 == 0)
        f16x8 x = *reinterpret_cast<const f16x8*>(l + v0);
        if (r.table || r.stop) {
            u32x4 w0 = u32x4{0u, 0u, 0u, 0u}, w1 = w0;
            if (r.table) {
                w0 = *reinterpret_cast<const u32x4*>(w + v0);
                w1 = *reinterpret_cast<const u32x4*>(w + v0 + 4);
            }
#pragma unroll
            for (int e = 0; e < 8; e++) x[e] = lp_element(x[e], v0 + e, e < 4 ? w0[e] : w1[e - 4], r, s_inflight, s_stop);
        }
        *reinterpret_cast<f16x8*>(o + v0) = x;
    } else {
        const int hi = min(V, v0 + 8);
        for (int v = v0; v < hi; v++) {
            f16 x = l[v];
            if (r.table || r.stop) x = lp_element(x, v, r.table ? w[v] : 0u, r, s_inflight, s_stop);
            o[v] = x;
        }
    }
}
// the kernel instantiation follows the presence of a.c.deny (<C>) and of a.g.allow (<C, G>)
int process_logits(const LpArgsG& a, int T, hipStream_t st) {
    if (T == 0) return 0;
    if (a.stop_width < 0 || a.stop_width > QS_LP_MAX_STOP || a.nslots < 1 || a.rows_per_seq < 1 || a.j_base < 0 ||
        a.j_base + a.rows_per_seq - 1 > QS_LP_MAX_INFLIGHT)
        return -1;
    const dim3 grid((a.V + QS_LP_CHUNK - 1) / QS_LP_CHUNK, T);
    if (!a.c.deny) {
        hipLaunchKernelGGL(process_logits_kernel<false>, grid, dim3(256), 0, st, static_cast<const LpArgs&>(a));
        return 0;
    }
    if (a.c.gen_cap < 1 || (int64_t)a.c.deny_words * 32 < a.V) return -1;
    if (!a.g.allow) {
        hipLaunchKernelGGL(process_logits_kernel<true>, grid, dim3(256), 0, st, static_cast<const LpArgsC&>(a));
        return 0;
    }
    if (a.g.words % 4 || (int64_t)a.g.words * 32 < a.V || a.g.n_states < 1 || a.g.n_trans < 1) return -1;
    hipLaunchKernelGGL((process_logits_kernel<true, true>), grid, dim3(256), 0, st, a);
    return 0;
}
// Admission (outside the graph): one workgroup per state of a guide's CSR (row_ptr [n_states + 1], tokens ascending and distinct
// per state, next states; validated by the host).  The allow row is assembled in LDS with LDS bit-sets and written with 16-byte
// stores; a workgroup scan of the word popcounts gives the rank row; the state's transitions go to nxt[trans_base + ...] as arena
// rows (state_base + next).  Rows are row_stride words apart (>= words, a multiple of 4); only `words` of each are written.
#define QS_GUIDE_MAX_WORDS 8192   // 32 KB of LDS: vocabularies up to 262144
__global__ __launch_bounds__(256) void guide_build_kernel(uint32_t* __restrict__ allow, int32_t* __restrict__ rank,
                                                          int32_t* __restrict__ off, int32_t* __restrict__ nxt, int words,
                                                          int row_stride, int V, int state_base, int trans_base, int n_trans,
                                                          const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ tokens,
                                                          const int32_t* __restrict__ next) {
    extern __shared__ uint32_t s_row[];
    __shared__ int s_sum[256];
    const int s = blockIdx.x, tid = threadIdx.x;
    for (int i = tid; i < words; i += 256) s_row[i] = 0u;
    __syncthreads();
    const int lo = min(max(row_ptr[s], 0), n_trans), hi = min(max(row_ptr[s + 1], lo), n_trans);
    for (int i = lo + tid; i < hi; i += 256) {
        const int t = tokens[i];
        if (t >= 0 && t < V) atomicOr(&s_row[t >> 5], 1u << (t & 31));
        nxt[trans_base + i] = state_base + next[i];
    }
    __syncthreads();
    uint32_t* arow = allow + (size_t)(state_base + s) * row_stride;
    int32_t* rrow = rank + (size_t)(state_base + s) * row_stride;
    for (int i = 4 * tid; i < words; i += 1024) *reinterpret_cast<u32x4*>(arow + i) = *reinterpret_cast<const u32x4*>(s_row + i);
    // every thread owns `per` consecutive words (a multiple of 4): its popcount sum, a scan over the 256 sums, its rank words
    const int per = ((words + 255) / 256 + 3) & ~3;
    const int w0 = min(tid * per, words), w1 = min(w0 + per, words);
    int sum = 0;
    for (int i = w0; i < w1; i++) sum += __builtin_popcount(s_row[i]);
    s_sum[tid] = sum;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const int v = tid >= d ? s_sum[tid - d] : 0;
        __syncthreads();
        s_sum[tid] += v;
        __syncthreads();
    }
    int run = s_sum[tid] - sum;
    for (int i = w0; i < w1; i += 4) {
        int4 r;
        r.x = run; run += __builtin_popcount(s_row[i]);
        r.y = run; run += __builtin_popcount(s_row[i + 1]);
        r.z = run; run += __builtin_popcount(s_row[i + 2]);
        r.w = run; run += __builtin_popcount(s_row[i + 3]);
        *reinterpret_cast<int4*>(rrow + i) = r;
    }
    if (tid == 0) off[state_base + s] = trans_base + lo;
}
int guide_build(uint32_t* allow, int32_t* rank, int32_t* off, int32_t* nxt, int words, int row_stride, int V, int state_base,
                int trans_base, int n_states, const int32_t* row_ptr, const int32_t* tokens, const int32_t* next, int n_trans,
                hipStream_t st) {
    if (n_states == 0) return 0;
    if (words < 4 || words % 4 || words > QS_GUIDE_MAX_WORDS || row_stride < words || row_stride % 4 || (int64_t)words * 32 < V)
        return -1;
    hipLaunchKernelGGL(guide_build_kernel, dim3(n_states), dim3(256), (size_t)words * 4, st, allow, rank, off, nxt, words,
                       row_stride, V, state_base, trans_base, n_trans, row_ptr, tokens, next);
    return 0;
}
// One thread per slot, as the token table's catch-up: a guided slot's state advances over the tokens committed since the last
// catch-up, in order (k + 1 at most in the steady state, two round trips each).  Idempotent: see the INVARIANT above.
__global__ void guide_catch_up_kernel(int B, int V, int32_t* __restrict__ gslot, LpGuide g, const int64_t* __restrict__ gen_tokens,
                                      int gen_cap, const int32_t* __restrict__ gen_lens) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int4 gs = *reinterpret_cast<const int4*>(gslot + 4 * b);
    if (!gs.w) return;
    const int hi = min(gen_lens[b], gen_cap), lo = max(gs.y, 0);
    if (hi <= lo) return;   // nothing new (or gen_lens went back: a freed slot; admission sets the state again)
    int s = gs.x;
    for (int i = lo; i < hi; i++) s = guide_next(g, V, s, gen_tokens[(size_t)b * gen_cap + i], gs.z);
    gslot[4 * b] = s;
    gslot[4 * b + 1] = hi;
}
int guide_catch_up(int B, int V, int32_t* gslot, const LpGuide& g, const int64_t* gen_tokens, int gen_cap,
                   const int32_t* gen_lens, hipStream_t st) {
    if (B == 0) return 0;
    hipLaunchKernelGGL(guide_catch_up_kernel, dim3((B + 63) / 64), dim3(64), 0, st, B, V, gslot, g, gen_tokens, gen_cap, gen_lens);
    return 0;
}
// Admission (outside the graph): ONE workgroup builds the slot's deny row -- all ones where the request has allowed_token_ids,
// their bits cleared, the single-token bad words' bits set (integer atomics: the result does not depend on the order) -- and
// copies its sorted bias list and its multi-token bad words.  meta = {flags, n_bias, n_words, 0}: the tail is the admission's.
// Ids outside [0, V) are ignored.  Everything zero: the slot is unconstrained (the row is left alone, its flag says unused).
__global__ __launch_bounds__(1024) void token_constraints_set_kernel(
    uint32_t* __restrict__ deny, int deny_words, int V, const int64_t* __restrict__ allowed, int n_allowed,
    const int64_t* __restrict__ banned, int n_banned, int32_t* __restrict__ bias_ids, float* __restrict__ bias_vals,
    const int32_t* __restrict__ src_bias_ids, const float* __restrict__ src_bias_vals, int n_bias, int32_t* __restrict__ words,
    int32_t* __restrict__ word_lens, const int32_t* __restrict__ src_words, const int32_t* __restrict__ src_word_lens,
    int n_words, int32_t* __restrict__ meta, int bad_words_present) {
    const int tid = threadIdx.x;
    if (n_allowed > 0 || n_banned > 0) {
        const uint32_t fill = n_allowed > 0 ? 0xFFFFFFFFu : 0u;
        for (int i = tid; i < deny_words; i += blockDim.x) deny[i] = fill;
        __syncthreads();
        for (int i = tid; i < n_allowed; i += blockDim.x) {
            const int64_t v = allowed[i];
            if (v >= 0 && v < V) atomicAnd(deny + (v >> 5), ~(1u << (v & 31)));
        }
        __syncthreads();
        for (int i = tid; i < n_banned; i += blockDim.x) {
            const int64_t v = banned[i];
            if (v >= 0 && v < V) atomicOr(deny + (v >> 5), 1u << (v & 31));
        }
    }
    for (int i = tid; i < n_bias; i += blockDim.x) {
        bias_ids[i] = src_bias_ids[i];
        bias_vals[i] = src_bias_vals[i];
    }
    for (int i = tid; i < n_words * QS_TC_WORD_LEN; i += blockDim.x) words[i] = src_words[i];
    for (int i = tid; i < n_words; i += blockDim.x) word_lens[i] = src_word_lens[i];
    if (tid == 0) {
        meta[0] = ((n_allowed > 0 || n_banned > 0) ? 1 : 0) | (bad_words_present ? 2 : 0);
        meta[1] = n_bias;
        meta[2] = n_words;
        meta[3] = 0;
    }
}
int token_constraints_set(uint32_t* deny, int deny_words, int32_t* meta, int32_t* bias_ids, float* bias_vals, int32_t* words,
                          int32_t* word_lens, int V, int slot, const int64_t* allowed, int n_allowed, const int64_t* banned,
                          int n_banned, const int32_t* src_bias_ids, const float* src_bias_vals, int n_bias,
                          const int32_t* src_words, const int32_t* src_word_lens, int n_words, int bad_words_present,
                          hipStream_t st) {
    if (n_bias > QS_TC_MAX_BIAS || n_words > QS_TC_MAX_WORDS || (int64_t)deny_words * 32 < V) return -1;
    hipLaunchKernelGGL(token_constraints_set_kernel, dim3(1), dim3(1024), 0, st, deny + (size_t)slot * deny_words, deny_words, V,
                       allowed, n_allowed, banned, n_banned, bias_ids + (size_t)slot * QS_TC_MAX_BIAS,
                       bias_vals + (size_t)slot * QS_TC_MAX_BIAS, src_bias_ids, src_bias_vals, n_bias,
                       words + (size_t)slot * QS_TC_MAX_WORDS * QS_TC_WORD_LEN, word_lens + (size_t)slot * QS_TC_MAX_WORDS,
                       src_words, src_word_lens, n_words, meta + 4 * slot, bad_words_present);
    return 0;
}

// advance_step_flashattn_kernel without the CUDA-graph padding branch (num_seqs == num_queries).
__global__ void advance_step_kernel(int n, int block_size, int64_t* __restrict__ input_tokens,
                                    const int64_t* __restrict__ sampled, int64_t* __restrict__ positions,
                                    int32_t* __restrict__ seq_lens, int64_t* __restrict__ slot_mapping,
                                    const int32_t* __restrict__ block_tables, int64_t bt_stride) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    input_tokens[i] = sampled[i];
    const int next_len = seq_lens[i] + 1;
    const int pos = next_len - 1;
    seq_lens[i] = next_len;
    positions[i] = pos;
    slot_mapping[i] = (int64_t)block_tables[bt_stride * i + pos / block_size] * block_size + pos % block_size;
}
int advance_step(int n, int block_size, int64_t* input_tokens, const int64_t* sampled, int64_t* positions,
                 int32_t* seq_lens, int64_t* slot_mapping, const int32_t* block_tables, int64_t bt_stride,
                 hipStream_t st) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(advance_step_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, block_size, input_tokens,
                       sampled, positions, seq_lens, slot_mapping, block_tables, bt_stride);
    return 0;
}


// ---------------------------------------------------------------- spec-decode cycle glue
// The per-cycle input assembly that the reference does on the host between GPU passes
// (TP1DraftModelRunner first-step inputs, vllm/spec_decode/draft_model_runner.py:169-262;
//  MQAScorer.score_proposals, vllm/spec_decode/mqa_scorer.py:12-76;
//  SpecDecodeWorker._create_output_sampler_list bookkeeping, spec_decode_worker.py:972-1063)
// kept on the GPU so that a whole draft+verify+accept cycle is one graph with no host sync.
// Sequence state: seq_lens[b] = L tokens known, KV valid for positions < L-1, last_token[b] = token L-1.
// Empty batch slots (seq_lens[b] <= 0: a finished / not yet admitted request) run through the captured cycle as a
// harmless dummy: token 0 at position 0, context of one key, slot -1 (nothing is written to the cache), no output.
// A position beyond the sequence's block table (max_blocks entries) also gets slot -1 instead of reading past the row:
// the host refuses such a step beforehand (QSpecEngine.step), this is the in-kernel safety net.
__device__ __forceinline__ int64_t spec_slot(const int32_t* block_tables, int64_t bt_stride, int b, int pos,
                                             int block_size, int max_blocks) {
    const int blk = pos / block_size;
    if (pos < 0 || (max_blocks > 0 && blk >= max_blocks)) return -1;
    return (int64_t)block_tables[bt_stride * b + blk] * block_size + pos % block_size;
}
// (each bookkeeping step below is a per-row device function returning the row's input token: the plain kernels run one row per
// thread; the `_embed` kernels run one row per WORKGROUP -- thread 0 does the bookkeeping, then all 256 copy the token's embedding
// row into the forward's hidden buffer (embedding_kernel's copy): one launch of the cycle's chain less per forward)
__device__ __forceinline__ int64_t spec_prepare_draft_row(int b, int block_size, int max_blocks, const int64_t* last_token,
                                                          const int32_t* seq_lens, const int32_t* step_mask, int32_t* eff_lens,
                                                          const int32_t* block_tables, int64_t bt_stride, int64_t* input_tokens,
                                                          int64_t* positions, int64_t* slot_mapping, int32_t* ctx_lens) {
    int L = seq_lens[b];
    if (step_mask) {   // eff_lens = seq_lens * step_mask (slots that sit this step out count as empty)
        L *= step_mask[b];
        eff_lens[b] = L;
    }
    const int pos = L - 1;
    if (L <= 0) {
        input_tokens[b] = 0;
        positions[b] = 0;
        ctx_lens[b] = 1;
        slot_mapping[b] = -1;
        return 0;
    }
    const int64_t tok = last_token[b];
    input_tokens[b] = tok;
    positions[b] = pos;
    ctx_lens[b] = L;
    slot_mapping[b] = spec_slot(block_tables, bt_stride, b, pos, block_size, max_blocks);
    return tok;
}
__global__ void spec_prepare_draft_kernel(int B, int block_size, int max_blocks, const int64_t* __restrict__ last_token,
                                          const int32_t* __restrict__ seq_lens,
                                          const int32_t* __restrict__ block_tables, int64_t bt_stride,
                                          int64_t* __restrict__ input_tokens, int64_t* __restrict__ positions,
                                          int64_t* __restrict__ slot_mapping, int32_t* __restrict__ ctx_lens) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    spec_prepare_draft_row(b, block_size, max_blocks, last_token, seq_lens, nullptr, nullptr, block_tables, bt_stride, input_tokens,
                           positions, slot_mapping, ctx_lens);
}
struct SpecEmbed {
    const f16* table;   // [V, H]
    f16* out;           // [rows, H]
    int H, V;
};
__device__ __forceinline__ void spec_embed_row(const SpecEmbed& e, int row, int64_t tok_thread0) {
    __shared__ int64_t s_tok;
    if (threadIdx.x == 0) s_tok = tok_thread0;
    __syncthreads();
    int64_t id = s_tok;
    if (id < 0 || id >= e.V) id = 0;  // padded slot (embedding_kernel's rule)
    const f16* src = e.table + id * e.H;
    for (int i = threadIdx.x; i < e.H / 8; i += blockDim.x)
        *reinterpret_cast<f16x8*>(e.out + (size_t)row * e.H + 8 * i) = *reinterpret_cast<const f16x8*>(src + 8 * i);
}
__global__ __launch_bounds__(256) void spec_prepare_draft_embed_kernel(int block_size, int max_blocks, const int64_t* __restrict__ last_token,
                                                                       const int32_t* __restrict__ seq_lens, const int32_t* __restrict__ step_mask,
                                                                       int32_t* __restrict__ eff_lens, const int32_t* __restrict__ block_tables,
                                                                       int64_t bt_stride, int64_t* __restrict__ input_tokens,
                                                                       int64_t* __restrict__ positions, int64_t* __restrict__ slot_mapping,
                                                                       int32_t* __restrict__ ctx_lens, SpecEmbed e) {
    const int b = blockIdx.x;
    int64_t tok = 0;
    if (threadIdx.x == 0)
        tok = spec_prepare_draft_row(b, block_size, max_blocks, last_token, seq_lens, step_mask, eff_lens, block_tables, bt_stride,
                                     input_tokens, positions, slot_mapping, ctx_lens);
    spec_embed_row(e, b, tok);
}
// _gpu_advance_step between two draft steps (draft_model_runner.py:78-135) with the two engine rules above: a row
// whose slot is -1 (empty, or out of blocks) stays put; a new position beyond the block table gets slot -1.
__device__ __forceinline__ int64_t spec_advance_draft_row(int i, int block_size, int max_blocks, int64_t* input_tokens,
                                                          const int64_t* sampled, int64_t* positions, int32_t* ctx_lens,
                                                          int64_t* slot_mapping, const int32_t* block_tables, int64_t bt_stride) {
    if (slot_mapping[i] < 0) return input_tokens[i];
    const int64_t tok = sampled[i];
    input_tokens[i] = tok;
    const int next_len = ctx_lens[i] + 1;
    const int pos = next_len - 1;
    const int64_t slot = spec_slot(block_tables, bt_stride, i, pos, block_size, max_blocks);
    if (slot < 0) {   // out of blocks: freeze the row (its remaining draft steps recompute the same token)
        slot_mapping[i] = -1;
        return tok;
    }
    ctx_lens[i] = next_len;
    positions[i] = pos;
    slot_mapping[i] = slot;
    return tok;
}
__global__ void spec_advance_draft_kernel(int n, int block_size, int max_blocks, int64_t* __restrict__ input_tokens,
                                          const int64_t* __restrict__ sampled, int64_t* __restrict__ positions,
                                          int32_t* __restrict__ ctx_lens, int64_t* __restrict__ slot_mapping,
                                          const int32_t* __restrict__ block_tables, int64_t bt_stride) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    spec_advance_draft_row(i, block_size, max_blocks, input_tokens, sampled, positions, ctx_lens, slot_mapping, block_tables, bt_stride);
}
__global__ __launch_bounds__(256) void spec_advance_draft_embed_kernel(int block_size, int max_blocks, int64_t* __restrict__ input_tokens,
                                                                       const int64_t* __restrict__ sampled, int64_t* __restrict__ positions,
                                                                       int32_t* __restrict__ ctx_lens, int64_t* __restrict__ slot_mapping,
                                                                       const int32_t* __restrict__ block_tables, int64_t bt_stride, SpecEmbed e) {
    const int i = blockIdx.x;
    int64_t tok = 0;
    if (threadIdx.x == 0)
        tok = spec_advance_draft_row(i, block_size, max_blocks, input_tokens, sampled, positions, ctx_lens, slot_mapping, block_tables,
                                     bt_stride);
    spec_embed_row(e, i, tok);
}
// verify query of sequence b = [last_token, d_1 .. d_k] at positions L-1 .. L-1+k (mqa_scorer.py:42-60)
__device__ __forceinline__ int64_t spec_prepare_verify_row(int i, int k, int block_size, int max_blocks, const int64_t* last_token,
                                                           const int64_t* draft_ids, int64_t di_sb, int64_t di_sk, const int32_t* seq_lens,
                                                           const int32_t* block_tables, int64_t bt_stride, int64_t* v_tokens,
                                                           int64_t* v_positions, int64_t* v_slots, int32_t* v_ctx_lens) {
    const int b = i / (k + 1), j = i % (k + 1);
    const int L = seq_lens[b], pos = L - 1 + j;
    if (L <= 0) {   // empty slot: k + 1 dummy queries over the first k + 1 keys of the row, nothing written
        v_tokens[i] = 0;
        v_positions[i] = j;
        v_slots[i] = -1;
        if (j == 0) v_ctx_lens[b] = k + 1;
        return 0;
    }
    const int64_t tok = j == 0 ? last_token[b] : draft_ids[b * di_sb + (j - 1) * di_sk];
    v_tokens[i] = tok;
    v_positions[i] = pos;
    v_slots[i] = spec_slot(block_tables, bt_stride, b, pos, block_size, max_blocks);
    if (j == 0) v_ctx_lens[b] = L + k;
    return tok;
}
__global__ void spec_prepare_verify_kernel(int B, int k, int block_size, int max_blocks, const int64_t* __restrict__ last_token,
                                           const int64_t* __restrict__ draft_ids, int64_t di_sb, int64_t di_sk,
                                           const int32_t* __restrict__ seq_lens,
                                           const int32_t* __restrict__ block_tables, int64_t bt_stride,
                                           int64_t* __restrict__ v_tokens, int64_t* __restrict__ v_positions,
                                           int64_t* __restrict__ v_slots, int32_t* __restrict__ v_ctx_lens) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * (k + 1)) return;
    spec_prepare_verify_row(i, k, block_size, max_blocks, last_token, draft_ids, di_sb, di_sk, seq_lens, block_tables, bt_stride, v_tokens,
                            v_positions, v_slots, v_ctx_lens);
}
__global__ __launch_bounds__(256) void spec_prepare_verify_embed_kernel(int k, int block_size, int max_blocks, const int64_t* __restrict__ last_token,
                                                                        const int64_t* __restrict__ draft_ids, int64_t di_sb, int64_t di_sk,
                                                                        const int32_t* __restrict__ seq_lens,
                                                                        const int32_t* __restrict__ block_tables, int64_t bt_stride,
                                                                        int64_t* __restrict__ v_tokens, int64_t* __restrict__ v_positions,
                                                                        int64_t* __restrict__ v_slots, int32_t* __restrict__ v_ctx_lens, SpecEmbed e) {
    const int i = blockIdx.x;
    int64_t tok = 0;
    if (threadIdx.x == 0)
        tok = spec_prepare_verify_row(i, k, block_size, max_blocks, last_token, draft_ids, di_sb, di_sk, seq_lens, block_tables, bt_stride,
                                      v_tokens, v_positions, v_slots, v_ctx_lens);
    spec_embed_row(e, i, tok);
}
// append the emitted tokens (out != -1, a prefix of the row) and advance the sequence state
__global__ void spec_commit_kernel(int B, int k, const int64_t* __restrict__ out_tokens,
                                   int32_t* __restrict__ seq_lens, int64_t* __restrict__ last_token,
                                   int64_t* __restrict__ gen_tokens, int32_t* __restrict__ gen_lens, int gen_cap) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    int n = 0;
    for (int j = 0; j <= k; j++) {
        int64_t t = out_tokens[b * (k + 1) + j];
        if (t == -1) break;
        if (gen_tokens && gen_lens[b] + n < gen_cap) gen_tokens[(int64_t)b * gen_cap + gen_lens[b] + n] = t;
        n++;
    }
    if (n > 0) {
        last_token[b] = out_tokens[b * (k + 1) + n - 1];
        seq_lens[b] += n;
        if (gen_lens) gen_lens[b] += n;
    }
}
// The small per-cycle sequence state, copied aside at the start of a cycle (restore = the same kernel with the
// arguments swapped): seq_lens / gen_lens [B] i32, last_token [B] i64, counters [3] i64, rng_state [2] i64.
// snap_i32 [2B], snap_i64 [B + 5].
__global__ void spec_snapshot_kernel(int B, const int32_t* __restrict__ seq_lens, const int32_t* __restrict__ gen_lens,
                                     const int64_t* __restrict__ last_token, const int64_t* __restrict__ counters,
                                     const int64_t* __restrict__ rng_state, int32_t* __restrict__ snap_i32,
                                     int64_t* __restrict__ snap_i64) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) {
        snap_i32[i] = seq_lens[i];
        snap_i32[B + i] = gen_lens[i];
        snap_i64[i] = last_token[i];
    }
    if (i < 3) snap_i64[B + i] = counters[i];
    if (i < 2) snap_i64[B + 3 + i] = rng_state[i];
}
__global__ void spec_restore_kernel(int B, int32_t* __restrict__ seq_lens, int32_t* __restrict__ gen_lens,
                                    int64_t* __restrict__ last_token, int64_t* __restrict__ counters,
                                    int64_t* __restrict__ rng_state, const int32_t* __restrict__ snap_i32,
                                    const int64_t* __restrict__ snap_i64) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < B) {
        seq_lens[i] = snap_i32[i];
        gen_lens[i] = snap_i32[B + i];
        last_token[i] = snap_i64[i];
    }
    if (i < 3) counters[i] = snap_i64[B + i];
    if (i < 2) rng_state[i] = snap_i64[B + 3 + i];
}
// out[0] = OR of |*w| over up to four sticky error words (hand-off workspaces, one-shot all-reduce; NULL = none): read
// by the host together with the cycle's output tokens; all-reduced (sum) over the ranks under tensor parallelism.
// The addresses are kernel arguments (constants of a captured graph), not a device table.
__global__ void collect_error_words_kernel(int32_t* w0, int32_t* w1, int32_t* w2, int32_t* w3, int clear,
                                           int64_t* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int32_t* ws[4] = {w0, w1, w2, w3};
    int64_t acc = 0;
    for (int i = 0; i < 4; i++) {
        if (!ws[i]) continue;
        const int32_t v = __hip_atomic_load(ws[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        acc |= (int64_t)(v < 0 ? -(int64_t)v : (int64_t)v);
        if (clear) __hip_atomic_store(ws[i], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (out) out[0] = acc;
}
int spec_snapshot(int B, int restore, int32_t* seq_lens, int32_t* gen_lens, int64_t* last_token, int64_t* counters,
                  int64_t* rng_state, int32_t* snap_i32, int64_t* snap_i64, hipStream_t st) {
    const int n = B > 3 ? B : 3;
    if (restore)
        hipLaunchKernelGGL(spec_restore_kernel, dim3((n + 63) / 64), dim3(64), 0, st, B, seq_lens, gen_lens, last_token,
                           counters, rng_state, snap_i32, snap_i64);
    else
        hipLaunchKernelGGL(spec_snapshot_kernel, dim3((n + 63) / 64), dim3(64), 0, st, B, seq_lens, gen_lens, last_token,
                           counters, rng_state, snap_i32, snap_i64);
    return 0;
}
int collect_error_words(int32_t* w0, int32_t* w1, int32_t* w2, int32_t* w3, int clear, int64_t* out, hipStream_t st) {
    hipLaunchKernelGGL(collect_error_words_kernel, dim3(1), dim3(64), 0, st, w0, w1, w2, w3, clear, out);
    return 0;
}
int spec_prepare_draft_embed(int B, int block_size, int max_blocks, const int64_t* last_token, const int32_t* seq_lens,
                             const int32_t* step_mask, int32_t* eff_lens, const int32_t* block_tables, int64_t bt_stride,
                             int64_t* input_tokens, int64_t* positions, int64_t* slot_mapping, int32_t* ctx_lens, const f16* table,
                             f16* hidden_out, int H, int V, hipStream_t st) {
    if (B == 0) return 0;
    if (H % 8 || (step_mask && !eff_lens)) return -1;
    hipLaunchKernelGGL(spec_prepare_draft_embed_kernel, dim3(B), dim3(256), 0, st, block_size, max_blocks, last_token, seq_lens, step_mask,
                       eff_lens, block_tables, bt_stride, input_tokens, positions, slot_mapping, ctx_lens, SpecEmbed{table, hidden_out, H, V});
    return 0;
}
int spec_advance_draft_embed(int n, int block_size, int max_blocks, int64_t* input_tokens, const int64_t* sampled, int64_t* positions,
                             int32_t* ctx_lens, int64_t* slot_mapping, const int32_t* block_tables, int64_t bt_stride, const f16* table,
                             f16* hidden_out, int H, int V, hipStream_t st) {
    if (n == 0) return 0;
    if (H % 8) return -1;
    hipLaunchKernelGGL(spec_advance_draft_embed_kernel, dim3(n), dim3(256), 0, st, block_size, max_blocks, input_tokens, sampled, positions,
                       ctx_lens, slot_mapping, block_tables, bt_stride, SpecEmbed{table, hidden_out, H, V});
    return 0;
}
int spec_prepare_verify_embed(int B, int k, int block_size, int max_blocks, const int64_t* last_token, const int64_t* draft_ids,
                              int64_t di_sb, int64_t di_sk, const int32_t* seq_lens, const int32_t* block_tables, int64_t bt_stride,
                              int64_t* v_tokens, int64_t* v_positions, int64_t* v_slots, int32_t* v_ctx_lens, const f16* table,
                              f16* hidden_out, int H, int V, hipStream_t st) {
    if (B == 0) return 0;
    if (H % 8) return -1;
    hipLaunchKernelGGL(spec_prepare_verify_embed_kernel, dim3(B * (k + 1)), dim3(256), 0, st, k, block_size, max_blocks, last_token, draft_ids,
                       di_sb, di_sk, seq_lens, block_tables, bt_stride, v_tokens, v_positions, v_slots, v_ctx_lens,
                       SpecEmbed{table, hidden_out, H, V});
    return 0;
}
int spec_prepare_draft(int B, int block_size, int max_blocks, const int64_t* last_token, const int32_t* seq_lens,
                       const int32_t* block_tables, int64_t bt_stride, int64_t* input_tokens, int64_t* positions,
                       int64_t* slot_mapping, int32_t* ctx_lens, hipStream_t st) {
    if (B == 0) return 0;
    hipLaunchKernelGGL(spec_prepare_draft_kernel, dim3((B + 63) / 64), dim3(64), 0, st, B, block_size, max_blocks,
                       last_token, seq_lens, block_tables, bt_stride, input_tokens, positions, slot_mapping, ctx_lens);
    return 0;
}
int spec_advance_draft(int n, int block_size, int max_blocks, int64_t* input_tokens, const int64_t* sampled,
                       int64_t* positions, int32_t* ctx_lens, int64_t* slot_mapping, const int32_t* block_tables,
                       int64_t bt_stride, hipStream_t st) {
    if (n == 0) return 0;
    hipLaunchKernelGGL(spec_advance_draft_kernel, dim3((n + 63) / 64), dim3(64), 0, st, n, block_size, max_blocks,
                       input_tokens, sampled, positions, ctx_lens, slot_mapping, block_tables, bt_stride);
    return 0;
}
int spec_prepare_verify(int B, int k, int block_size, int max_blocks, const int64_t* last_token, const int64_t* draft_ids,
                        int64_t di_sb, int64_t di_sk, const int32_t* seq_lens, const int32_t* block_tables, int64_t bt_stride, int64_t* v_tokens,
                        int64_t* v_positions, int64_t* v_slots, int32_t* v_ctx_lens, hipStream_t st) {
    if (B == 0) return 0;
    const int n = B * (k + 1);
    hipLaunchKernelGGL(spec_prepare_verify_kernel, dim3((n + 63) / 64), dim3(64), 0, st, B, k, block_size, max_blocks, last_token,
                       draft_ids, di_sb, di_sk, seq_lens, block_tables, bt_stride, v_tokens, v_positions, v_slots, v_ctx_lens);
    return 0;
}
int spec_commit(int B, int k, const int64_t* out_tokens, int32_t* seq_lens, int64_t* last_token, int64_t* gen_tokens,
                int32_t* gen_lens, int gen_cap, hipStream_t st) {
    if (B == 0) return 0;
    hipLaunchKernelGGL(spec_commit_kernel, dim3((B + 63) / 64), dim3(64), 0, st, B, k, out_tokens, seq_lens,
                       last_token, gen_tokens, gen_lens, gen_cap);
    return 0;
}

}  // namespace qspec
