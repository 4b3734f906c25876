// Token logprobs, ranks and the N best per row (include/qspec_hip.h, "logprobs"): what Sampler.forward's get_logprobs /
// _get_ranks (sampler.py:861-879, :882 ff.) and the worker's torch expression computed with several full passes over the
// vocabulary and two [rows, V] temporaries.  ONE launch, one workgroup of 16 waves per row, no workspace, no global atomics:
//
//   pass 1   rank count (#{x > x[token]}), the row maximum (logits form) and a histogram of the top 12 key bits
//   refine   while the bin holding the N-th largest value has more than LP_SMALL members: a histogram of the next 12 bits of
//            the members of that bin (a radix select -- the idea of topk_hist_kernel / topk_select_kernel in sampler.hip)
//   collect  everything above the threshold bin (< N values) and the bin's members (<= LP_SMALL, or -- exact ties only -- the
//            lowest ids in order) into an LDS list of at most 96 candidates, which is ranked by (value desc, id asc)
//
// The logits form's sum of exponentials rides in the second pass, whichever that is.  A row is 256 KB of fp16 or 513 KB of
// fp32 at V = 128256: it comes from HBM once and from L2 in the later passes (two to four; five for an fp32 row whose N-th
// value sits in a tie group of more than LP_SMALL).  Values are ordered through a monotone integer key (-0 counts as +0), so
// every compare is exact and denormals never depend on the float mode.
#include <float.h>

#include "common.cuh"
#include "kernels.h"

namespace qspec {
namespace {

constexpr int LP_THREADS = 1024;
constexpr int LP_WAVES = LP_THREADS / 64;
constexpr int LP_MAX_TOP = 32;                    // QS_MAX_LOGPROBS of include/qspec_hip.h
constexpr int LP_DIGIT = 12;                      // key bits per histogram level
constexpr int LP_BINS = 1 << LP_DIGIT;
constexpr int LP_SMALL = 64;                      // a threshold bin of at most this many members is collected whole
constexpr int LP_CAND = LP_MAX_TOP + LP_SMALL;    // candidates: < N above the bin + the bin (or the ties taken from it)
constexpr int LP_UNROLL = 4;                      // 16-byte loads in flight per lane

template <typename T> struct Elem;
template <> struct Elem<float> {
    static constexpr int VEC = 4, KEY_BITS = 32;
    static __device__ __forceinline__ u32 bits(const u32x4& r, int e) { return r[e]; }
    static __device__ __forceinline__ u32 load_bits(const float* p) { return __builtin_bit_cast(u32, *p); }
    static __device__ __forceinline__ u32 key(u32 b) {
        if ((b << 1) == 0) b = 0;
        return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
    }
    static __device__ __forceinline__ float value(u32 k) {
        return __builtin_bit_cast(float, k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu));
    }
};
template <> struct Elem<f16> {
    static constexpr int VEC = 8, KEY_BITS = 16;
    static __device__ __forceinline__ u32 bits(const u32x4& r, int e) { return (r[e >> 1] >> ((e & 1) * 16)) & 0xFFFFu; }
    static __device__ __forceinline__ u32 load_bits(const f16* p) { return h2u(*p); }
    static __device__ __forceinline__ u32 key(u32 b) {
        if ((b & 0x7FFFu) == 0) b = 0;
        return b ^ ((b & 0x8000u) ? 0xFFFFu : 0x8000u);
    }
    static __device__ __forceinline__ float value(u32 k) {
        return h2f(u2h((uint16_t)(k ^ ((k & 0x8000u) ? 0x8000u : 0xFFFFu))));
    }
};

// Walks one row: wave w owns a contiguous range of 16-byte vectors, its lanes take consecutive vectors, so ids ascend with
// (iteration, lane, element).  f(id0, keys, valid) is called by ALL 64 lanes together (it may use wave collectives); bit e of
// `valid` says whether element id0 + e is inside [0, vocab).  Vector j covers the elements j * VEC - a0 ..., a0 being the
// row's misalignment in elements: a vector that is whole inside the row is ONE aligned 16-byte load, the (at most two)
// boundary vectors are read element by element, and nothing outside the row is touched.
template <typename T, typename F>
__device__ __forceinline__ void scan_row(const T* row, int vocab, int a0, int nv, F&& f) {
    typedef Elem<T> E;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int per_wave = (nv + LP_WAVES - 1) / LP_WAVES;
    const int v0 = wave * per_wave, v1 = min(v0 + per_wave, nv);
    for (int base = v0; base < v1; base += 64 * LP_UNROLL) {
        u32x4 raw[LP_UNROLL];
        bool whole[LP_UNROLL];
#pragma unroll
        for (int u = 0; u < LP_UNROLL; ++u) {
            const int j = base + u * 64 + lane;
            const int64_t e0 = (int64_t)j * E::VEC - a0;
            whole[u] = j < v1 && e0 >= 0 && e0 + E::VEC <= vocab;
            raw[u] = u32x4{0, 0, 0, 0};
            if (whole[u]) raw[u] = *reinterpret_cast<const u32x4*>(row + e0);
        }
#pragma unroll
        for (int u = 0; u < LP_UNROLL; ++u) {
            const int j = base + u * 64 + lane;
            const int64_t e0 = (int64_t)j * E::VEC - a0;
            u32 keys[E::VEC];
            u32 valid = 0;
#pragma unroll
            for (int e = 0; e < E::VEC; ++e) {
                const int64_t id = e0 + e;
                const bool ok = j < v1 && id >= 0 && id < vocab;
                u32 b = E::bits(raw[u], e);
                if (!whole[u] && ok) b = E::load_bits(row + id);
                keys[e] = E::key(b);
                valid |= ok ? (1u << e) : 0u;
            }
            f((int)e0, keys, valid);
        }
    }
}

// hist[bin] += 1 for the lanes with `on`; a wave whose lanes all hit one bin (a row of zeros behind a top-k mask, an
// all-equal row) sends ONE LDS atomic instead of 64 to the same address.
__device__ __forceinline__ void hist_add(u32* hist, u32 bin, bool on) {
    const uint64_t mask = __builtin_amdgcn_ballot_w64(on);
    if (mask == 0) return;
    const int leader = __builtin_ctzll(mask);
    const u32 first = (u32)__shfl((int)bin, leader, 64);
    const uint64_t same = __builtin_amdgcn_ballot_w64(on && bin == first);
    if (same == mask) {
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(&hist[first], (u32)__builtin_popcountll(mask));
    } else if (on) {
        atomicAdd(&hist[bin], 1u);
    }
}

__device__ __forceinline__ u32 wave_sum_u(u32 v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (u32)__shfl_xor((int)v, d, 64);
    return v;
}
__device__ __forceinline__ u32 wave_max_u(u32 v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, (u32)__shfl_xor((int)v, d, 64));
    return v;
}
__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ u32 wave_incl_scan_u(u32 v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const u32 o = (u32)__shfl_up((int)v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

struct Threshold {
    int bin, above, count;   // the bin in which the running count from the top reaches `need`, the count above it, its own
};

// hist[0 .. nbins): where, walking down from the top bin, the running count reaches `need` (1 <= need <= total).  Ends with
// a barrier; `part` is LP_WAVES words and `out` one Threshold of LDS.
__device__ __forceinline__ Threshold find_threshold(const u32* hist, int nbins, int need, u32* part, Threshold* out) {
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const int per = (nbins + LP_THREADS - 1) / LP_THREADS;
    u32 local = 0;
    for (int i = 0; i < per; ++i) {
        const int ri = t * per + i;   // reversed index: 0 = the top bin
        if (ri < nbins) local += hist[nbins - 1 - ri];
    }
    const u32 incl_w = wave_incl_scan_u(local);
    if (lane == 63) part[wave] = incl_w;
    __syncthreads();
    u32 offset = 0;
    for (int w = 0; w < wave; ++w) offset += part[w];
    const u32 incl = offset + incl_w, excl = incl - local;
    if (excl < (u32)need && (u32)need <= incl) {   // exactly one thread
        u32 run = excl;
        for (int i = 0; i < per; ++i) {
            const int ri = t * per + i;
            if (ri >= nbins) break;
            const u32 c = hist[nbins - 1 - ri];
            if (run + c >= (u32)need) {
                out->bin = nbins - 1 - ri;
                out->above = (int)run;
                out->count = (int)c;
                break;
            }
            run += c;
        }
    }
    __syncthreads();
    return *out;
}

template <typename T, bool LOGITS>
__global__ __launch_bounds__(LP_THREADS) void token_logprobs_kernel(const T* __restrict__ x, int64_t row_stride,
                                                                    const int64_t* __restrict__ token_ids, int vocab, int num_top,
                                                                    float* __restrict__ token_logprob,
                                                                    int32_t* __restrict__ token_rank, int32_t* __restrict__ top_ids,
                                                                    float* __restrict__ top_logprobs) {
    typedef Elem<T> E;
    __shared__ u32 hist[LP_BINS];
    __shared__ u32 cand_key[LP_CAND];
    __shared__ int cand_id[LP_CAND];
    __shared__ int tie_id[LP_WAVES][LP_MAX_TOP];
    __shared__ int tie_cnt[LP_WAVES];
    __shared__ u32 part_u[LP_WAVES], part_m[LP_WAVES], part_s[LP_WAVES];
    __shared__ float part_f[LP_WAVES];
    __shared__ Threshold thr;
    __shared__ int n_cand;

    const int r = blockIdx.x, t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const T* row = x + (int64_t)r * row_stride;
    const int a0 = (int)((reinterpret_cast<uintptr_t>(row) / sizeof(T)) % E::VEC);
    const int nv = (int)(((int64_t)a0 + vocab + E::VEC - 1) / E::VEC);
    const int64_t tok = token_ids[r];
    const bool in_range = tok >= 0 && tok < vocab;
    const u32 tok_key = in_range ? E::key(E::load_bits(row + tok)) : 0xFFFFFFFFu;
    const int n_eff = min(num_top, vocab);

    // ---- pass 1: rank count, row maximum, first histogram level
    int s = E::KEY_BITS - LP_DIGIT;   // shift of the digit in hand (both key widths have more than LP_DIGIT bits)
    for (int i = t; i < LP_BINS; i += LP_THREADS) hist[i] = 0;
    if (t == 0) n_cand = 0;
    if (t < LP_WAVES) tie_cnt[t] = 0;
    __syncthreads();
    u32 gt = 0, mkey = 0;
    scan_row(row, vocab, a0, nv, [&](int id0, const u32* keys, u32 valid) {
#pragma unroll
        for (int e = 0; e < E::VEC; ++e) {
            const bool ok = (valid >> e) & 1u;
            gt += (ok && keys[e] > tok_key) ? 1u : 0u;
            if (LOGITS) mkey = max(mkey, ok ? keys[e] : 0u);
            if (num_top > 0) hist_add(hist, keys[e] >> s, ok);
        }
    });
    gt = wave_sum_u(gt);
    mkey = wave_max_u(mkey);
    if (lane == 0) {
        part_u[wave] = gt;
        part_m[wave] = mkey;
    }
    __syncthreads();
    gt = 0;
    mkey = 0;
    for (int w = 0; w < LP_WAVES; ++w) {
        gt += part_u[w];
        mkey = max(mkey, part_m[w]);
    }
    const float m = LOGITS ? E::value(mkey) : 0.0f;
    float esum = 0.0f;        // this thread's share of sum exp(x - m)
    bool summed = !LOGITS;    // (uniform) the share has been accumulated
    auto add_exp = [&](const u32* keys, u32 valid) {
#pragma unroll
        for (int e = 0; e < E::VEC; ++e)
            if ((valid >> e) & 1u) esum += expf(E::value(keys[e]) - m);
    };

    // ---- radix select of the n_eff-th largest key: prefix P of the key bits above s, `need` still to be taken from its bin
    u32 P = 0;
    int need = n_eff, cnt = vocab;
    if (num_top > 0) {
        Threshold th = find_threshold(hist, LP_BINS, need, part_s, &thr);
        need -= th.above;
        P = (u32)th.bin;
        cnt = th.count;
        while (cnt > LP_SMALL && s > 0) {
            const int width = min(LP_DIGIT, s);
            const int hi = s;   // the prefix is key >> hi
            s -= width;
            const int nb = 1 << width;
            for (int i = t; i < nb; i += LP_THREADS) hist[i] = 0;
            __syncthreads();
            const bool do_sum = !summed;
            scan_row(row, vocab, a0, nv, [&](int id0, const u32* keys, u32 valid) {
#pragma unroll
                for (int e = 0; e < E::VEC; ++e)
                    hist_add(hist, (keys[e] >> s) & (u32)(nb - 1), ((valid >> e) & 1u) && (keys[e] >> hi) == P);
                if (do_sum) add_exp(keys, valid);
            });
            summed = true;
            __syncthreads();
            th = find_threshold(hist, nb, need, part_s, &thr);
            need -= th.above;
            P = (P << width) | (u32)th.bin;
            cnt = th.count;
        }
        // ---- collect: keys above the threshold prefix, and its bin whole -- or, a tie group of more than LP_SMALL (s == 0,
        // P the key itself), per wave the first LP_MAX_TOP ids in ascending order
        const bool ties = cnt > LP_SMALL;
        const bool do_sum = !summed;
        int wave_ties = 0;   // (uniform) ties this wave has seen
        scan_row(row, vocab, a0, nv, [&](int id0, const u32* keys, u32 valid) {
            u32 eq = 0;
#pragma unroll
            for (int e = 0; e < E::VEC; ++e) {
                if (!((valid >> e) & 1u)) continue;
                const u32 pk = keys[e] >> s;
                if (pk > P || (pk == P && !ties)) {
                    const int slot = atomicAdd(&n_cand, 1);
                    if (slot < LP_CAND) {
                        cand_key[slot] = keys[e];
                        cand_id[slot] = id0 + e;
                    }
                } else if (pk == P) {
                    eq |= 1u << e;
                }
            }
            if (ties && wave_ties < LP_MAX_TOP && __builtin_amdgcn_ballot_w64(eq != 0) != 0) {
                const u32 mine = (u32)__builtin_popcount(eq);
                const u32 incl = wave_incl_scan_u(mine);
                u32 at = (u32)wave_ties + incl - mine;
#pragma unroll
                for (int e = 0; e < E::VEC; ++e)
                    if ((eq >> e) & 1u) {
                        if (at < (u32)LP_MAX_TOP) tie_id[wave][at] = id0 + e;
                        ++at;
                    }
                wave_ties += (int)__shfl((int)incl, 63, 64);
            }
            if (do_sum) add_exp(keys, valid);
        });
        summed = true;
        if (ties && lane == 0) tie_cnt[wave] = min(wave_ties, LP_MAX_TOP);
        __syncthreads();
        if (ties && t == 0) {   // the `need` lowest ids of the tie group: the waves' lists in wave order
            int n = min(n_cand, LP_CAND);
            int taken = 0;
            for (int w = 0; w < LP_WAVES && taken < need; ++w)
                for (int i = 0; i < tie_cnt[w] && taken < need && n < LP_CAND; ++i, ++taken, ++n) {
                    cand_key[n] = P;
                    cand_id[n] = tie_id[w][i];
                }
            n_cand = n;
        }
        __syncthreads();
    } else if (LOGITS) {
        scan_row(row, vocab, a0, nv, [&](int id0, const u32* keys, u32 valid) { add_exp(keys, valid); });
        summed = true;
    }

    float lse = 0.0f;
    if (LOGITS) {
        esum = wave_sum_f(esum);
        if (lane == 0) part_f[wave] = esum;
        __syncthreads();
        float total = 0.0f;
        for (int w = 0; w < LP_WAVES; ++w) total += part_f[w];
        lse = m + logf(total);
    }
    auto lp = [&](u32 key) {
        const float v = E::value(key);
        return LOGITS ? v - lse : logf(fmaxf(v, FLT_MIN));
    };
    if (t == 0) {
        token_logprob[r] = in_range ? lp(tok_key) : 0.0f;
        token_rank[r] = in_range ? (int32_t)(1 + gt) : -1;
    }
    if (num_top > 0) {
        const int nc = min(n_cand, LP_CAND);
        int32_t* ids = top_ids + (int64_t)r * num_top;
        float* lps = top_logprobs + (int64_t)r * num_top;
        if (t < nc) {   // position among the candidates by (value descending, id ascending)
            const u32 k = cand_key[t];
            const int id = cand_id[t];
            int pos = 0;
            for (int j = 0; j < nc; ++j) pos += (cand_key[j] > k || (cand_key[j] == k && cand_id[j] < id)) ? 1 : 0;
            if (pos < n_eff) {
                ids[pos] = id;
                lps[pos] = lp(k);
            }
        }
        if (t >= n_eff && t < num_top) {   // num_top > vocab: the surplus entries
            ids[t] = -1;
            lps[t] = -__builtin_inff();
        }
    }
}

template <typename T, bool LOGITS>
int launch(const T* x, int64_t row_stride, const int64_t* token_ids, int rows, int vocab, int num_top, float* token_logprob,
           int32_t* token_rank, int32_t* top_ids, float* top_logprobs, hipStream_t st) {
    if (vocab < 1 || num_top < 0 || num_top > LP_MAX_TOP || row_stride < vocab) return -1;
    if (rows <= 0) return 0;
    hipLaunchKernelGGL((token_logprobs_kernel<T, LOGITS>), dim3(rows), dim3(LP_THREADS), 0, st, x, row_stride, token_ids, vocab,
                       num_top, token_logprob, token_rank, top_ids, top_logprobs);
    return 0;
}

}  // namespace

int token_logprobs_from_probs(const float* probs, int64_t row_stride, const int64_t* token_ids, int rows, int vocab, int num_top,
                              float* token_logprob, int32_t* token_rank, int32_t* top_ids, float* top_logprobs, hipStream_t st) {
    return launch<float, false>(probs, row_stride, token_ids, rows, vocab, num_top, token_logprob, token_rank, top_ids,
                                top_logprobs, st);
}

int token_logprobs_from_logits(const f16* logits, int64_t row_stride, const int64_t* token_ids, int rows, int vocab, int num_top,
                               float* token_logprob, int32_t* token_rank, int32_t* top_ids, float* top_logprobs, hipStream_t st) {
    return launch<f16, true>(logits, row_stride, token_ids, rows, vocab, num_top, token_logprob, token_rank, top_ids,
                             top_logprobs, st);
}

}  // namespace qspec
