// LayerNorm-without-gamma (+ per-token int4 quant) and row-absmax int4 quant.
//
// Replaces (reference, relative to /root/reference):
//   generalLayerNorm_fuse_sum_i4<half, at::Half>   third-party/kernels/csrc/layernorm_kernels.cu:569-716
//   rms_norm_general_fuse_sum_{i4,fp16} launchers   :890-957
//   rowAbsMaxQuantizeKernel                          third-party/QuaRot/quarot/kernels/quant.cu:102-167
//
// The reference runs 1024 threads per row with 2-byte strided loads.  Here one
// 256-thread workgroup owns a row; thread j plays the reference's "virtual
// threads" 4j..4j+3, so each trip is one coalesced 8-byte load per lane while
// the fp32 summation tree (thread-strided partials -> 32-lane xor butterfly ->
// 32 warp sums -> butterfly) is reproduced bit for bit.  That is what makes
// the packed int4 bytes identical to the oracle's.
#include "common.cuh"
#include "kernels.h"

namespace qspec {

// Reference summation tree over 1024 virtual-thread partials held 4 per lane.
// red must hold 32 floats and is written once per call site (callers pass distinct regions, so no barrier is needed
// in front); all 256 threads return the same bits.  First butterfly (virtual lane bits 4,3,2 <-> j ^ 4, 2, 1) as
// one-instruction DPP adds, the four chains interleaved; second butterfly over the 32 warp sums ACROSS LANES (lane l takes
// warp sum l & 31; levels 16, 8, 4, 2, 1 by ds_swizzle and DPP adds): same pairings, same order, every addition
// commutative -- the same bits as the reference's shuffle form -- in 6 instructions instead of 8 broadcast LDS reads + 31
// adds per thread.  The result is wave-uniform (read back from lane 0).
__device__ __forceinline__ float ref_tree_sum_1024(float p0, float p1, float p2, float p3, float* red) {
    float p[4] = {p0, p1, p2, p3};
    dpp_add_tree421_x4(p);
    // virtual lane bits 1, 0 are in-thread
    const float r0 = p[0] + p[2], r1 = p[1] + p[3];
    const float s = r0 + r1;
    const int j = threadIdx.x;
    if ((j & 7) == 0) red[j >> 3] = s;
    __syncthreads();
    float x = red[j & 31];
    x = x + swizzle_xor16_f(x);
    x = dpp_add_xor<8>(x);
    x = dpp_add_xor<4>(x);
    x = dpp_add_xor<2>(x);
    x = dpp_add_xor<1>(x);
    return readlane_f(x, 0);
}

// red: 4 floats of its own (written once per call site)
__device__ __forceinline__ float block_max_256(float v, float* red) {
    v = wave_max_uniform(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

// MODE 0: int4 quant (q, scale, input_sum); MODE 1: fp16 out.
// If delta != nullptr the row is first formed as h(f(x) + f(delta)) (the fp16
// residual add of quarot_llama.py:380,390) and written to hidden_out.
template <int NI, int MODE>
__global__ __launch_bounds__(256) void ln_kernel(const f16* x, const f16* __restrict__ delta,
                                                 f16* hidden_out /* may alias x */, f16* __restrict__ out,
                                                 int8_t* __restrict__ q, f16* __restrict__ scale,
                                                 f16* __restrict__ input_sum, float eps, int H,
                                                 const float* __restrict__ part = nullptr,
                                                 const f16* __restrict__ pws = nullptr, int S = 0, size_t pstride = 0,
                                                 const int* __restrict__ ipart = nullptr, const f16* __restrict__ pxs = nullptr,
                                                 int xp = 0 /* MODE 1: `out` in the W4A16 fragment-major layout (T <= 16) */) {
    __shared__ __attribute__((aligned(16))) float red_all[4][32];   // one region per reduction: no barrier in front
    float* red = red_all[0];
    const int row = blockIdx.x, j = threadIdx.x;
    const f16* xr = x + (size_t)row * H;
    float v[NI][4];
    // every load of the row first, unconditionally; the (uniform) choice between plain / delta / K-slice-partial
    // input then selects among values, not among loads: a load behind a branch costs its own round trip (hipcc waits
    // vmcnt(0) at the join), and with NI trips that was NI serialized round trips
    f16x4 xa[NI], da[NI];
    const f16* dsrc = delta ? delta : x;   // dummy re-read of x when there is no delta
#pragma unroll
    for (int it = 0; it < NI; it++) {
        xa[it] = *reinterpret_cast<const f16x4*>(xr + it * 1024 + 4 * j);
        da[it] = *reinterpret_cast<const f16x4*>(dsrc + (size_t)row * H + it * 1024 + 4 * j);
    }
    if (part) {
        // delta arrives as S raw fp32 K-slice sums of a W4A16 projection (gemm_stream_w4a16.hip, SEPI_PARTIAL):
        // delta = h((p_0 + p_1 + ...) * f(sw)), the expression of w4a16_partial_finish_kernel
        f32x4 sum[NI];
        f16x4 w4[NI];
#pragma unroll
        for (int it = 0; it < NI; it++) {
            const size_t col = (size_t)it * 1024 + 4 * j;
            sum[it] = *reinterpret_cast<const f32x4*>(part + (size_t)row * H + col);
            w4[it] = *reinterpret_cast<const f16x4*>(pws + col);
        }
        for (int s2 = 1; s2 < S; s2++) {
            f32x4 t[NI];
#pragma unroll
            for (int it = 0; it < NI; it++)
                t[it] = *reinterpret_cast<const f32x4*>(part + (size_t)s2 * pstride + (size_t)row * H + (size_t)it * 1024 + 4 * j);
#pragma unroll
            for (int it = 0; it < NI; it++)
#pragma unroll
                for (int c = 0; c < 4; c++) sum[it][c] = sum[it][c] + t[it][c];
        }
#pragma unroll
        for (int it = 0; it < NI; it++)
#pragma unroll
            for (int c = 0; c < 4; c++) da[it][c] = f2h(sum[it][c] * h2f(w4[it][c]));
    }
    if (ipart) {
        // delta arrives as S raw int32 K-slice sums of a W4A4 projection (gemm_stream_w4a4.hip, SEPI_IPART): the slices add up
        // exactly, then the GEMM's own epilogue expression: delta = h((f(i_0 + i_1 + ...) * f(xs[row])) * f(sw[col]))
        typedef int i32x4v __attribute__((ext_vector_type(4)));
        i32x4v isum[NI];
        f16x4 w4[NI];
        const float xsr = h2f(pxs[row]);
#pragma unroll
        for (int it = 0; it < NI; it++) {
            const size_t col = (size_t)it * 1024 + 4 * j;
            isum[it] = *reinterpret_cast<const i32x4v*>(ipart + (size_t)row * H + col);
            w4[it] = *reinterpret_cast<const f16x4*>(pws + col);
        }
        for (int s2 = 1; s2 < S; s2++) {
            i32x4v t[NI];
#pragma unroll
            for (int it = 0; it < NI; it++)
                t[it] = *reinterpret_cast<const i32x4v*>(ipart + (size_t)s2 * pstride + (size_t)row * H + (size_t)it * 1024 + 4 * j);
#pragma unroll
            for (int it = 0; it < NI; it++) isum[it] = isum[it] + t[it];
        }
#pragma unroll
        for (int it = 0; it < NI; it++)
#pragma unroll
            for (int c = 0; c < 4; c++) da[it][c] = f2h(((float)isum[it][c] * xsr) * h2f(w4[it][c]));
    }
    const bool has_delta = part != nullptr || ipart != nullptr || delta != nullptr;
#pragma unroll
    for (int it = 0; it < NI; it++) {
        f16x4 a = xa[it];
        if (has_delta) {
#pragma unroll
            for (int c = 0; c < 4; c++) a[c] = f2h(h2f(a[c]) + h2f(da[it][c]));
            if (hidden_out) *reinterpret_cast<f16x4*>(hidden_out + (size_t)row * H + it * 1024 + 4 * j) = a;
        }
#pragma unroll
        for (int c = 0; c < 4; c++) v[it][c] = h2f(a[c]);
    }
    float p[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        float s = 0.0f;
#pragma unroll
        for (int it = 0; it < NI; it++) s = s + v[it][c];
        p[c] = s;
    }
    // x / H for a power of two H is x * (1 / H) bit for bit (both the one correct rounding of the same real); H = 1024 NI
    constexpr bool pow2 = (NI & (NI - 1)) == 0;
    constexpr float invH = 1.0f / (float)(NI * 1024);
    const float msum = ref_tree_sum_1024(p[0], p[1], p[2], p[3], red);
    const float mean = pow2 ? msum * invH : msum / (float)H;
    // max |x - mean| rides on the variance pass: the reference's amax = max |h((x - mean) * rstd)| equals
    // |h(max|x - mean| * rstd)| bit for bit (rstd > 0, both roundings monotonic and sign-symmetric), which saves the
    // third block reduction when input_sum (a write-only output the wrapper drops) is not requested
    float dm = 0.0f;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        float s = 0.0f;
#pragma unroll
        for (int it = 0; it < NI; it++) {
            float d = v[it][c] - mean;
            s = __builtin_fmaf(d, d, s);
            dm = fmaxf(dm, __builtin_fabsf(d));
        }
        p[c] = s;
    }
    if (MODE == 0) {
        dm = wave_max_uniform(dm);
        if ((j & 63) == 0) red_all[3][j >> 6] = dm;   // published by the barrier inside the variance tree
    }
    const float vsum = ref_tree_sum_1024(p[0], p[1], p[2], p[3], red_all[1]);
    const float var = pow2 ? vsum * invH : vsum / (float)H;
    const float rstd = 1.0f / __builtin_sqrtf(var + eps);

    if (MODE == 1) {
#pragma unroll
        for (int it = 0; it < NI; it++) {
            f16x4 o;
#pragma unroll
            for (int c = 0; c < 4; c++) o[c] = f2h((v[it][c] - mean) * rstd);
            if (xp) {
                // thread j holds elements e = 4 (j & 1) .. + 3 of the 8-half group j / 2 of this trip; the group is stored in
                // the order e0 e4 e1 e5 | e2 e6 e3 e7: the even thread writes the first four, the odd one the last four,
                // after swapping two halves each with its neighbour (lane ^ 1)
                const u32 lo = __builtin_bit_cast(u32, f16x2{o[0], o[1]}), hi = __builtin_bit_cast(u32, f16x2{o[2], o[3]});
                const bool odd = j & 1;
                const u32 got = (u32)__shfl_xor((int)(odd ? lo : hi), 1, 64);       // even gets the partner's (e4, e5); odd (e2, e3)
                const f16x2 mine = __builtin_bit_cast(f16x2, odd ? hi : lo), other = __builtin_bit_cast(f16x2, got);
                const f16x4 w4 = odd ? f16x4{other[0], mine[0], other[1], mine[1]} : f16x4{mine[0], other[0], mine[1], other[1]};
                const int k0 = it * 1024 + 8 * (j >> 1);
                *reinterpret_cast<f16x4*>(out + w4a16_xperm_offset(row, k0, H) + 4 * (j & 1)) = w4;
            } else {
                *reinterpret_cast<f16x4*>(out + (size_t)row * H + it * 1024 + 4 * j) = o;
            }
        }
        return;
    }
    float sum_f = 0.0f;
    if (input_sum) {   // uniform; fp16-accumulated per-thread partials of the rounded values, as the reference keeps them
#pragma unroll
        for (int c = 0; c < 4; c++) {
            f16 s16 = (f16)0.0f;
#pragma unroll
            for (int it = 0; it < NI; it++) s16 = f2h(h2f(s16) + h2f(f2h((v[it][c] - mean) * rstd)));
            p[c] = h2f(s16);
        }
        sum_f = ref_tree_sum_1024(p[0], p[1], p[2], p[3], red_all[2]);
    }
    const float dmax = fmaxf(fmaxf(red_all[3][0], red_all[3][1]), fmaxf(red_all[3][2], red_all[3][3]));
    const f16 a16 = f2h(dmax * rstd), floor16 = f2h(1e-6f);
    const float amax = h2f(a16 > floor16 ? a16 : floor16);
    // 7 / amax (the multiplier) in the even lanes, amax / 7 (the stored scale) in the odd ones: one IEEE division
    const bool second = (j & 1) != 0;
    const float ql = (second ? amax : 7.0f) / (second ? 7.0f : amax);
    const float s = readlane_f(ql, 0);
    // |t| <= 7.21 for every finite row (gemm_stream_w4a4.hip:ln_compute has the bound), so the reference's clamp to [-8, 7]
    // never acts; round to nearest even by adding 1.5 * 2^23 (+ 8): the low mantissa nibble is q + 8 with zeros above it
    // up to bit 22 -> four nibbles spliced by three shift-or's, one xor turns the offset nibbles into two's complement
#pragma unroll
    for (int it = 0; it < NI; it++) {
        u32 b[4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            float t = ((v[it][c] - mean) * rstd) * s;
            t = t + 12582920.0f;
            asm("" : "+v"(t));
            b[c] = __builtin_bit_cast(u32, t);
        }
        u32 w = (b[1] << 4) | b[0];
        w = (b[2] << 8) | w;
        w = (b[3] << 12) | w;
        *reinterpret_cast<uint16_t*>(q + (size_t)row * (H / 2) + it * 512 + 2 * j) = (uint16_t)(w ^ 0x8888u);
    }
    if (j == 1) scale[row] = f2h(ql);
    if (j == 0 && input_sum) input_sum[row] = f2h(sum_f);
}

template <int MODE>
static int launch_ln(const f16* x, const f16* delta, f16* hidden_out, f16* out, int8_t* q, f16* scale, f16* isum,
                     float eps, int T, int H, hipStream_t st, int xp = 0) {
    if (T == 0) return 0;
    if (xp && (MODE != 1 || T > 32 || H % 128)) return -1;
#define QS_LN_CASE(NI)                                                                                        \
    case NI:                                                                                                  \
        hipLaunchKernelGGL((ln_kernel<NI, MODE>), dim3(T), dim3(256), 0, st, x, delta, hidden_out, out, q, scale, \
                           isum, eps, H, (const float*)nullptr, (const f16*)nullptr, 0, (size_t)0, (const int*)nullptr, \
                           (const f16*)nullptr, xp);                                                          \
        break;
    switch (H / 1024) {
        QS_LN_CASE(1) QS_LN_CASE(2) QS_LN_CASE(3) QS_LN_CASE(4) QS_LN_CASE(5) QS_LN_CASE(6) QS_LN_CASE(7) QS_LN_CASE(8)
        default: return -1;
    }
#undef QS_LN_CASE
    return 0;
}

int ln_quant_i4(const f16* x, const f16* delta, f16* hidden_out, int8_t* q, f16* scale, f16* isum, float eps, int T,
                int H, hipStream_t st) {
    return launch_ln<0>(x, delta, hidden_out, nullptr, q, scale, isum, eps, T, H, st);
}
int ln_fp16(const f16* x, const f16* delta, f16* hidden_out, f16* out, float eps, int T, int H, hipStream_t st, int xp) {
    return launch_ln<1>(x, delta, hidden_out, out, nullptr, nullptr, nullptr, eps, T, H, st, xp);
}
// delta = the W4A4 projection whose S int32 K-slice sums are ipart [S][T][H] (activation scales xs [T], channel scales ws [H]);
// q != nullptr: int4 output (the draft pass's next norm), else fp16 `out` (the final norm)
int ln_ipartial(const f16* x, const int* ipart, const f16* xs, const f16* ws, int S, f16* hidden_out, f16* out, int8_t* q,
                f16* scale, float eps, int T, int H, hipStream_t st) {
    if (T == 0) return 0;
    if (S < 1 || !ipart || !xs || !ws) return -1;
#define QS_LNI_CASE(NI)                                                                                              \
    case NI:                                                                                                         \
        if (q)                                                                                                       \
            hipLaunchKernelGGL((ln_kernel<NI, 0>), dim3(T), dim3(256), 0, st, x, (const f16*)nullptr, hidden_out,     \
                               (f16*)nullptr, q, scale, (f16*)nullptr, eps, H, (const float*)nullptr, ws, S,          \
                               (size_t)T * H, ipart, xs);                                                            \
        else                                                                                                         \
            hipLaunchKernelGGL((ln_kernel<NI, 1>), dim3(T), dim3(256), 0, st, x, (const f16*)nullptr, hidden_out, out, \
                               (int8_t*)nullptr, (f16*)nullptr, (f16*)nullptr, eps, H, (const float*)nullptr, ws, S,  \
                               (size_t)T * H, ipart, xs);                                                            \
        break;
    switch (H / 1024) {
        QS_LNI_CASE(1) QS_LNI_CASE(2) QS_LNI_CASE(3) QS_LNI_CASE(4) QS_LNI_CASE(5) QS_LNI_CASE(6) QS_LNI_CASE(7) QS_LNI_CASE(8)
        default: return -1;
    }
#undef QS_LNI_CASE
    return 0;
}
int ln_fp16_partial(const f16* x, const float* part, const f16* ws, int S, f16* hidden_out, f16* out, float eps, int T,
                    int H, hipStream_t st, int xp) {
    if (T == 0) return 0;
    if (S < 1 || !part || !ws) return -1;
    if (xp && (T > 32 || H % 128)) return -1;
#define QS_LNP_CASE(NI)                                                                                              \
    case NI:                                                                                                         \
        hipLaunchKernelGGL((ln_kernel<NI, 1>), dim3(T), dim3(256), 0, st, x, (const f16*)nullptr, hidden_out, out,   \
                           (int8_t*)nullptr, (f16*)nullptr, (f16*)nullptr, eps, H, part, ws, S, (size_t)T * H,      \
                           (const int*)nullptr, (const f16*)nullptr, xp);                                            \
        break;
    switch (H / 1024) {
        QS_LNP_CASE(1) QS_LNP_CASE(2) QS_LNP_CASE(3) QS_LNP_CASE(4) QS_LNP_CASE(5) QS_LNP_CASE(6) QS_LNP_CASE(7) QS_LNP_CASE(8)
        default: return -1;
    }
#undef QS_LNP_CASE
    return 0;
}

// ----------------------------------------------------------------- row absmax
// scale = h(h(amax/7) * h(clip)); q = clamp(rn_even(h(x / scale)), -8, 7); all-zero row -> NaN -> 0.
// max is order independent, so lanes take 16-byte chunks.
__global__ __launch_bounds__(256) void rowabsmax_quant_kernel(const f16* __restrict__ x, f16* __restrict__ scale,
                                                              int8_t* __restrict__ q, float clip, int K) {
    __shared__ float red[4];
    const int row = blockIdx.x, j = threadIdx.x;
    const f16* xr = x + (size_t)row * K;
    const int nvec = (K % 8 == 0) ? K / 8 : 0;  // rows are 16-byte aligned only then
    float amax = 0.0f;
    for (int i = j; i < nvec; i += 256) {
        f16x8 a = *reinterpret_cast<const f16x8*>(xr + 8 * i);
#pragma unroll
        for (int c = 0; c < 8; c++) {
            float f = __builtin_fabsf(h2f(a[c]));
            amax = f > amax ? f : amax;
        }
    }
    for (int i = nvec * 8 + j; i < K; i += 256) {
        float f = __builtin_fabsf(h2f(xr[i]));
        amax = f > amax ? f : amax;
    }
    amax = block_max_256(amax, red);
    const f16 sc = f2h(h2f(f2h(amax / 7.0f)) * h2f(f2h(clip)));
    const float scf = h2f(sc);
    const float rcf = div3_rcp(scf);   // correctly rounded reciprocal for div3_h
    if (j == 0) scale[row] = sc;
    int8_t* qr = q + (size_t)row * (K / 2);
    for (int i = j; i < nvec; i += 256) {
        f16x8 a = *reinterpret_cast<const f16x8*>(xr + 8 * i);
        uint32_t w = 0;
#pragma unroll
        for (int c = 0; c < 8; c++) {
            float d = h2f(f2h(div3_h(h2f(a[c]), rcf, scf)));
            int v = rni_sat(d, -8, 7);
            w |= (uint32_t)(v & 0xF) << (4 * c);
        }
        *reinterpret_cast<uint32_t*>(qr + 4 * i) = w;
    }
    for (int i = nvec * 4 + j; i < K / 2; i += 256) {
        int v0 = rni_sat(h2f(f2h(div3_h(h2f(xr[2 * i]), rcf, scf))), -8, 7);
        int v1 = rni_sat(h2f(f2h(div3_h(h2f(xr[2 * i + 1]), rcf, scf))), -8, 7);
        qr[i] = (int8_t)pack_nib(v0, v1);
    }
}

int rowabsmax_quant(const f16* x, f16* scale, int8_t* q, float clip, int T, int K, hipStream_t st) {
    if (T == 0) return 0;
    hipLaunchKernelGGL(rowabsmax_quant_kernel, dim3(T), dim3(256), 0, st, x, scale, q, clip, K);
    return 0;
}

}  // namespace qspec
