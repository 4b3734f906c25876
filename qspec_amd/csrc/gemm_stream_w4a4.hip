// Weight-streaming W4A4 GEMM for decode-sized M (<= 16 tokens), second generation: the kernel of the draft pass.
//
// Same arithmetic and the same shared packed-int4 weight buffer as gemm.hip:gemm_w4a4_kernel (reference:
// third-party/ao/torchao/csrc/cuda/rowwise_scaled_linear_cutlass/rowwise_scaled_linear_cutlass_unified.cuh:240-488,
// Python quarot_nn/linear.py:67-84), restructured around what bounds it at M = 4: bytes in flight and launches.
//
//   * A workgroup of NW waves (4 / 8 / 16 by K) owns 16-row weight tiles and LOOPS over them (stride gridDim.x).
//     The waves interleave over K in 64-byte steps, 8 steps (8 KiB per wave) per batch; the loads of the NEXT
//     batch -- usually the next tile -- are issued before the current one is consumed, so every wave keeps 8 KiB
//     in flight across the reduce / epilogue of a tile.  With K = 4096 and NW = 4, or K = 14336 and NW = 16, one
//     batch is one tile: all of a tile's bytes are requested at once.
//   * Activations live in LDS (int4-packed, [M][K/2 + 32]: the 32-byte pad spreads the token rows over the banks),
//     fragments are ds_read_b128 -- LDS reads count in lgkmcnt and never queue behind the weight loads in vmcnt.
//   * PRO_LN: the residual add + LayerNorm-no-gamma + per-token int4 quantisation that feeds qkv_proj / gate_up
//     (layernorm_kernels.cu:569-716, quarot_llama.py:373-388) runs as the PROLOGUE of the GEMM, redundantly in every
//     workgroup, underneath the latency of the first weight batch: the LN kernel and its launch boundary disappear.
//     It is the same arithmetic as norm_quant.hip:ln_kernel (reference reduction tree, bit for bit), batched over
//     rows.  Workgroup 0 also writes the updated residual stream (hidden_out != hidden_in: ping-pong, no race).
//     Forms: PRO_LN / PRO_LN1 (every wave of the workgroup takes part in the norm; LN1 = no delta, no write-back),
//     PRO_LNS / PRO_LN1S (M <= 4, what the draft pass launches: four extra norm waves, one row each with no barrier
//     inside, while the streaming waves already request their first two tiles), PRO_LNH (a few producer workgroups
//     hand the rows over through L2; M >= 8, not the default any more).
//   * PRO_RQ (M <= 4, K = 4096): fp16 rows + eight partial row maxima each (the spread head-Hadamard's output) -> the
//     row-absmax int4 quantiser (quant.cu:102-167: scale = h(h(amax / 7) h(clip)), q = clamp(rne(h(x / scale)), -8, 7)) in
//     the prologue of o_proj, under the latency of the workgroup's one weight tile.
//   * Epilogues as in gemm.hip (plain / RoPE + KV-cache write / silu(gate)*up), with their operands (channel
//     scale, cos/sin, position, slot) prefetched together with the tile's weights.
//   * Cross-wave K reduction through LDS in wave order: int32, exact, deterministic.
//
// Also in this file (round 3), all bit-identical to the register forms: three LDS-DMA forms of the draft GEMMs, measured and
// left OFF ("Stage A"): the loader / consumer engine (gemm_w4a4_engine_kernel, QSPEC_ENGINE=1), the
// self-service form (gemm_w4a4_sdma_kernel, QSPEC_SDMA=1..3) and loader waves beside the register stream (template parameter
// DMA of the kernel below, QSPEC_DMA_TILES=1..3).  The W4A16 and lm_head kernels on the same skeleton: gemm_stream_w4a16.hip,
// gemm_stream_f16.hip; what the three share: stream_common.cuh.
#include "stream_common.cuh"

namespace qspec {

// Reference summation tree over 1024 virtual-thread partials held 4 per lane (norm_quant.hip:ref_tree_sum_1024),
// for RB rows at once.  j = index inside the 256-thread group; red = [RB][32] floats of this group, written once.
// Same pairings, same order as the reference's two xor butterflies (so the same bits):
//   * first butterfly (virtual lane = 4 j + c): lanes ^4, ^2, ^1 as one-instruction DPP adds, the four chains of a row
//     interleaved (dpp_add_tree421_x4), then the c pairs (0,2), (1,3) and the last add in registers;
//   * second butterfly over the 32 warp sums: lane l of a wave takes warp sum l & 31 of row (l >> 5) (two rows per
//     register), and the five levels 16, 8, 4, 2, 1 run ACROSS LANES (ds_swizzle for 16, DPP adds for the rest) --
//     10 instructions for two rows where every thread used to add up all 32 sums of every row (8 broadcast
//     ds_read_b128 + 31 adds per row).  Every lane of a butterfly ends with the same value; lane 0 / 32 is read back
//     as a wave-uniform value.
template <int RB>
__device__ __forceinline__ void tree_sum_rows(float (&p)[RB][4], float* red, int j, float (&out)[RB]) {
    const int lane = j & 63;
#pragma unroll
    for (int i = 0; i < RB; i++) {
        dpp_add_tree421_x4(p[i]);
        const float r0 = p[i][0] + p[i][2], r1 = p[i][1] + p[i][3];
        const float s = r0 + r1;
        if ((j & 7) == 0) red[i * 32 + (j >> 3)] = s;
    }
    __syncthreads();
#pragma unroll
    for (int i0 = 0; i0 < RB; i0 += 2) {
        float x = red[i0 * 32 + (RB == 1 ? (lane & 31) : lane)];
        x = x + swizzle_xor16_f(x);
        x = dpp_add_xor<8>(x);
        x = dpp_add_xor<4>(x);
        x = dpp_add_xor<2>(x);
        x = dpp_add_xor<1>(x);
        out[i0] = readlane_f(x, 0);
        if (RB > 1) out[i0 + 1] = readlane_f(x, 32);
    }
}

// Residual add + LN-no-gamma + int4 quant of all M rows into LDS (xq_lds [MP][RS] bytes, xs_lds [16] floats).
// NG groups of 256 threads, RB rows per group per pass.  Split in a load half and a compute half so that the caller
// can put the first weight batch between them: vector-memory results return in issue order, so the residual
// stream must be requested BEFORE the weights for the norm to run underneath their latency.
// Arithmetic = norm_quant.hip:ln_kernel (layernorm_kernels.cu:569-716), with cheaper but bit-equivalent forms:
// |fp16| maxima compared as fp16, round-to-nearest-even to integer by adding 1.5 * 2^23.
template <int NI, int RB>
struct LnRegs {
    f16x4 x[RB][NI], d[RB][NI];
};

template <int NI, int NG, int RB, bool HASD = true>
__device__ __forceinline__ void ln_load(const StreamArgs& a, int base, LnRegs<NI, RB>& rg) {
    const int tid = threadIdx.x, j = tid & 255, grp = tid >> 8;
    const int H = a.K;
    const f16* dptr = a.delta ? a.delta : a.hidden_in;
#pragma unroll
    for (int i = 0; i < RB; i++) {
        const int row = base + grp * RB + i;
        const int rr = row < a.M ? row : 0;
#pragma unroll
        for (int it = 0; it < NI; it++) {
            // no branch around a load: hipcc answers control flow with s_waitcnt vmcnt(0), which would serialise
            // every load of the prologue (delta == nullptr re-reads hidden_in and the value is discarded)
            rg.x[i][it] = *reinterpret_cast<const f16x4*>(a.hidden_in + (size_t)rr * H + it * 1024 + 4 * j);
            if (HASD) rg.d[i][it] = *reinterpret_cast<const f16x4*>(dptr + (size_t)rr * H + it * 1024 + 4 * j);
        }
    }
}

#ifdef QS_STREAM_STAMPS
#ifdef QS_STAMPS_DRAIN   // drains vmcnt first: "the time until the residual stream has arrived" (perturbs: also waits for the weights)
#define QS_LNSTAMP(i) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(lnst[i])::"memory")
#else
#define QS_LNSTAMP(i) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(lnst[i])::"memory")
#endif
__device__ long long g_lnst[8];
#else
#define QS_LNSTAMP(i)
#endif
template <int NI, int NG, int RB, bool HASD = true>
__device__ __forceinline__ void ln_compute(const StreamArgs& a, int base, LnRegs<NI, RB>& rg,
                                           unsigned char* xq_lds, int RS, float* xs_lds,
                                           float* lnred /* [3][NG][RB][32] */, bool write_hidden) {
    static_assert(RB == 1 || RB == 2 || RB == 4, "rows per 256-thread group");
    const int tid = threadIdx.x, j = tid & 255, grp = tid >> 8, lane = tid & 63;
    const int H = a.K;
    float* red_mean = lnred + (0 * NG + grp) * RB * 32;
    float* red_var = lnred + (1 * NG + grp) * RB * 32;
    float* red_max = lnred + (2 * NG + grp) * RB * 32;
    // v[i][it][h] = elements (2h, 2h + 1) of the thread's 4-element piece: the element-wise passes run on pairs
    // (v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32: one VALU issue per two elements, each half rounded like the scalar op)
    f32x2 v[RB][NI][2];
    const int row0 = base + grp * RB;   // rows row0 .. row0 + RB - 1 (< MP <= 16: the caller's LDS rows exist even beyond M)
#ifdef QS_STREAM_STAMPS
    long long lnst[8];
#endif
    QS_LNSTAMP(0);   // (stamps build: drains vmcnt first -> the time until the residual stream has arrived)
    if (HASD && a.delta) {  // uniform; no load inside
#pragma unroll
        for (int i = 0; i < RB; i++)
#pragma unroll
            for (int it = 0; it < NI; it++)
#pragma unroll
                for (int c = 0; c < 4; c++) rg.x[i][it][c] = f2h(h2f(rg.x[i][it][c]) + h2f(rg.d[i][it][c]));
    }
#pragma unroll
    for (int i = 0; i < RB; i++) {
        const bool act = row0 + i < a.M;
        const int rr = act ? row0 + i : 0;
#pragma unroll
        for (int it = 0; it < NI; it++) {
            if (HASD && write_hidden && act)
                *reinterpret_cast<f16x4*>(a.hidden_out + (size_t)rr * H + it * 1024 + 4 * j) = rg.x[i][it];
            v[i][it][0] = f32x2{h2f(rg.x[i][it][0]), h2f(rg.x[i][it][1])};
            v[i][it][1] = f32x2{h2f(rg.x[i][it][2]), h2f(rg.x[i][it][3])};
        }
    }
    float p[RB][4], mean[RB], var[RB];
#pragma unroll
    for (int i = 0; i < RB; i++)
#pragma unroll
        for (int h = 0; h < 2; h++) {
            // (the reference starts its chain at +0: 0 + v == v except that an all -0 chain ends as +0 there and -0
            // here; a mean of -0 instead of +0 changes no deviation's magnitude and no rounded quotient)
            f32x2 s = v[i][0][h];
#pragma unroll
            for (int it = 1; it < NI; it++) s = s + v[i][it][h];
            p[i][2 * h] = s[0];
            p[i][2 * h + 1] = s[1];
        }
    tree_sum_rows<RB>(p, red_mean, j, mean);
    QS_LNSTAMP(1);
    // x / H for a power of two H is x * (1 / H) bit for bit (both are the one correct rounding of the same real)
    // (compile-time: H = 1024 NI; left to a run-time test hipcc computes the division anyway and selects)
    constexpr bool pow2 = (NI & (NI - 1)) == 0;
    constexpr float invH = 1.0f / (float)(NI > 0 ? NI * 1024 : 1);   // (NI = 0: instantiated but never run)
    // Second pass: sum of squared deviations AND max |deviation|.  The reference takes the maximum over
    // |h((x - mean) * rstd)| after the variance is known (a third block reduction); rstd > 0 and both roundings are
    // monotonic and sign-symmetric, so that maximum is |h(max|x - mean| * rstd)| bit for bit and the maximum can ride
    // on the variance pass's barrier.  The deviations replace the values in registers: the last pass needs only them.
#pragma unroll
    for (int i = 0; i < RB; i++) {
        mean[i] = pow2 ? mean[i] * invH : mean[i] / (float)H;
        const f32x2 m2 = {mean[i], mean[i]};
        float dm = 0.0f;
#pragma unroll
        for (int h = 0; h < 2; h++) {
            f32x2 s;
#pragma unroll
            for (int it = 0; it < NI; it++) {
                const f32x2 d = v[i][it][h] - m2;
                v[i][it][h] = d;
                s = it == 0 ? d * d : __builtin_elementwise_fma(d, d, s);   // fma(d, d, +0) == d * d
                dm = fmaxf(fmaxf(dm, __builtin_fabsf(d[0])), __builtin_fabsf(d[1]));
            }
            p[i][2 * h] = s[0];
            p[i][2 * h + 1] = s[1];
        }
        dm = wave_max_uniform(dm);
        if ((j & 63) == 0) red_max[i * 32 + (j >> 6)] = dm;
    }
    tree_sum_rows<RB>(p, red_var, j, var);
    QS_LNSTAMP(2);
    // Row scalars, ONE IEEE sqrt and TWO IEEE divisions per call instead of one sqrt and five divisions per row (each
    // ~11 dependent VALU instructions that every wave of every workgroup repeats): lane l works on row l % RB; lanes
    // with bit RB clear produce 7 / amax (the quantiser's multiplier), lanes with it set amax / 7 (the stored scale).
    const int li = lane & (RB - 1);
    float tv = pow2 ? var[0] * invH : var[0] / (float)H;
    tv = tv + a.eps;
    f32x4 m4 = *reinterpret_cast<const f32x4*>(red_max + li * 32);
#pragma unroll
    for (int i = 1; i < RB; i++) {
        float t = pow2 ? var[i] * invH : var[i] / (float)H;
        t = t + a.eps;
        tv = li == i ? t : tv;
    }
    const float rl = 1.0f / __builtin_sqrtf(tv);
    const float dmax = fmaxf(fmaxf(m4[0], m4[1]), fmaxf(m4[2], m4[3]));
    const f16 a16 = f2h(dmax * rl), floor16 = f2h(1e-6f);
    const float amax = h2f(a16 > floor16 ? a16 : floor16);
    const bool second = (lane & RB) != 0;
    const float ql = (second ? amax : 7.0f) / (second ? 7.0f : amax);
    if (j >= RB && j < 2 * RB) xs_lds[row0 + j - RB] = h2f(f2h(ql));
    // Last pass.  |(x - mean) * rstd| <= dmax * rstd =: y and amax >= h(y) >= y (1 - 2^-11) (fp16 normal range; below it
    // the absolute rounding error 2^-25 against the floor of 17 * 2^-24 bounds the ratio by 1.03; h(y) = inf gives s = 0),
    // so |t| <= 7.21 for every finite row and rounds into [-7, 7]: the reference's clamp to [-8, 7] never acts and is
    // not executed.  Round to nearest even by adding 1.5 * 2^23 (+ 8): the low mantissa nibble is then q + 8 in 0..15
    // with zeros above it up to bit 22, so the four nibbles of a piece are spliced with three shift-or's, no masks, and
    // one xor with 0x8888 turns the offset nibbles into two's complement.
#pragma unroll
    for (int i = 0; i < RB; i++) {
        const float rstd = readlane_f(rl, i), s = readlane_f(ql, i);
        const f32x2 r2 = {rstd, rstd}, s2 = {s, s}, mg2 = {12582920.0f, 12582920.0f};
#pragma unroll
        for (int it = 0; it < NI; it++) {
            u32 b[4];
#pragma unroll
            for (int h = 0; h < 2; h++) {
                f32x2 t = (v[i][it][h] * r2) * s2;
                t = t + mg2;
                float t0 = t[0], t1 = t[1];
                asm("" : "+v"(t0), "+v"(t1));
                b[2 * h] = __builtin_bit_cast(u32, t0);
                b[2 * h + 1] = __builtin_bit_cast(u32, t1);
            }
            u32 w = (b[1] << 4) | b[0];
            w = (b[2] << 8) | w;
            w = (b[3] << 12) | w;
            *reinterpret_cast<uint16_t*>(xq_lds + (size_t)(row0 + i) * RS + it * 512 + 2 * j) = (uint16_t)(w ^ 0x8888u);
        }
    }
    QS_LNSTAMP(3);
    __syncthreads();  // the reduction scratch is reused by the next pass; also publishes xq_lds / xs_lds
    QS_LNSTAMP(4);
#ifdef QS_STREAM_STAMPS
    if (blockIdx.x == 100 && threadIdx.x == 0 && base == 0)
        for (int i = 0; i < 5; i++) g_lnst[i] = lnst[i];
#endif
}

// ---- The same norm + quantiser with ONE WAVE PER ROW: no LDS, no barrier inside.  Lane l of the row's wave plays the
// reference's virtual threads t = 16 l + i, i = 0..15, i.e. holds the 16 CONSECUTIVE elements 1024 it + 16 l + i of every
// 1024-block `it` (two 16-byte loads per block, one 8-byte LDS store):
//   first butterfly (t ^ 16, 8, 4, 2, 1):  lane ^ 1 as DPP adds on all 16 partials, then i ^ 8, 4, 2, 1 in registers;
//   second butterfly over the 32 warp sums (warp = t >> 5 = lane >> 1; levels 16, 8, 4, 2, 1): lane ^ 32 and lane ^ 16 with
//   v_permlane32_swap / v_permlane16_swap, lane ^ 8, 4, 2 as DPP adds.
// Same pairings in the same order as ref_tree_sum_1024, every addition commutative: the same bits.  On the critical path
// of all eight waves this form is SLOWER than ln_compute (four waves x 550 instructions against eight x 430 with three
// barriers); it is what the split forms run on their four norm waves, where having no barrier is the point.
template <int NI>
struct LnwRegs {
    u32x4 x[NI > 0 ? NI : 1][2], d[NI > 0 ? NI : 1][2];
};

template <int NI, bool HASD>
__device__ __forceinline__ void lnw_load(const StreamArgs& a, int row, LnwRegs<NI>& rg) {
    const int lane = threadIdx.x & 63;
    const int rr = row < a.M ? row : 0;   // no branch around a load: clamped, the value is discarded
    const f16* xp = a.hidden_in + (size_t)rr * a.K + 16 * lane;
    const f16* dp = (a.delta ? a.delta : a.hidden_in) + (size_t)rr * a.K + 16 * lane;
#pragma unroll
    for (int it = 0; it < NI; it++)
#pragma unroll
        for (int h = 0; h < 2; h++) {
            rg.x[it][h] = *reinterpret_cast<const u32x4*>(xp + it * 1024 + 8 * h);
            if (HASD) rg.d[it][h] = *reinterpret_cast<const u32x4*>(dp + it * 1024 + 8 * h);
        }
}

__device__ __forceinline__ float lnw_tree(f32x2 (&p)[8]) {
    dpp_add_xor1_x4(p[0], p[1]);
    dpp_add_xor1_x4(p[2], p[3]);
    dpp_add_xor1_x4(p[4], p[5]);
    dpp_add_xor1_x4(p[6], p[7]);
#pragma unroll
    for (int k = 0; k < 4; k++) p[k] = p[k] + p[k + 4];
    p[0] = p[0] + p[2];
    p[1] = p[1] + p[3];
    p[0] = p[0] + p[1];
    float s = p[0][0] + p[0][1];
    s = add_xor32(s);
    s = add_xor16(s);
    s = dpp_add_xor<8>(s);
    s = dpp_add_xor<4>(s);
    s = dpp_add_xor<2>(s);
    return readlane_f(s, 0);
}

// row < a.M (the caller skips the others); the arithmetic, step for step, is ln_compute's (see there for the proofs of
// the maximum riding on the variance pass, the dead clamp and the nibble splice)
template <int NI, bool HASD>
__device__ __forceinline__ void lnw_compute(const StreamArgs& a, int row, LnwRegs<NI>& rg, unsigned char* xq_lds, int RS,
                                            float* xs_lds, bool write_hidden) {
    const int lane = threadIdx.x & 63;
    f32x2 v[NI > 0 ? NI : 1][8];
#ifdef QS_STREAM_STAMPS
    long long lnst[8];
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(lnst[0])::"memory");
    asm volatile("s_waitcnt vmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(lnst[1])::"memory");
#endif
#pragma unroll
    for (int it = 0; it < NI; it++) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            f16x8 x8 = __builtin_bit_cast(f16x8, rg.x[it][h]);
            if (HASD && a.delta) {   // uniform; no load inside
                const f16x8 d8 = __builtin_bit_cast(f16x8, rg.d[it][h]);
#pragma unroll
                for (int e = 0; e < 8; e++) x8[e] = f2h(h2f(x8[e]) + h2f(d8[e]));
            }
            if (HASD && write_hidden)
                *reinterpret_cast<u32x4*>(a.hidden_out + (size_t)row * a.K + it * 1024 + 16 * lane + 8 * h) =
                    __builtin_bit_cast(u32x4, x8);
#pragma unroll
            for (int k = 0; k < 4; k++) v[it][4 * h + k] = f32x2{h2f(x8[2 * k]), h2f(x8[2 * k + 1])};
        }
    }
    f32x2 p[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        f32x2 s = v[0][k];
#pragma unroll
        for (int it = 1; it < NI; it++) s = s + v[it][k];
        p[k] = s;
    }
    constexpr bool pow2 = (NI & (NI - 1)) == 0;
    constexpr float invH = 1.0f / (float)(NI > 0 ? NI * 1024 : 1);
    float mean = lnw_tree(p);
    QS_LNSTAMP(2);
    mean = pow2 ? mean * invH : mean / (float)a.K;
    const f32x2 m2 = {mean, mean};
    float dm = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        f32x2 s;
#pragma unroll
        for (int it = 0; it < NI; it++) {
            const f32x2 d = v[it][k] - m2;
            v[it][k] = d;
            s = it == 0 ? d * d : __builtin_elementwise_fma(d, d, s);
            dm = fmaxf(fmaxf(dm, __builtin_fabsf(d[0])), __builtin_fabsf(d[1]));
        }
        p[k] = s;
    }
    float var = lnw_tree(p);
    QS_LNSTAMP(3);
    const float dmax = wave_max_uniform(dm);
    var = pow2 ? var * invH : var / (float)a.K;
    const float rstd = 1.0f / __builtin_sqrtf(var + a.eps);
    const f16 a16 = f2h(dmax * rstd), floor16 = f2h(1e-6f);
    const float amax = h2f(a16 > floor16 ? a16 : floor16);
    // 7 / amax (the multiplier) in the even lanes, amax / 7 (the stored scale) in the odd ones: one division
    const bool second = (lane & 1) != 0;
    const float ql = (second ? amax : 7.0f) / (second ? 7.0f : amax);
    if (lane == 1) xs_lds[row] = h2f(f2h(ql));
    const float sq = readlane_f(ql, 0);
    const f32x2 r2 = {rstd, rstd}, s2 = {sq, sq}, mg2 = {12582920.0f, 12582920.0f};
#pragma unroll
    for (int it = 0; it < NI; it++) {
        u32 half[4];
#pragma unroll
        for (int q4 = 0; q4 < 4; q4++) {   // 4 elements -> 16 bits (upper bits: junk)
            u32 b[4];
#pragma unroll
            for (int h = 0; h < 2; h++) {
                f32x2 t = (v[it][2 * q4 + h] * r2) * s2;
                t = t + mg2;
                float t0 = t[0], t1 = t[1];
                asm("" : "+v"(t0), "+v"(t1));
                b[2 * h] = __builtin_bit_cast(u32, t0);
                b[2 * h + 1] = __builtin_bit_cast(u32, t1);
            }
            u32 w = (b[1] << 4) | b[0];
            w = (b[2] << 8) | w;
            half[q4] = (b[3] << 12) | w;
        }
        // bytes 0, 1 of the even piece, bytes 0, 1 of the odd piece
        u32x2 o;
        o[0] = __builtin_amdgcn_perm(half[1], half[0], 0x05040100u) ^ 0x88888888u;
        o[1] = __builtin_amdgcn_perm(half[3], half[2], 0x05040100u) ^ 0x88888888u;
        *reinterpret_cast<u32x2*>(xq_lds + (size_t)row * RS + it * 512 + 8 * lane) = o;
    }
#ifdef QS_STREAM_STAMPS
    QS_LNSTAMP(4);
    if (blockIdx.x == 100 && row == 0 && lane == 0)
        for (int i = 0; i < 5; i++) g_lnst[i] = lnst[i];
#endif
}

// NW waves; UB steps of 64 packed bytes per wave and batch (K/2 = 64 * NW * UB * NB bytes, NB batches per tile);
// NI = K / 1024 for the LN prologue (0 otherwise).
#ifdef QS_STREAM_STAMPS
__device__ long long g_sstamps[8];
__device__ long long g_wgspan[1024][2];   // per workgroup: first / last instruction of thread 0, s_memrealtime (100 MHz, chip-wide)
#define QS_SSTAMP(i) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(stamp[i])::"memory")
#else
#define QS_SSTAMP(i)
#endif
// MT = 16-token tiles per workgroup (1: M <= 16; 2: M <= 32, PRO_Q only, activation fragments kept PACKED in registers
// and widened at each use -- 8 VGPRs per step and tile would not fit beside the weight ring at 1024 threads).
// PRO_LNS / PRO_LN1S ("split", M <= 4): the workgroup has NW + 4 waves.  Waves 0 .. NW-1 are the STREAM waves: they request
// the workgroup's first 1 + PF weight tiles into registers right away and then wait; waves NW .. NW+3 are NORM waves: one
// row each (lnw_compute: no barrier inside), then they retire.  One barrier joins them.  Why: a CU holds ~32 KB of loads in
// flight and a wave that issues a load beyond that stalls AT THE ISSUE, so weight requests inside the norm's instruction
// stream stop the norm ("Measured and rejected") and HBM idled underneath it; waves that have nothing else to
// do can stall, provided no barrier of the norm waits for them.
template <int PRO>
constexpr bool pro_split() { return PRO == PRO_LNS || PRO == PRO_LN1S; }
// Tiles beyond the first that the stream waves request up front.  Measured in the engine (same box, ms per cycle): unsplit
// 7.96, split with 1 / 2 extra tiles 7.92 / 7.95; gate_up with 3 / 4 / 5 extra tiles 14.3 / 14.5 / 15.2 us per launch
// against 13.4 -- also with a vmcnt(0) between the tiles' requests (13.3 / 13.7 / 14.0 / 14.6 us for 1 / 2 / 3 / 4): the
// stream waves reach the joining barrier only when their last request has been ISSUED, i.e. when all but one of the
// requested tiles have returned, and the serial consumption of the hoard then costs more than the overlap won.
#ifndef QS_LN_PF
#define QS_LN_PF 1
#endif
// DMA > 0 (split forms, M <= 4): the workgroup's tiles 1 .. DMA are brought in by FOUR LOADER WAVES with LDS-DMA
// (global_load_lds_dwordx4 nt) from the first microsecond on, beside tile 0 in the stream waves' registers.  What bounds a
// register-streaming CU is ~32 KB of loads in flight (a wave stalls at the issue beyond that); LDS-DMA loads are not subject
// to it (scripts/micro/ldsdma.hip: four loader waves keep > 100 KB in flight and reach 7.3 TB/s over the chip), so the
// bytes of the next tiles travel underneath the norm prologue and tile 0's latency instead of behind them.  The LDS image
// of a tile is the register image (load j = stream wave j / UB, step j % UB: lane-linear, no swizzle), consumed with
// ds_read_b128.  No flags: the loaders take part in the stream waves' barriers and wait for their tile's loads
// (`s_waitcnt vmcnt`) in front of the barrier after which the tile is read -- the barrier IS the publication -- and retire.
template <int EPI>
constexpr int finish_barriers() { return (EPI == SEPI_QKV || EPI == SEPI_GATEUP) ? 2 : 1; }
template <int EPI, int PRO, int NW, int UB, int NI, int MT = 1, int DMA = 0>
__global__ __launch_bounds__(NW * 64 + (pro_split<PRO>() ? 256 : 0) + (DMA > 0 ? 256 : 0)) void gemm_w4a4_stream_kernel(StreamArgs a) {
    static_assert(MT == 1 || (PRO == PRO_Q && NW >= 8), "two token tiles: (xq, xs) input, >= 512 threads for the epilogue");
    static_assert(EPI != SEPI_IPART || PRO == PRO_Q, "K-slice partials: (xq, xs) input");
    static_assert(DMA == 0 || (pro_split<PRO>() && MT == 1 && NW * UB == 32 && DMA <= 3), "LDS-DMA tiles: split forms, 32 KiB tiles");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
#ifdef QS_STREAM_STAMPS
    long long stamp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#endif
    QS_SSTAMP(0);
#ifdef QS_STREAM_STAMPS
    long long wg_t0;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(wg_t0)::"memory");
#endif
    constexpr int NG = NW / 4;
    constexpr int RB = NW == 4 ? 4 : (NW == 8 ? 2 : 1);
    constexpr bool SPLIT = pro_split<PRO>();
    const int tid = threadIdx.x, lane = tid & 63;   // (split: the norm waves are tid >= NW * 64: no epilogue thread among them)
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int Kb = a.K >> 1, RS = Kb + 32;
    // SEPI_IPART: this workgroup's K slice starts kofs bytes into every row; rows are ldw / ldx bytes apart
    const size_t kofs = EPI == SEPI_IPART ? (size_t)blockIdx.y * Kb : 0;
    const size_t ldwb = EPI == SEPI_IPART ? (size_t)a.ldw : (size_t)Kb, ldxb = EPI == SEPI_IPART ? (size_t)a.ldx : (size_t)Kb;
    const int MP = a.M <= 4 ? 4 : (a.M <= 8 ? 8 : 16);
    unsigned char* xq_lds = smem;
    float* xs_lds = reinterpret_cast<float*>(smem + (PRO == PRO_Q ? (size_t)0 : (size_t)MP * RS));   // (xq, xs) input: no staged rows
    int* red = reinterpret_cast<int*>(xs_lds + 16);                 // [2][NW][MT][256]
    f16* ex = reinterpret_cast<f16*>(red + 2 * NW * MT * 256);       // [2][MT * 256]
    float* lnred = reinterpret_cast<float*>(ex + 2 * MT * 256);      // [3][NG][RB][32]
    const int NB = Kb / (64 * NW * UB);                              // batches per tile (exact: checked on the host)
    unsigned char* dma_lds = reinterpret_cast<unsigned char*>(lnred + 3 * NG * RB * 32);   // [DMA][32 KiB] (1 KiB aligned by the host)
    dma_lds = smem + (((size_t)(dma_lds - smem) + 1023) & ~(size_t)1023);
    if constexpr (DMA > 0) {
        if (tid >= (NW + 4) * 64) {   // ---- loader waves (wave-uniform): issue, mirror the barriers, retire
            const int lw = wave - (NW + 4);
            const int mt = (a.ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
            const int nd = min(DMA, mt - 1);   // tiles this workgroup takes through LDS
            const u32 base3 = (u32)(unsigned long long)(__attribute__((address_space(3))) unsigned char*)dma_lds;
            __builtin_amdgcn_s_barrier();   // #0 (the norm waves' row requests are out)
            for (int d = 1; d <= nd; d++) {
                const int td = blockIdx.x + d * (int)gridDim.x;
                const uint8_t* wp = a.wq + (size_t)stile_row<EPI>(td, lane & 15, a.I, a.hdl) * Kb + (lane >> 4) * 16;
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    const int j = lw + 4 * i;   // load j of the tile = (stream wave j / UB, step j % UB)
                    glds16<1>(wp + step_off<NW, UB>(j / UB, j % UB), base3 + (u32)((d - 1) * 32 + j) * 1024u);
                }
            }
            __builtin_amdgcn_s_barrier();   // #1
            for (int d = 1; d <= nd; d++) {   // the barriers of finish(tile d - 1); tile d is read behind the last of them
#pragma unroll
                for (int b2 = 0; b2 < finish_barriers<EPI>() - 1; b2++) __builtin_amdgcn_s_barrier();
                const int left = nd - d;      // tiles still allowed in flight (8 loads each)
                if (left >= 2) vmcnt_le<16>();
                else if (left == 1) vmcnt_le<8>();
                else vmcnt_le<0>();
                __builtin_amdgcn_s_barrier();
            }
            return;
        }
    }

    // epilogue thread (tid < 256) owns accumulator element (token m, tile column c)
    // epilogue thread t owns output (token m = t / 16, tile column c = t % 16): for M <= 4 that is wave 0 alone, the
    // other waves go straight back to streaming.  ridx = where the MFMA left that element in a wave's accumulators.
    const int c = tid & 15, m = tid >> 4;
    const bool ethread = m < a.M;
    const int ridx = (m >> 4) * 256 + (m & 3) * 64 + ((m >> 2) & 3) * 16 + c;   // (token tile, element) in a wave's block
    const int mc = m < a.M ? m : 0;

    // No load in this kernel sits behind a branch: hipcc resolves control flow around vector-memory operations
    // with s_waitcnt vmcnt(0), which would drain the weight stream.  Addresses are clamped instead.
    int64_t pos_m = 0, slot_m = -1;
    if (EPI == SEPI_QKV) {  // the kernel's first loads
        pos_m = a.positions[mc];
        slot_m = a.slot_mapping[mc];
    }
    struct Pre {
        f16 swn, cf, sf;
    };
    auto load_pre = [&](Pre& pre, int tile) {  // epilogue operands of (token m, column c) of `tile`
        if (EPI != SEPI_IPART) pre.swn = a.ws[stile_row<EPI>(tile, c, a.I, a.hdl)];
        if (EPI == SEPI_RESID) pre.cf = a.resid_in[(size_t)mc * a.N + tile * 16 + c];   // the residual element
        if (EPI == SEPI_QKV) stream_pre_qkv(a, tile, c, pos_m, pre.cf, pre.sf);
    };
    auto wptr = [&](int tile, int b) -> const uint8_t* {
        return a.wq + (size_t)stile_row<EPI>(tile, r, a.I, a.hdl) * ldwb + kofs + (size_t)(b * UB * NW) * 64 + g * 16;
    };
    // A wave owns the same K steps of every tile (one batch per tile: NB == 1, checked on the host), so its
    // activation fragments are widened ONCE and stay in registers: no per-step LDS read, and with (xq, xs) given
    // (PRO_Q) no LDS staging and no barrier in front of the first MFMA at all.
    const unsigned char* arow = xq_lds + (size_t)(r & (MP - 1)) * RS + g * 16;
    i32x4 af0[UB], af1[UB];
    u32x4 apk[MT][UB];   // MT == 2: packed fragments
    float xs_m = 0.0f;   // activation scale of this epilogue thread's token
    i32x4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) acc[mt] = i32x4{0, 0, 0, 0};
    auto use = [&](const u32x4& w, int b, int u) {
        const i32x4 b0 = widen16(w[0], w[1]), b1 = widen16(w[2], w[3]);
        if constexpr (MT == 1) {
            acc[0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af0[u], b0, acc[0], 0, 0, 0);
            acc[0] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af1[u], b1, acc[0], 0, 0, 0);
        } else {
#pragma unroll
            for (int mt = 0; mt < MT; mt++) {
                // the widening is loop invariant (a wave meets the same K steps in every tile): left visible, hipcc
                // hoists it and keeps 8 VGPRs per step and tile live -- spills at 1024 threads.  Opaque copies keep it here.
                // (Up to 512 threads the budget is 256 VGPRs: there the hoist is what we want -- the fragments are widened
                // once and config 3's gate_up no longer spends a third of its issue cycles re-widening them.)
                u32 p0 = apk[mt][u][0], p1 = apk[mt][u][1], p2 = apk[mt][u][2], p3 = apk[mt][u][3];
                if constexpr (NW > 8 || UB > 7) asm volatile("" : "+v"(p0), "+v"(p1), "+v"(p2), "+v"(p3));   // (8 x 8 steps: 1-4 spills)
                acc[mt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(widen16(p0, p1), b0, acc[mt], 0, 0, 0);
                acc[mt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(widen16(p2, p3), b1, acc[mt], 0, 0, 0);
            }
        }
    };
    auto finish = [&](int tile, int par, const Pre& pre) {
        int* rb = red + par * NW * MT * 256;
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
#pragma unroll
            for (int i = 0; i < 4; i++) rb[(wave * MT + mt) * 256 + i * 64 + lane] = acc[mt][i];
            acc[mt] = i32x4{0, 0, 0, 0};
        }
        __syncthreads();
        f16 hv = (f16)0.0f;
        if (ethread) {
            int sum = 0;
#pragma unroll
            for (int w2 = 0; w2 < NW; w2++) sum += rb[w2 * MT * 256 + ridx];
            if (EPI == SEPI_IPART) {   // the slice's raw sum (both operands carried a factor 16: an exact multiple of 256)
                a.ipart[((size_t)blockIdx.y * a.M + m) * a.N + tile * 16 + c] = sum >> 8;
                return;
            }
            const float v = ((float)(sum >> 8) * xs_m) * h2f(pre.swn);  // both operands carried a factor 16
            hv = f2h(v);
        }
        if (EPI == SEPI_IPART) return;
        if (EPI == SEPI_PLAIN) {
            if (ethread) a.out[(size_t)m * a.N + tile * 16 + c] = hv;
            return;
        }
        if (EPI == SEPI_RESID) {   // hidden = residual + proj_out, an fp16 add of two fp16 tensors (quarot_llama.py:380,390)
            if (ethread) a.resid_out[(size_t)m * a.N + tile * 16 + c] = f2h(h2f(pre.cf) + h2f(hv));
            return;
        }
        f16* e = ex + par * MT * 256;
        if (tid < MT * 256) e[tid] = hv;
        __syncthreads();
        if (!ethread) return;
        if constexpr (EPI == SEPI_QKV || EPI == SEPI_GATEUP)
            stream_epilogue_pair<EPI>(a, tile, m, c, hv, e[tid ^ 8], pre.cf, pre.sf, slot_m);
    };

    int tile = blockIdx.x, b = 0, par = 0;
    const int my_tiles = (a.ntiles - tile + (int)gridDim.x - 1) / (int)gridDim.x;  // >= 1: grid <= ntiles
    const int n_units = my_tiles * NB;
    u32x4 w[UB];
    Pre pre = {};
    const uint8_t* wp0 = wptr(tile, 0);
    // split forms: tiles beyond the first that the stream waves request underneath the norm (one batch per tile there)
    constexpr int PF = (SPLIT && DMA == 0) ? QS_LN_PF : 0;
    constexpr int SKIP = DMA > 0 ? DMA : PF;   // tiles behind tile 0 that do not come through `w`
    Pre dpre[DMA > 0 ? DMA : 1];
    u32x4 pfw[PF > 0 ? PF : 1][UB];
    Pre pfpre[PF > 0 ? PF : 1];

    // ---- prologue: activations -> LDS.  Their loads are issued BEFORE the first weight batch (results return in
    // issue order), the arithmetic runs underneath the weights' latency.
    if (PRO == PRO_LNH) {
        // The norm is NOT recomputed by every workgroup: the first P workgroups ("producers") each normalise and
        // quantise NG rows (one per 256-thread group) and publish the packed rows through memory; every workgroup
        // meanwhile has its first weight batch in flight, waits for the P flags and copies the M x K/2 bytes into
        // LDS.  Hand-off without fences (MI355X_MICROARCH.md, "Valid forms"): write-through (sc0 sc1) stores, every
        // storing wave drains vmcnt, workgroup barrier, one lane's flag store; the consumer's polling lane sees the
        // flags, the workgroup barrier releases the other waves, every load of the published bytes is an sc1 load.
        // The call cleans up after itself: each workgroup takes a ticket once it has read the rows, the last one
        // zeroes flags and ticket counter for the next call (launch boundary orders that against the next call).
        const int P = (a.M + NG - 1) / NG;
        int* flags = a.sync;
        int* done = a.sync + 16;
        unsigned char* xq_glob = reinterpret_cast<unsigned char*>(a.sync + 32);
        u32* xs_glob = reinterpret_cast<u32*>(xq_glob + (size_t)16 * Kb);
        if ((int)blockIdx.x < P) {
            LnRegs<NI, 1> rg;
            const int base = blockIdx.x * NG;
            ln_load<NI, NG, 1>(a, base, rg);
            ln_compute<NI, NG, 1>(a, base, rg, xq_lds, RS, xs_lds, lnred, a.hidden_out != nullptr);
            const int nrows = min(NG, a.M - base), per_row = Kb >> 3;
            for (int i = tid; i < nrows * per_row; i += NW * 64) {
                const int row = base + i / per_row, q8 = i % per_row;
                const uint64_t v = *reinterpret_cast<const uint64_t*>(xq_lds + (size_t)row * RS + q8 * 8);
                __hip_atomic_store(reinterpret_cast<uint64_t*>(xq_glob + (size_t)row * Kb + q8 * 8), v, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            }
            if (tid < nrows)
                __hip_atomic_store(&xs_glob[base + tid], __builtin_bit_cast(u32, xs_lds[base + tid]), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (tid == 0) __hip_atomic_store(&flags[blockIdx.x], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
#pragma unroll
        for (int u = 0; u < UB; u++) w[u] = wload<u32x4>(wp0 + step_off<NW, UB>(wave, u));
        load_pre(pre, tile);
        QS_SSTAMP(1);
        if (tid == 0) {
            int ok = 0;
            for (int guard = 0; guard < (1 << 22) && !ok; guard++) {   // bounded: a lost producer must not hang the GPU
                ok = 1;
                for (int i = 0; i < P; i++)
                    ok &= __hip_atomic_load(&flags[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
                if (!ok) __builtin_amdgcn_s_sleep(4);
            }
            // ... and must not pass silently either: sticky error word of the workspace (word 31), read by the host once
            // per cycle (QSpecEngine.error_flag)
            if (!ok) __hip_atomic_store(&a.sync[31], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        {
            const int per_row = Kb >> 3, total = a.M * per_row;
            constexpr int FI = 2;   // M = 4, K = 4096, 512 threads: both items of a thread in flight together
            uint64_t v[FI];
            int off[FI];
#pragma unroll
            for (int f = 0; f < FI; f++) {
                const int i = min(tid + f * NW * 64, total - 1);
                const int row = i / per_row, q8 = i - row * per_row;
                off[f] = row * RS + q8 * 8;
                v[f] = __hip_atomic_load(reinterpret_cast<const uint64_t*>(xq_glob + (size_t)row * Kb + q8 * 8),
                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            const u32 xsb = __hip_atomic_load(&xs_glob[tid < a.M ? tid : 0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int f = 0; f < FI; f++) *reinterpret_cast<uint64_t*>(xq_lds + off[f]) = v[f];
            for (int i = tid + FI * NW * 64; i < total; i += NW * 64) {
                const int row = i / per_row, q8 = i - row * per_row;
                *reinterpret_cast<uint64_t*>(xq_lds + (size_t)row * RS + q8 * 8) =
                    __hip_atomic_load(reinterpret_cast<const uint64_t*>(xq_glob + (size_t)row * Kb + q8 * 8),
                                      __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (tid < a.M) xs_lds[tid] = __builtin_bit_cast(float, xsb);
        }
        __syncthreads();
        if (tid == 0) {
            const int ticket = __hip_atomic_fetch_add(done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (ticket == (int)gridDim.x - 1) {
                for (int i = 0; i < P; i++) __hip_atomic_store(&flags[i], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(done, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    } else if (PRO == PRO_RQ) {
        // thread tid owns the 16-byte chunks tid, tid + 512, ... of every row (K = 4096: 512 chunks per row = the 512
        // threads; K = 5120: 640 chunks, the first 128 threads take a second one)
        constexpr int NCH = NI * 128;                          // 16-byte chunks of a row (K = 1024 NI)
        constexpr int CPT = (NCH + NW * 64 - 1) / (NW * 64);   // chunks per thread
        u32x4 xr[4][CPT];
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int cc = 0; cc < CPT; cc++)   // (clamped: no branch around a load; a clamped chunk is never stored)
                xr[i][cc] = *reinterpret_cast<const u32x4*>(a.x16 + (size_t)min(i, a.M - 1) * a.K + 8 * min(tid + cc * NW * 64, NCH - 1));
        float pv = a.part_amax[min(lane & 31, a.M * 8 - 1)];   // lanes 8 r .. 8 r + 7: the eight partial maxima of row r
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();   // every wave's row requests before any weight request (in-order L1, see PRO_LN)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < UB; u++) w[u] = wload<u32x4>(wp0 + step_off<NW, UB>(wave, u));
        __builtin_amdgcn_sched_barrier(0);
        load_pre(pre, tile);
        __builtin_amdgcn_sched_barrier(0);
        pv = dpp_max_xor<1>(pv);
        pv = dpp_max_xor<2>(pv);
        pv = dpp_max_xor<4>(pv);
        // scale = h(h(amax / 7) * h(clip)) and its correctly rounded reciprocal, lane-parallel (lane 8 r works on row r)
        const f16 scl = f2h(h2f(f2h(pv / 7.0f)) * h2f(f2h(a.clip)));
        const float scfl = h2f(scl), rcfl = div3_rcp(scfl);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float scf = readlane_f(scfl, 8 * i), rcf = readlane_f(rcfl, 8 * i);
#pragma unroll
            for (int cc = 0; cc < CPT; cc++) {
                const f16x8 x8 = __builtin_bit_cast(f16x8, xr[i][cc]);
                // rni_sat(h(x / scale), -8, 7) as: clamp, then round to nearest even by adding 1.5 * 2^23 -- the two's
                // complement integer is the low mantissa bits.  (No quotient is NaN: with a scale of 0 div3_rcp makes div3_h
                // give +-inf for x != 0, which clamps to +7 / -8 as the reference's x / 0 does, and 0 for x = 0.)
                u32 pk = 0;
#pragma unroll
                for (int c = 0; c < 8; c++) {
                    float dq = h2f(f2h(div3_h(h2f(x8[c]), rcf, scf)));
                    dq = __builtin_amdgcn_fmed3f(dq, -8.0f, 7.0f);
                    float mg = dq + 12582912.0f;
                    asm("" : "+v"(mg));
                    pk |= (__builtin_bit_cast(u32, mg) & 0xFu) << (4 * c);
                }
                const int ch = tid + cc * NW * 64;
                if (i < a.M && (CPT * NW * 64 == NCH || ch < NCH)) *reinterpret_cast<u32*>(xq_lds + (size_t)i * RS + 4 * ch) = pk;
            }
            if (i < a.M && tid == 0) xs_lds[i] = scf;
        }
        __syncthreads();   // publishes xq_lds / xs_lds
    } else if (SPLIT) {
        constexpr bool HASD = PRO == PRO_LNS;
        if (tid >= NW * 64) {   // ---- norm waves (wave-uniform branch): row = wave - NW, then retire
            const int row = wave - NW;
            LnwRegs<NI> rg;
            lnw_load<NI, HASD>(a, row, rg);
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_barrier();   // #0: every row request is out before any weight request (in-order L1)
            __builtin_amdgcn_sched_barrier(0);
            if (row < a.M) lnw_compute<NI, HASD>(a, row, rg, xq_lds, RS, xs_lds, blockIdx.x == 0 && a.hidden_out != nullptr);
            __syncthreads();                // #1: publishes xq_lds / xs_lds
            return;                         // retired waves leave the workgroup's later barriers
        }
        __builtin_amdgcn_s_barrier();       // #0
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < UB; u++) w[u] = wload<u32x4>(wp0 + step_off<NW, UB>(wave, u));
        __builtin_amdgcn_sched_barrier(0);
        load_pre(pre, tile);
        __builtin_amdgcn_sched_barrier(0);
        // The next PF tiles, where the workgroup has them (uniform branches around loads cost nothing HERE: a CU holds one
        // tile's worth of loads in flight, so tile d + 1 could not be requested before tile d has returned anyway, and
        // this wave has nothing to do but wait).
#pragma unroll
        for (int d = 1; d <= PF; d++) {
            if (d < my_tiles) {
                const uint8_t* wpd = wptr(tile + d * (int)gridDim.x, 0);
#pragma unroll
                for (int u = 0; u < UB; u++) pfw[d - 1][u] = wload<u32x4>(wpd + step_off<NW, UB>(wave, u));
                load_pre(pfpre[d - 1], tile + d * (int)gridDim.x);
            }
        }
        if constexpr (DMA > 0) {
#pragma unroll
            for (int d = 1; d <= DMA; d++)   // (clamped: no branch around a load; unused beyond my_tiles)
                load_pre(dpre[d - 1], min(tile + d * (int)gridDim.x, a.ntiles - 1));
        }
        __builtin_amdgcn_sched_barrier(0);
        QS_SSTAMP(1);
        // #1 (a bare barrier: __syncthreads() is fine too, the loads above are what this wave waits for next anyway; the
        // norm waves drained their LDS writes in front of theirs, the clobber keeps this wave's LDS reads behind it)
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
    } else if (PRO == PRO_LN || PRO == PRO_LN1) {
        constexpr bool HASD = PRO == PRO_LN;
        LnRegs<NI, RB> rg;
        ln_load<NI, NG, RB, HASD>(a, 0, rg);
        __builtin_amdgcn_sched_barrier(0);
        // The CU's vector L1 returns data in request order ACROSS waves, and its address path takes the eight waves' row
        // requests one by one (~1 k cycles from the first to the last; the waves themselves start within 30 cycles of
        // each other, scripts/micro/wave_start.hip): a wave whose (L2-resident) rows were requested behind an earlier
        // wave's weight loads gets them only when those HBM misses have returned, and the norm's first barrier waited
        // ~2.5 k cycles for that wave (in-kernel stamps).  So: every wave's row requests first (a bare barrier, no
        // memory wait), then the weights.
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < UB; u++) w[u] = wload<u32x4>(wp0 + step_off<NW, UB>(wave, u));
        __builtin_amdgcn_sched_barrier(0);   // (else hipcc hoists load_pre's wait for the position load above the weight loads)
        load_pre(pre, tile);
        __builtin_amdgcn_sched_barrier(0);
        const bool wh = blockIdx.x == 0 && a.hidden_out != nullptr;
        QS_SSTAMP(1);
        ln_compute<NI, NG, RB, HASD>(a, 0, rg, xq_lds, RS, xs_lds, lnred, wh);
        for (int base = NG * RB; base < a.M; base += NG * RB) {
            ln_load<NI, NG, RB, HASD>(a, base, rg);
            ln_compute<NI, NG, RB, HASD>(a, base, rg, xq_lds, RS, xs_lds, lnred, wh);
        }
    } else {
        u32x4 araw[UB];
        const unsigned char* xrow = reinterpret_cast<const unsigned char*>(a.xq) + (size_t)(r < a.M ? r : 0) * ldxb + kofs + g * 16;
#pragma unroll
        for (int u = 0; u < UB; u++) araw[u] = *reinterpret_cast<const u32x4*>(xrow + step_off<NW, UB>(wave, u));
        if constexpr (MT > 1) {
#pragma unroll
            for (int mt = 0; mt < MT; mt++) {
                const int row = mt * 16 + r;
                const unsigned char* xr = reinterpret_cast<const unsigned char*>(a.xq) + (size_t)(row < a.M ? row : 0) * ldxb + kofs + g * 16;
#pragma unroll
                for (int u = 0; u < UB; u++) apk[mt][u] = *reinterpret_cast<const u32x4*>(xr + step_off<NW, UB>(wave, u));
            }
        }
        f16 xsh = (f16)0.0f;
        if (EPI != SEPI_IPART) xsh = a.xs[mc];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < UB; u++) w[u] = wload<u32x4>(wp0 + step_off<NW, UB>(wave, u));
        __builtin_amdgcn_sched_barrier(0);   // (else hipcc hoists load_pre's wait for the position load above the weight loads)
        load_pre(pre, tile);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < UB; u++) {
            af0[u] = widen16(araw[u][0], araw[u][1]);
            af1[u] = widen16(araw[u][2], araw[u][3]);
        }
        xs_m = h2f(xsh);
    }
    if (PRO != PRO_Q) {   // the norm left the packed rows in LDS: take this wave's fragments out once
#pragma unroll
        for (int u = 0; u < UB; u++) {
            const u32x4 av = *reinterpret_cast<const u32x4*>(arow + step_off<NW, UB>(wave, u));
            af0[u] = widen16(av[0], av[1]);
            af1[u] = widen16(av[2], av[3]);
        }
        xs_m = xs_lds[mc];
    }

    // ---- main loop: one unit = UB steps of every wave.  Each step's register is refilled with the same step of
    // the NEXT unit as soon as it has been consumed: UB loads per wave stay in flight across tile boundaries,
    // reductions and epilogues.  The last unit is peeled (nothing to refill), so the loop body has no branch
    // around a load and the waits hipcc inserts are the exact counted ones.
    QS_SSTAMP(2);
    int n_left = n_units;
    if constexpr (SKIP > 0) {   // split forms (one batch per tile): tile 0 from w, tiles 1 .. SKIP from registers / from LDS
        {
            const bool more = SKIP + 1 < my_tiles;   // uniform
            const int tn = tile + (SKIP + 1) * (int)gridDim.x;
            Pre npre = pre;
            if (more) load_pre(npre, tn);          // (a branch around loads: everything in flight has arrived by now)
#pragma unroll
            for (int u = 0; u < UB; u++) use(w[u], 0, u);
            if (more) {
                const uint8_t* wp = wptr(tn, 0);
#pragma unroll
                for (int u = 0; u < UB; u++) w[u] = wload<u32x4>(wp + step_off<NW, UB>(wave, u));
            }
            finish(tile, par, pre);
            par ^= 1;
            pre = npre;
        }
        if constexpr (DMA > 0) {
#pragma unroll
            for (int d = 1; d <= DMA; d++) {
                if (d < my_tiles) {   // uniform.  Tile d has landed: the loaders waited for it in front of the last barrier
                    const unsigned char* tl = dma_lds + (size_t)((d - 1) * 32 + wave * UB) * 1024 + lane * 16;
                    u32x4 lw4[UB];
#pragma unroll
                    for (int u = 0; u < UB; u++) lw4[u] = *reinterpret_cast<const u32x4*>(tl + u * 1024);
#pragma unroll
                    for (int u = 0; u < UB; u++) use(lw4[u], 0, u);
                    finish(tile + d * (int)gridDim.x, par, dpre[d - 1]);
                    par ^= 1;
                }
            }
        } else {
#pragma unroll
            for (int d = 1; d <= PF; d++) {
                if (d < my_tiles) {   // uniform; no load inside
#pragma unroll
                    for (int u = 0; u < UB; u++) use(pfw[d - 1][u], 0, u);
                    finish(tile + d * (int)gridDim.x, par, pfpre[d - 1]);
                    par ^= 1;
                }
            }
        }
        tile += (SKIP + 1) * (int)gridDim.x;
        n_left = my_tiles - (SKIP + 1);
    }
    if (SKIP == 0 || n_left > 0) {
    for (int q = 0; q < n_left - 1; q++) {
        int nb = b + 1, nt = tile;
        if (nb == NB) {
            nb = 0;
            nt = tile + gridDim.x;
        }
        const uint8_t* wp = wptr(nt, nb);
        Pre npre;
        load_pre(npre, nt);
#pragma unroll
        for (int u = 0; u < UB; u++) {
            use(w[u], b, u);
            // pin the refill right behind its consumer: left alone, the scheduler sinks all UB loads below the last
            // use and the stream drains every unit
            __builtin_amdgcn_sched_barrier(0);
            w[u] = wload<u32x4>(wp + step_off<NW, UB>(wave, u));
            __builtin_amdgcn_sched_barrier(0);
        }
        if (b == NB - 1) {
            finish(tile, par, pre);
            par ^= 1;
        }
        pre = npre;
        tile = nt;
        b = nb;
    }
    QS_SSTAMP(3);
#pragma unroll
    for (int u = 0; u < UB; u++) use(w[u], b, u);
    QS_SSTAMP(4);
    finish(tile, par, pre);
    }
    QS_SSTAMP(5);
#ifdef QS_STREAM_STAMPS
    if (PRO != PRO_Q && a.hidden_out && blockIdx.x == 100 && tid == 0) {  // debug build only: stamps into the tail of hidden_out
        long long* sb = reinterpret_cast<long long*>(a.hidden_out + (size_t)a.M * a.K) - 8;
        for (int i = 0; i < 6; i++) sb[i] = stamp[i];
        long long* sb2 = sb - 8;
        for (int i = 0; i < 5; i++) sb2[i] = g_lnst[i];
    }
    // forms without a hidden_out (LN1 / LN1S gate_up): into a device array read back by qspec_debug_stamps()
    if (EPI == SEPI_GATEUP && !a.hidden_out && blockIdx.x == 100 && tid == 0)
        for (int i = 0; i < 6; i++) g_sstamps[i] = stamp[i];
    if (EPI == SEPI_GATEUP && !a.hidden_out && tid == 0 && blockIdx.x < 1024) {
        long long t1;
        asm volatile("s_waitcnt vmcnt(0)\n\ts_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t1)::"memory");
        g_wgspan[blockIdx.x][0] = wg_t0;
        g_wgspan[blockIdx.x][1] = t1;
    }
#endif
}

// ------------------------------------------------------------------ long rows: several batches per tile
// K = 28672 (Llama-3-70B's down_proj: 224 steps of 64 bytes per weight row) does not fit the one-batch-per-tile kernel above:
// 16 waves x 14 steps would hold 112 VGPRs of widened activation fragments per lane against a budget of 128 at 1024 threads.
// Here a tile is NB batches of NW x UB steps; a wave keeps its activation fragments PACKED (4 VGPRs per step and batch,
// widened at the use: 8 VALU beside the 2 MFMAs of a step -- this kernel's waves wait for memory 90 % of their cycles) and
// refills each weight register with the same step of the NEXT batch -- the next tile's first batch behind the last one --
// right behind its consumer, so UB KiB per wave stay in flight across tile boundaries exactly as above.  (xq, xs) input,
// M <= 16, plain / residual epilogue; same int32 sums, same epilogue expression, same bits as gemm.hip's kernel.
template <int EPI, int NW, int UB, int NB>
__global__ __launch_bounds__(NW * 64) void gemm_w4a4_longk_kernel(StreamArgs a) {
    static_assert(EPI == SEPI_PLAIN || EPI == SEPI_RESID, "epilogues built so far");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    int* red = reinterpret_cast<int*>(smem);   // [2][NW][256]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int Kb = a.K >> 1;
    const int c = tid & 15, m = tid >> 4;
    const bool ethread = m < a.M;
    const int ridx = (m & 3) * 64 + ((m >> 2) & 3) * 16 + c;
    const int mc = m < a.M ? m : 0;
    constexpr int BB = UB * NW * 64;           // bytes of a weight row per batch
    struct Pre {
        f16 swn, cf;
    };
    auto load_pre = [&](Pre& pre, int tile) {
        pre.swn = a.ws[tile * 16 + c];
        if (EPI == SEPI_RESID) pre.cf = a.resid_in[(size_t)mc * a.N + tile * 16 + c];
    };
    auto wptr = [&](int tile, int b) -> const uint8_t* { return a.wq + (size_t)(tile * 16 + r) * Kb + (size_t)b * BB + g * 16; };
    u32x4 apk[NB][UB];
    {
        const unsigned char* xrow = reinterpret_cast<const unsigned char*>(a.xq) + (size_t)(r < a.M ? r : 0) * Kb + g * 16;
#pragma unroll
        for (int b = 0; b < NB; b++)
#pragma unroll
            for (int u = 0; u < UB; u++) apk[b][u] = *reinterpret_cast<const u32x4*>(xrow + (size_t)b * BB + step_off<NW, UB>(wave, u));
    }
    const f16 xsh = a.xs[mc];
    __builtin_amdgcn_sched_barrier(0);
    int tile = blockIdx.x, par = 0;
    const int my_tiles = (a.ntiles - tile + (int)gridDim.x - 1) / (int)gridDim.x;
    u32x4 w[UB];
    Pre pre = {};
    {
        const uint8_t* wp0 = wptr(tile, 0);
#pragma unroll
        for (int u = 0; u < UB; u++) w[u] = wload<u32x4>(wp0 + step_off<NW, UB>(wave, u));
    }
    __builtin_amdgcn_sched_barrier(0);
    load_pre(pre, tile);
    __builtin_amdgcn_sched_barrier(0);
    const float xs_m = h2f(xsh);
    i32x4 acc = {0, 0, 0, 0};
    auto use = [&](const u32x4& wv, const u32x4& av) {
        u32 p0 = av[0], p1 = av[1], p2 = av[2], p3 = av[3];
        asm volatile("" : "+v"(p0), "+v"(p1), "+v"(p2), "+v"(p3));   // (keeps hipcc from hoisting the loop-invariant widening)
        acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(widen16(p0, p1), widen16(wv[0], wv[1]), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(widen16(p2, p3), widen16(wv[2], wv[3]), acc, 0, 0, 0);
    };
    auto finish = [&](int tile, int par, const Pre& pre) {
        int* rb = red + par * NW * 256;
#pragma unroll
        for (int i = 0; i < 4; i++) rb[wave * 256 + i * 64 + lane] = acc[i];
        acc = i32x4{0, 0, 0, 0};
        __syncthreads();
        if (!ethread) return;
        int sum = 0;
#pragma unroll
        for (int w2 = 0; w2 < NW; w2++) sum += rb[w2 * 256 + ridx];
        const f16 hv = f2h(((float)(sum >> 8) * xs_m) * h2f(pre.swn));   // both operands carried a factor 16
        if (EPI == SEPI_PLAIN) a.out[(size_t)m * a.N + tile * 16 + c] = hv;
        else a.resid_out[(size_t)m * a.N + tile * 16 + c] = f2h(h2f(pre.cf) + h2f(hv));
    };
    for (int q = 0; q < my_tiles - 1; q++) {
        const int nt = tile + (int)gridDim.x;
        Pre npre;
        load_pre(npre, nt);
#pragma unroll
        for (int b = 0; b < NB; b++) {
            const uint8_t* wp = b + 1 < NB ? wptr(tile, b + 1) : wptr(nt, 0);
#pragma unroll
            for (int u = 0; u < UB; u++) {
                use(w[u], apk[b][u]);
                __builtin_amdgcn_sched_barrier(0);   // the refill right behind its consumer (see the kernel above)
                w[u] = wload<u32x4>(wp + step_off<NW, UB>(wave, u));
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        finish(tile, par, pre);
        par ^= 1;
        pre = npre;
        tile = nt;
    }
#pragma unroll
    for (int b = 0; b < NB; b++) {   // the last tile: nothing to refill behind its last batch
#pragma unroll
        for (int u = 0; u < UB; u++) {
            use(w[u], apk[b][u]);
            if (b + 1 < NB) {
                __builtin_amdgcn_sched_barrier(0);
                w[u] = wload<u32x4>(wptr(tile, b + 1) + step_off<NW, UB>(wave, u));
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    finish(tile, par, pre);
}

static bool longk_shape(int K) { return K == 28672; }   // 224 steps = 16 waves x 7 steps x 2 batches
template <int EPI>
static int launch_longk(const StreamArgs& a, hipStream_t st) {
    if (a.M < 1 || a.M > 16 || !longk_shape(a.K)) return -1;
    const int grid = stream_grid(a.ntiles, stream_cap());
    hipLaunchKernelGGL((gemm_w4a4_longk_kernel<EPI, 16, 7, 2>), dim3(grid), dim3(16 * 64), (size_t)2 * 16 * 1024, st, a);
    return 0;
}

#ifdef QS_EXPERIMENTAL
#include "experimental/w4a4_engine.inc"   // loader / consumer ("engine") form of the draft GEMMs: QSPEC_ENGINE=1
#include "experimental/w4a4_sdma.inc"     // self-service LDS-DMA form of the draft GEMMs: QSPEC_SDMA=1..3
#endif

// Shape classes, each table once: the predicates below and the launch switches both walk them, so a new K is ONE line.
// X(NW, UB, TWO): K / 128 = NW * UB steps of 64 packed bytes, one batch per tile (the activation fragments of a wave's K slice
// live in registers); TWO = the class also exists with two token tiles (17..32 tokens: >= 512 threads for the epilogue).
// K = 4096, 14336, 8192, 5120, 2048, 1024, 3584, 13824 (Llama-2-13B's down_proj), 5632 (TinyLlama's)
#define QS_W4A4_SHAPES(X) X(8, 4, 1) X(16, 7, 1) X(8, 8, 1) X(8, 5, 1) X(4, 4, 0) X(4, 2, 0) X(4, 7, 0) X(12, 9, 1) X(4, 11, 0)
// LN prologue: the reference's 1024 virtual threads -> K a multiple of 1024.  X(K, NW, UB, NI = K / 1024, SPLIT): SPLIT = the
// split forms (PRO_LNS / PRO_LN1S) exist (K = 8192: the row-wave's 128 values per lane do not fit 168 VGPRs).
#define QS_LN_SHAPES(X) X(4096, 8, 4, 4, 1) X(8192, 8, 8, 8, 0) X(5120, 8, 5, 5, 1) X(2048, 4, 4, 2, 1) X(1024, 4, 2, 1, 1)

struct StreamShape {
    int NW, UB;
    bool two_tiles;
};
static bool stream_shape(int K, StreamShape* sh) {
    if (K % 128) return false;
#define X(NWV, UBV, TWO) if (K / 128 == NWV * UBV) { *sh = StreamShape{NWV, UBV, TWO != 0}; return true; }
    QS_W4A4_SHAPES(X)
#undef X
    return false;
}
static bool ln_shape(int K, bool split = false) {   // split: ... and the split forms exist
#define X(KV, NWV, UBV, NIV, SPLITV) if (K == KV) return !split || SPLITV;
    QS_LN_SHAPES(X)
#undef X
    return false;
}

static size_t stream_lds_bytes(int M, int K, int NW, bool staged_rows, int MT) {
    const int MP = M <= 4 ? 4 : (M <= 8 ? 8 : 16);
    const int NG = NW / 4, RB = NW == 4 ? 4 : (NW == 8 ? 2 : 1);
    return (staged_rows ? (size_t)MP * (K / 2 + 32) : 0) + 64 + (size_t)2 * NW * MT * 1024 + (size_t)MT * 1024 +
           (size_t)3 * NG * RB * 32 * 4;
}

template <int EPI, int PRO, int NW, int UB, int NI, int MT = 1, int DMA = 0>
static int launch_stream_inst(const StreamArgs& a, hipStream_t st) {
    const size_t lds = stream_lds_bytes(a.M, a.K, NW, PRO != PRO_Q, MT) + (DMA > 0 ? 1024 + (size_t)DMA * 32768 : 0);
    if (lds > 160 * 1024) return -7;
    if (const int rc = lds_optin<gemm_w4a4_stream_kernel<EPI, PRO, NW, UB, NI, MT, DMA>>(lds)) return rc;
    int cap = stream_cap();
    if (PRO == PRO_LNH && cap > 256) cap = 256;   // the fence-free hand-off is calibrated for one workgroup per CU
    const int slices = EPI == SEPI_IPART ? a.nq : 1;   // (nq carries the slice count for SEPI_IPART)
    if (slices > 1) cap = cap / slices > 0 ? cap / slices : 1;   // one workgroup per CU in total
    hipLaunchKernelGGL((gemm_w4a4_stream_kernel<EPI, PRO, NW, UB, NI, MT, DMA>), dim3(stream_grid(a.ntiles, cap), slices),
                       dim3(NW * 64 + (pro_split<PRO>() ? 256 : 0) + (DMA > 0 ? 256 : 0)), lds, st, a);
    return 0;
}

// (dev knob QSPEC_LN_SPLIT=0: the norm on the streaming waves themselves)
static bool ln_split() {
    static const int v = QS_DEV_KNOB("QSPEC_LN_SPLIT", 1);
    return v != 0;
}

// The prologue form of a launch.  (xq, xs) given: PRO_Q.  Norm prologue: PRO_LNH with a hand-off workspace; else the pure norm
// of hidden_in (no delta, no write-back: half the prologue loads) or the residual form, each as the split form at M <= 4
// where the K has one and as the form with the norm on the streaming waves otherwise.
// (pure norm with 16 waves instead of 8 at M <= 4 -- one row per 256-thread group, 4 waves per SIMD -- measured equal: qkv 9.4
// vs 9.1 us, gate_up 15.4 vs 15.6; the prologue is bound by the CU's VALU issue, not by one wave's latency chain)
static int stream_form(const StreamArgs& a, bool ln) {
    if (!ln) return PRO_Q;
    if (a.sync) return PRO_LNH;   // producers + hand-off
    const bool pure = !a.delta && !a.hidden_out;
    const bool split = a.M <= 4 && ln_split() && ln_shape(a.K, true);
    if (pure) return split ? PRO_LN1S : PRO_LN1;
    return split ? PRO_LNS : PRO_LN;
}

// The measured-and-rejected routes (experimental library only), tried in front of the tables: the loader / consumer engine,
// the self-service LDS-DMA form, loader waves beside the register stream.  QS_NO_ROUTE: none applies, walk the table.
constexpr int QS_NO_ROUTE = 1;
#ifdef QS_EXPERIMENTAL
// QSPEC_DMA_TILES=0..3: tiles behind the first that a multi-tile workgroup takes through LDS-DMA.  Default 0: 1 tile gains
// 0.6 us on back-to-back gate_up launches (12.9 against 13.5), 2 / 3 tiles lose (13.45 / 13.75): round 3
static int dma_tiles() {
    static const int v = QS_DEV_KNOB("QSPEC_DMA_TILES", 0);
    return (v < 0 || v > 3) ? 0 : v;
}
template <int EPI>
static int launch_stream_experimental(const StreamArgs& a, int pro, hipStream_t st) {
    if (a.K == 14336 && pro == PRO_Q) {
        if constexpr (EPI == SEPI_RESID)
            if (a.M <= 4 && a.ntiles <= 256 && engine_on()) return launch_engine_inst<EPI, PRO_Q, 0, 7, 7>(a, st);
    }
    if (a.K != 4096) return QS_NO_ROUTE;
    if (pro == PRO_LN1S) {   // the three LDS-DMA forms (Stage A: measured, none is the default)
        if constexpr (EPI == SEPI_GATEUP)
            if (engine_on()) return launch_engine_inst<EPI, PRO_LN1S, 4, 2, 8>(a, st);
        if constexpr (EPI == SEPI_GATEUP || EPI == SEPI_QKV)
            if (sdma_on<EPI>()) return launch_sdma_inst<EPI, PRO_LN1S, 4, QS_SDMA_R>(a, st);
        if (a.ntiles > 256) {   // several tiles per workgroup: the next ones through LDS-DMA
            const int dt = dma_tiles();
            if (dt == 3) return launch_stream_inst<EPI, PRO_LN1S, 8, 4, 4, 1, 3>(a, st);
            if (dt == 2) return launch_stream_inst<EPI, PRO_LN1S, 8, 4, 4, 1, 2>(a, st);
            if (dt == 1) return launch_stream_inst<EPI, PRO_LN1S, 8, 4, 4, 1, 1>(a, st);
        }
    }
    if (pro == PRO_LNS) {
        if constexpr (EPI == SEPI_GATEUP || EPI == SEPI_QKV)
            if (sdma_on<EPI>()) return launch_sdma_inst<EPI, PRO_LNS, 4, QS_SDMA_R>(a, st);
    }
    return QS_NO_ROUTE;
}
#else
template <int EPI>
static int launch_stream_experimental(const StreamArgs&, int, hipStream_t) { return QS_NO_ROUTE; }
#endif

// one table walk per form: (xq, xs) input with MT token tiles / norm prologue PRO
template <int EPI, int MT>
static int launch_stream_q(const StreamArgs& a, hipStream_t st) {
#define X(NWV, UBV, TWO) \
    if constexpr (MT == 1 || TWO) if (a.K / 128 == NWV * UBV) return launch_stream_inst<EPI, PRO_Q, NWV, UBV, 0, MT>(a, st);
    QS_W4A4_SHAPES(X)
#undef X
    return -1;
}
template <int EPI, int PRO>
static int launch_stream_ln(const StreamArgs& a, hipStream_t st) {
#define X(KV, NWV, UBV, NIV, SPLITV) \
    if constexpr (SPLITV || !pro_split<PRO>()) if (a.K == KV) return launch_stream_inst<EPI, PRO, NWV, UBV, NIV>(a, st);
    QS_LN_SHAPES(X)
#undef X
    return -1;
}
template <int EPI>
static int launch_stream(const StreamArgs& a, bool ln, hipStream_t st) {
    StreamShape sh;
    if (a.M < 1 || a.M > 32 || !stream_shape(a.K, &sh)) return -1;
    if (a.M > 16) return ln ? -1 : launch_stream_q<EPI, 2>(a, st);   // two token tiles: (xq, xs) input only
    const int pro = stream_form(a, ln);
    if (const int rc = launch_stream_experimental<EPI>(a, pro, st); rc != QS_NO_ROUTE) return rc;
    switch (pro) {
        case PRO_Q: return launch_stream_q<EPI, 1>(a, st);
        case PRO_LNH: return launch_stream_ln<EPI, PRO_LNH>(a, st);
        case PRO_LN1S: return launch_stream_ln<EPI, PRO_LN1S>(a, st);
        case PRO_LN1: return launch_stream_ln<EPI, PRO_LN1>(a, st);
        case PRO_LNS: return launch_stream_ln<EPI, PRO_LNS>(a, st);
        default: return launch_stream_ln<EPI, PRO_LN>(a, st);
    }
}

size_t gemm_w4a4_stream_sync_bytes() { return 32 * sizeof(int) + (size_t)16 * (8192 / 2) + 16 * sizeof(float) + 64; }

bool gemm_w4a4_stream_supported(int M, int N, int K, bool ln) {
    StreamShape sh;
    if (!ln && M >= 1 && M <= 16 && N % 16 == 0 && longk_shape(K)) return true;   // several batches per tile (longk kernel)
    if (M < 1 || M > 32 || N % 16 || K > (1 << 19) || !stream_shape(K, &sh)) return false;
    if (M > 16 && (ln || !sh.two_tiles)) return false;   // two token tiles: (xq, xs) input only
    if (ln && !ln_shape(K)) return false;
    return stream_lds_bytes(M, K, sh.NW, ln, M > 16 ? 2 : 1) <= 160 * 1024;
}

// act: either (xq, xs) or (hidden_in, delta, hidden_out, eps) -- see StreamArgs.
int gemm_w4a4_stream(const StreamActs& x, const int8_t* wq, const f16* ws, f16* out, int M, int N, int K,
                     hipStream_t st) {
    if (!gemm_w4a4_stream_supported(M, N, K, x.hidden_in != nullptr)) return -1;
    StreamArgs a = with_acts(stream_args(wq, ws, M, N, K), x);
    a.out = out;
    if (longk_shape(K)) return launch_longk<SEPI_PLAIN>(a, st);
    return launch_stream<SEPI_PLAIN>(a, x.hidden_in != nullptr, st);
}

// resid_out = h(f(resid_in) + f(h(x W^T scales)))  -- the projection and the residual add that follows it
int gemm_w4a4_stream_residual(const StreamActs& x, const int8_t* wq, const f16* ws, const f16* resid_in, f16* resid_out,
                              int M, int N, int K, hipStream_t st) {
    if (!gemm_w4a4_stream_supported(M, N, K, x.hidden_in != nullptr)) return -1;
    StreamArgs a = with_acts(stream_args(wq, ws, M, N, K), x);
    a.resid_in = resid_in; a.resid_out = resid_out;
    if (longk_shape(K)) return launch_longk<SEPI_RESID>(a, st);
    return launch_stream<SEPI_RESID>(a, x.hidden_in != nullptr, st);
}

// K-sliced W4A4 at 17..32 tokens: slice count for (M, N, K), 0 = not built / does not pay.  Two slices where a workgroup
// would otherwise hold ONE 16-row tile (N / 16 <= the chip's 256 workgroups): K = 14336 -> 2 x 7168 (Llama-3-8B down_proj).
int gemm_w4a4_stream_partial_slices(int M, int N, int K) {
    if (M < 17 || M > 32 || N % 32 || N / 16 > stream_cap()) return 0;
    if (K == 14336) return 2;
    return 0;
}
int gemm_w4a4_stream_partial(const int8_t* xq, const int8_t* wq, int* ipart, int M, int N, int K, int S, hipStream_t st) {
    if (S != gemm_w4a4_stream_partial_slices(M, N, K) || S < 2 || !ipart) return -1;
    StreamArgs a = stream_args(wq, nullptr, M, N, K / S);
    a.xq = xq; a.ipart = ipart; a.ldx = K / 2; a.ldw = K / 2; a.nq = S;
    // K slices of 7168 (14336 / 2), two token tiles: 8 waves x 7 steps
    if (a.K == 7168) return launch_stream_inst<SEPI_IPART, PRO_Q, 8, 7, 0, 2>(a, st);
    return -1;
}

bool gemm_w4a4_stream_residual_hq_supported(int M, int N, int K, int nparts) {
    return M >= 1 && M <= 4 && (K == 4096 || K == 5120) && nparts == 8 && N % 16 == 0 && N > 0;
}
int gemm_w4a4_stream_residual_hq(const f16* x16, const float* part_amax, int nparts, float clip, const int8_t* wq, const f16* ws,
                                 const f16* resid_in, f16* resid_out, int M, int N, int K, hipStream_t st) {
    if (!gemm_w4a4_stream_residual_hq_supported(M, N, K, nparts)) return -1;
    StreamArgs a = stream_args(wq, ws, M, N, K);
    a.x16 = x16; a.part_amax = part_amax; a.clip = clip;
    a.resid_in = resid_in; a.resid_out = resid_out;
    if (K == 5120) return launch_stream_inst<SEPI_RESID, PRO_RQ, 8, 5, 5>(a, st);
    return launch_stream_inst<SEPI_RESID, PRO_RQ, 8, 4, 4>(a, st);
}
int gemm_w4a4_stream_qkv_rope(const StreamActs& x, const int8_t* wq, const f16* ws, f16* qkv, int M, int N, int K,
                              const int64_t* positions, const f16* cos_sin_cache, f16* key_cache, f16* value_cache,
                              const int64_t* slot_mapping, int nq, int nkv, int d, int rot_dim, hipStream_t st, KvQuant kq) {
    if ((d != 128 && d != 64) || rot_dim != d || N != (nq + 2 * nkv) * d) return -1;
    if (!gemm_w4a4_stream_supported(M, N, K, x.hidden_in != nullptr)) return -1;
    StreamArgs a = with_qkv(with_acts(stream_args(wq, ws, M, N, K), x), positions, cos_sin_cache, key_cache, value_cache,
                            slot_mapping, nq, nkv, d, kq);
    a.out = qkv;
#ifdef QS_EXPERIMENTAL
    if (kq.fp8 && sdma_on<SEPI_QKV>()) return -10;   // the LDS-DMA variants write fp16 caches only (capi.hip names the reason)
    if (!sdma_on<SEPI_QKV>()) {   // (the LDS-DMA forms keep the classic tiles)
        if (const int L = d == 128 ? qkv_level_workgroups(nq, nkv, N) : 0) {
            a.I = L;
            a.ntiles = 2 * L;
        }
    }
#endif
    return launch_stream<SEPI_QKV>(a, x.hidden_in != nullptr, st);
}

int gemm_w4a4_stream_gate_up_silu(const StreamActs& x, const int8_t* wq, const f16* ws, f16* act, int M, int I, int K,
                                  hipStream_t st) {
    if (I % 8) return -1;
    if (!gemm_w4a4_stream_supported(M, 2 * I, K, x.hidden_in != nullptr)) return -1;
    StreamArgs a = with_acts(stream_args(wq, ws, M, 2 * I, K), x);   // (ntiles = 2 I / 16)
    a.out = act; a.I = I;
    return launch_stream<SEPI_GATEUP>(a, x.hidden_in != nullptr, st);
}

}  // namespace qspec

#ifdef QS_STREAM_STAMPS
extern "C" int qspec_debug_stamps(long long* host8) {   // dev builds only (scripts/stream_stamps.py)
    return hipMemcpyFromSymbol(host8, HIP_SYMBOL(qspec::g_sstamps), 8 * sizeof(long long)) == hipSuccess ? 0 : 1;
}
extern "C" int qspec_debug_lnst(long long* host8) {
    return hipMemcpyFromSymbol(host8, HIP_SYMBOL(qspec::g_lnst), 8 * sizeof(long long)) == hipSuccess ? 0 : 1;
}
#endif
#ifdef QS_ENG_STAMPS
extern "C" int qspec_debug_engst(long long* host128) {
    return hipMemcpyFromSymbol(host128, HIP_SYMBOL(qspec::g_engst), 384 * sizeof(long long)) == hipSuccess ? 0 : 1;
}
#endif
#ifdef QS_STREAM_STAMPS
extern "C" int qspec_debug_wgspan(long long* host2048) {
    return hipMemcpyFromSymbol(host2048, HIP_SYMBOL(qspec::g_wgspan), 2048 * sizeof(long long)) == hipSuccess ? 0 : 1;
}
#endif
