// Weight-streaming W4A16 GEMMs for decode-sized M: the kernels of the verify pass, on the streaming skeleton of
// gemm_stream_w4a4.hip (a workgroup of NW waves loops over 16-row weight tiles, every weight register refilled with the same
// step of the next tile right behind its consumer; see that file's header) and over the SAME packed-int4 weight buffer.
//   * gemm_w4a16_stream_kernel: M <= 16, fp16 activation fragments of a wave's K slice loaded once and kept in registers;
//   * gemm_w4a16_stream2_kernel: 17..32 tokens as two token tiles over one pass of the weight stream, K in NB passes;
//   * SEPI_PARTIAL: K slices across workgroups for the long-K layers, raw fp32 sums finished by w4a16_partial_finish_kernel
//     or inside the norm that follows (norm_quant.hip).
// Epilogues as in gemm.hip (plain / RoPE + KV-cache write / silu(gate)*up); the shared pieces: stream_common.cuh.
#include "stream_common.cuh"

namespace qspec {

// ------------------------------------------------------------------ W4A16 (verify pass), same streaming skeleton
// out[m,n] = h( (sum_k f(x[m,k]) * w[n,k]) * f(sw[n]) ), fp32 accumulate  (bitblas.Matmul, quarot_nn/linear.py:102-124)
// over the SAME packed buffer.  A wave always owns the same K steps of every tile, so its activation fragments
// (M <= 16 rows x its K slice, 16 * UB registers per lane) are loaded ONCE, pre-shuffled into the nibble order of
// the dequantiser, and stay in registers for the whole kernel: no LDS tile, no per-step activation traffic (a
// 16-row weight tile alone would need 4x its own bytes in activations per step).
__device__ __forceinline__ f16x8 sdequant_s4x8(u32 p) { return dequant_s4x8_bitop(p); }   // common.cuh (k order 0,4,1,5,2,6,3,7)
__device__ __forceinline__ f16x8 sshuffle_act8(u32x4 a) {  // 8 consecutive fp16 -> order 0,4,1,5,2,6,3,7
    u32x4 o;
    o[0] = __builtin_amdgcn_perm(a[2], a[0], 0x05040100u);
    o[1] = __builtin_amdgcn_perm(a[2], a[0], 0x07060302u);
    o[2] = __builtin_amdgcn_perm(a[3], a[1], 0x05040100u);
    o[3] = __builtin_amdgcn_perm(a[3], a[1], 0x07060302u);
    return __builtin_bit_cast(f16x8, o);
}

// XP: the activations arrive in FRAGMENT-MAJOR layout (a.x = the 16-row tile as [K / 128 steps][4 dwords][4 k-groups][16 rows][8
// halves, dequantiser order]: w4a16_xperm_offset) -- what this kernel's MFMA fragments are -- so a wave takes its fragments
// straight from memory with fully coalesced 1-KiB loads: no LDS staging pass, no barrier in front of the first MFMA.
template <int EPI, int NW, int UB, bool XP = false>
__global__ __launch_bounds__(NW * 64) void gemm_w4a16_stream_kernel(StreamArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int Kb = a.K >> 1;
    const size_t ldw = a.ldw ? (size_t)a.ldw : (size_t)Kb, ldx = a.ldx ? (size_t)a.ldx : (size_t)a.K;
    // SEPI_PARTIAL: blockIdx.y picks one of gridDim.y K slices of length K (x row stride ldx, weight row stride ldw);
    // the raw fp32 sums go to part[blockIdx.y] and are combined in slice order by whoever consumes them
    const size_t kofs = EPI == SEPI_PARTIAL ? (size_t)blockIdx.y * a.K : 0;
    float* red = reinterpret_cast<float*>(smem);                     // [2][NW][256]
    f16* ex = reinterpret_cast<f16*>(red + 2 * NW * 256);            // [2][256]
    // epilogue thread t owns output (token m = t / 16, tile column c = t % 16): for M <= 4 that is wave 0 alone, the
    // other waves go straight back to streaming.  ridx = where the MFMA left that element in a wave's accumulators.
    const int c = tid & 15, m = tid >> 4;
    const bool ethread = m < a.M;
    const int ridx = (m & 3) * 64 + ((m >> 2) & 3) * 16 + c;
    const int mc = m < a.M ? m : 0;
    int64_t pos_m = 0, slot_m = -1;
    if (EPI == SEPI_QKV) {
        pos_m = a.positions[mc];
        slot_m = a.slot_mapping[mc];
    }
    struct Pre {
        f16 swn, cf, sf;
    };
    auto load_pre = [&](Pre& pre, int tile) {
        pre.swn = a.ws[stile_row<EPI>(tile, c, a.I, a.hdl)];
        if (EPI == SEPI_QKV) stream_pre_qkv(a, tile, c, pos_m, pre.cf, pre.sf);
    };
    auto wptr = [&](int tile) -> const uint8_t* {
        return a.wq + (size_t)stile_row<EPI>(tile, r, a.I, a.hdl) * ldw + (kofs >> 1) + g * 16;
    };
    // Activation fragments of this wave's K slice (rows >= M repeat row 0: their outputs are never stored).
    // As MFMA fragments they are 16 rows x 64-byte pieces per load instruction (measured: the 128 KB per workgroup cost
    // ~3 us that way), so the workgroup copies the [16 x K] tile through LDS instead: fully coalesced global loads
    // (1 KiB of one row per wave instruction), 16-byte chunks XOR-swizzled by the row so the ds_read_b128 fragment
    // reads are conflict-free, one stage = the K range of a pair of steps (NW * 256 k), double buffered.
    constexpr int UE = UB & ~1, NST = (UB + 1) / 2;            // paired steps / stages
    constexpr int CPT = 8;                                      // 16-byte chunks per thread and (full) stage
    unsigned char* abuf = smem + (size_t)2 * NW * 1024 + 1024;  // [2][16 rows][NW * 512 B]
    constexpr int SBMAX = NW * 512;
    u32x4 areg[2][CPT];
    auto stage_load = [&](u32x4(&dst)[CPT], int st_) {
        const bool paired = 2 * st_ < UE;
        const int cpr = paired ? NW * 32 : NW * 16;             // chunks per row in this stage
        const size_t kbase = paired ? (size_t)st_ * NW * 256 : (size_t)UE * NW * 128;
#pragma unroll
        for (int i = 0; i < CPT; i++) {
            const int cidx = tid + i * NW * 64;
            const int row = paired ? cidx / (NW * 32) : (cidx / (NW * 16)) & 15;   // unpaired: CPT covers the rows twice
            const int q = cidx % cpr;
            dst[i] = *reinterpret_cast<const u32x4*>(a.x + (size_t)(row < a.M ? row : 0) * ldx + kofs + kbase + (size_t)q * 8);
        }
    };
    auto stage_store = [&](const u32x4(&src)[CPT], int st_) {
        const bool paired = 2 * st_ < UE;
        const int cpr = paired ? NW * 32 : NW * 16;
        unsigned char* buf = abuf + (size_t)(st_ & 1) * 16 * SBMAX;
#pragma unroll
        for (int i = 0; i < CPT; i++) {
            const int cidx = tid + i * NW * 64;
            const int row = paired ? cidx / (NW * 32) : (cidx / (NW * 16)) & 15;
            const int q = cidx % cpr;
            *reinterpret_cast<u32x4*>(buf + (size_t)row * SBMAX + ((q ^ row) << 4)) = src[i];
        }
    };
    f16x8 af[UB][4];
    if constexpr (XP) {
        const f16* xp = a.x + (kofs >> 7) * 2048 + (size_t)lane * 8;     // (step, dword) blocks of 64 lanes x 8 halves
#pragma unroll
        for (int u = 0; u < UB; u++) {
            const int kstep = step_off<NW, UB>(wave, u) >> 6;            // this wave's step u = K step kstep of the row
#pragma unroll
            for (int dd = 0; dd < 4; dd++) af[u][dd] = *reinterpret_cast<const f16x8*>(xp + ((size_t)kstep * 4 + dd) * 512);
        }
    } else {
        stage_load(areg[0], 0);
        if (NST > 1) stage_load(areg[1], 1);
    }
    int tile = a.tile0 + blockIdx.x, par = 0;
    const int tile_end = a.tile0 + a.ntiles;
    const int my_tiles = (tile_end - tile + (int)gridDim.x - 1) / (int)gridDim.x;
    u32x4 w[UB];
    Pre pre = {};
    __builtin_amdgcn_sched_barrier(0);
    {
        const uint8_t* wp0 = wptr(tile);
#pragma unroll
        for (int u = 0; u < UB; u++) w[u] = wload<u32x4>(wp0 + step_off<NW, UB>(wave, u));
        load_pre(pre, tile);
    }
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (!XP)
#pragma unroll
    for (int st_ = 0; st_ < NST; st_++) {
        stage_store(areg[st_ & 1], st_);
        __syncthreads();
        if (st_ + 2 < NST) stage_load(areg[st_ & 1], st_ + 2);   // compile-time condition (unrolled)
        const bool paired = 2 * st_ < UE;
        const unsigned char* buf = abuf + (size_t)(st_ & 1) * 16 * SBMAX + (size_t)r * SBMAX;
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int u = 2 * st_ + j;
            if (u < UB) {
#pragma unroll
                for (int dd = 0; dd < 4; dd++) {
                    const int qq = paired ? wave * 32 + j * 16 + g * 4 + dd : wave * 16 + g * 4 + dd;
                    af[u][dd] = sshuffle_act8(*reinterpret_cast<const u32x4*>(buf + ((qq ^ r) << 4)));
                }
            }
        }
    }

    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    auto use = [&](const u32x4& wv, int u) {
#pragma unroll
        for (int dd = 0; dd < 4; dd++)
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[u][dd], sdequant_s4x8(wv[dd]), acc, 0, 0, 0);
    };
    auto finish = [&](int tile, int par, const Pre& pre) {
        float* rb = red + par * NW * 256;
#pragma unroll
        for (int i = 0; i < 4; i++) rb[wave * 256 + i * 64 + lane] = acc[i];
        acc = f32x4{0.f, 0.f, 0.f, 0.f};
        __syncthreads();
        f16 hv = (f16)0.0f;
        if (ethread) {
            float sum = rb[ridx];
#pragma unroll
            for (int w2 = 1; w2 < NW; w2++) sum = sum + rb[w2 * 256 + ridx];   // wave order: deterministic
            hv = f2h(sum * h2f(pre.swn));
            if (EPI == SEPI_PARTIAL) a.part[((size_t)blockIdx.y * a.M + m) * a.N + tile * 16 + c] = sum;
        }
        if (EPI == SEPI_PARTIAL) return;
        if (EPI == SEPI_PLAIN) {
            if (ethread) a.out[(size_t)m * a.N + tile * 16 + c] = hv;
            return;
        }
        f16* e = ex + par * 256;
        if (tid < 256) e[tid] = hv;
        __syncthreads();
        if (!ethread) return;
        if constexpr (EPI == SEPI_QKV || EPI == SEPI_GATEUP)
            stream_epilogue_pair<EPI>(a, tile, m, c, hv, e[tid ^ 8], pre.cf, pre.sf, slot_m);
    };
    for (int q = 0; q < my_tiles - 1; q++) {
        const int nt = tile + gridDim.x;
        const uint8_t* wp = wptr(nt);
        Pre npre;
        load_pre(npre, nt);
#pragma unroll
        for (int u = 0; u < UB; u++) {
            use(w[u], u);
            __builtin_amdgcn_sched_barrier(0);
            w[u] = wload<u32x4>(wp + step_off<NW, UB>(wave, u));
            __builtin_amdgcn_sched_barrier(0);
        }
        finish(tile, par, pre);
        par ^= 1;
        pre = npre;
        tile = nt;
    }
#pragma unroll
    for (int u = 0; u < UB; u++) use(w[u], u);
    finish(tile, par, pre);
}

// out[m,n] = h( (p_0 + p_1 + ...)[m,n] * f(sw[n]) ): K slices combined in slice order (deterministic).  The verify
// pass does this inside the next norm kernel instead (norm_quant.hip, ln_kernel with `part`); same expression.
__global__ __launch_bounds__(256) void w4a16_partial_finish_kernel(const float* __restrict__ part, const f16* __restrict__ ws,
                                                                     f16* __restrict__ out, int MN, int N, int S) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= MN) return;
    float sum = part[i];
    for (int s2 = 1; s2 < S; s2++) sum = sum + part[(size_t)s2 * MN + i];
    out[i] = f2h(sum * h2f(ws[i % N]));
}

// ---- 17..32 tokens: TWO 16-token tiles over one pass of the weight stream, K in NB passes.
// The M-tiled kernel (gemm_tiled.hip, built for prompt-sized M) dequantises every packed dword for one 32-token block only and
// leaves a SIMD with one wave: Llama-3-70B's verify pass at 32 tokens spent 151 us per layer in its four GEMMs where the draft
// pass streams the same bytes in 82.  Here the streaming kernel takes a second token tile: x is TWO fragment-major 16-row tiles
// (common.cuh: w4a16_xperm_offset32; the producers write them), loaded straight into the MFMA operand registers -- 2 x UB x 16
// VGPRs, which is why K is walked in NB passes of 128 * NW * UB k: pass p holds the fragments of its K range, streams that range
// of EVERY tile of the workgroup and leaves the tile's fp32 sums in LDS (tsum; wave order, then pass order: deterministic); the
// last pass adds its own and runs the epilogue.  8 waves: the tile's 32 x 16 outputs are one per thread.
template <int EPI, int NW, int UB, int NB>
__global__ __launch_bounds__(NW * 64) void gemm_w4a16_stream2_kernel(StreamArgs a) {
    static_assert(NW == 8, "one epilogue thread per output of the two-tile block");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    // SEPI_PARTIAL (NB = 1): blockIdx.y picks one of gridDim.y K slices of length K out of rows of ldx halves (x tiles) / ldw bytes
    // (weights); the raw fp32 sums go to part[blockIdx.y] and are combined in slice order by the norm that follows
    const size_t kofs = EPI == SEPI_PARTIAL ? (size_t)blockIdx.y * a.K : 0;
    const size_t ldw = a.ldw ? (size_t)a.ldw : (size_t)(a.K >> 1), Kx = a.ldx ? (size_t)a.ldx : (size_t)a.K;
    float* red = reinterpret_cast<float*>(smem);                     // [2][NW][2][256]
    f16* ex = reinterpret_cast<f16*>(red + 2 * NW * 512);            // [2][512]
    float* tsum = reinterpret_cast<float*>(ex + 2 * 512);            // [tiles of this workgroup][512] (NB > 1)
    const int c = tid & 15, m = tid >> 4;                            // epilogue thread: (token m of 32, tile column c)
    const bool ethread = m < a.M;
    const int ridx = (m >> 4) * 256 + (m & 3) * 64 + ((m >> 2) & 3) * 16 + c;
    const int mc = m < a.M ? m : 0;
    int64_t pos_m = 0, slot_m = -1;
    if (EPI == SEPI_QKV) {
        pos_m = a.positions[mc];
        slot_m = a.slot_mapping[mc];
    }
    struct Pre {
        f16 swn, cf, sf;
    };
    auto load_pre = [&](Pre& pre, int tile) {
        if (EPI != SEPI_PARTIAL) pre.swn = a.ws[stile_row<EPI>(tile, c, a.I, a.hdl)];
        if (EPI == SEPI_QKV) stream_pre_qkv(a, tile, c, pos_m, pre.cf, pre.sf);
    };
    auto wptr = [&](int tile, int p) -> const uint8_t* {
        return a.wq + (size_t)stile_row<EPI>(tile, r, a.I, a.hdl) * ldw + (kofs >> 1) + (size_t)p * (NW * UB * 64) + g * 16;
    };
    const int tile_first = blockIdx.x;
    const int my_tiles = (a.ntiles - tile_first + (int)gridDim.x - 1) / (int)gridDim.x;
    f16x8 af[2][UB][4];
    auto load_af = [&](int p) {
#pragma unroll
        for (int mt = 0; mt < 2; mt++) {
            const f16* xp = a.x + (size_t)mt * 16 * Kx + (kofs >> 7) * 2048 + (size_t)lane * 8;
#pragma unroll
            for (int u = 0; u < UB; u++) {
                const int kstep = p * (NW * UB) + (step_off<NW, UB>(wave, u) >> 6);
#pragma unroll
                for (int dd = 0; dd < 4; dd++) af[mt][u][dd] = *reinterpret_cast<const f16x8*>(xp + ((size_t)kstep * 4 + dd) * 512);
            }
        }
    };
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    auto use = [&](const u32x4& wv, int u) {
#pragma unroll
        for (int dd = 0; dd < 4; dd++) {
            const f16x8 b = sdequant_s4x8(wv[dd]);
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[0][u][dd], b, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[1][u][dd], b, acc[1], 0, 0, 0);
        }
    };
    int par = 0;
    auto finish = [&](int tile, int ti, int p, const Pre& pre) {
        float* rb = red + par * NW * 512;
#pragma unroll
        for (int mt = 0; mt < 2; mt++) {
#pragma unroll
            for (int i = 0; i < 4; i++) rb[(wave * 2 + mt) * 256 + i * 64 + lane] = acc[mt][i];
            acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        __syncthreads();
        float sum = rb[ridx];
#pragma unroll
        for (int w2 = 1; w2 < NW; w2++) sum = sum + rb[w2 * 512 + ridx];   // wave order: deterministic
        par ^= 1;
        if (NB > 1) {
            if (p > 0) sum = tsum[ti * 512 + tid] + sum;                   // pass order
            if (p < NB - 1) {
                tsum[ti * 512 + tid] = sum;
                return;
            }
        }
        if (EPI == SEPI_PARTIAL) {
            if (ethread) a.part[((size_t)blockIdx.y * a.M + m) * a.N + tile * 16 + c] = sum;
            return;
        }
        const f16 hv = f2h(sum * h2f(pre.swn));
        if (EPI == SEPI_PLAIN) {
            if (ethread) a.out[(size_t)m * a.N + tile * 16 + c] = hv;
            return;
        }
        f16* e = ex + (par ^ 1) * 512;
        e[tid] = hv;
        __syncthreads();
        if (!ethread) return;
        if constexpr (EPI == SEPI_QKV || EPI == SEPI_GATEUP)
            stream_epilogue_pair<EPI, false>(a, tile, m, c, hv, e[tid ^ 8], pre.cf, pre.sf, slot_m);   // (never a half tile)
    };
    // the (pass, tile) units of this workgroup in order; the weights of unit q + 1 are requested behind the use of unit q's
    const int n_units = NB * my_tiles;
    u32x4 w[UB];
    Pre pre = {};
    load_af(0);
    __builtin_amdgcn_sched_barrier(0);
    {
        const uint8_t* wp0 = wptr(tile_first, 0);
#pragma unroll
        for (int u = 0; u < UB; u++) w[u] = wload<u32x4>(wp0 + step_off<NW, UB>(wave, u));
        if (NB == 1) load_pre(pre, tile_first);
    }
    __builtin_amdgcn_sched_barrier(0);
    int p = 0, ti = 0, tile = tile_first;
    for (int q = 0; q < n_units - 1; q++) {
        int np = p, nti = ti + 1, ntile = tile + (int)gridDim.x;
        if (nti == my_tiles) {
            np = p + 1;
            nti = 0;
            ntile = tile_first;
        }
        const uint8_t* wp = wptr(ntile, np);
        Pre npre = {};
        if (np == NB - 1) load_pre(npre, ntile);
#pragma unroll
        for (int u = 0; u < UB; u++) {
            use(w[u], u);
            __builtin_amdgcn_sched_barrier(0);
            w[u] = wload<u32x4>(wp + step_off<NW, UB>(wave, u));
            __builtin_amdgcn_sched_barrier(0);
        }
        finish(tile, ti, p, pre);
        if (np != p) load_af(np);   // (behind the last use of pass p's fragments)
        pre = npre;
        p = np;
        ti = nti;
        tile = ntile;
    }
#pragma unroll
    for (int u = 0; u < UB; u++) use(w[u], u);
    finish(tile, ti, p, pre);
}

// shapes of the two-tile kernel, X(K, UB, NB): K = 128 * 8 * UB * NB.  The table is walked by the predicate and by the launch
// switch: a new K is one X() here.
#define QS_W4A16_SHAPES32(X) X(4096, 4, 1) X(8192, 4, 2) X(28672, 4, 7) X(14336, 2, 7) X(5120, 5, 1)
static bool stream32_shape(int K, int* NB) {
#define X(KV, UBV, NBV) if (K == KV) { *NB = NBV; return true; }
    QS_W4A16_SHAPES32(X)
#undef X
    return false;
}
bool gemm_w4a16_stream32_supported(int M, int N, int K) {
    int NB;
    if (M < 17 || M > 32 || N % 16 || !stream32_shape(K, &NB)) return false;
    const int nt = N / 16, per = (nt + stream_cap() - 1) / stream_cap();   // tiles per workgroup
    return NB == 1 || (size_t)per * 2048 <= 96 * 1024;   // tsum: 2 KB per tile of a workgroup
}
template <int EPI, int UB, int NB>
static int launch_stream32_inst(const StreamArgs& a, hipStream_t st) {
    const int slices = EPI == SEPI_PARTIAL ? a.nq : 1;   // (nq carries the slice count for SEPI_PARTIAL)
    const int cap = slices > 1 ? (stream_cap() / slices > 0 ? stream_cap() / slices : 1) : stream_cap();   // one workgroup per CU in all
    const int grid = stream_grid(a.ntiles, cap), per = a.ntiles > cap ? (a.ntiles + cap - 1) / cap : 1;   // tiles per workgroup
    const size_t lds = (size_t)2 * 8 * 512 * 4 + 2 * 512 * 2 + (NB > 1 ? (size_t)per * 2048 : 0);
    if (const int rc = lds_optin<gemm_w4a16_stream2_kernel<EPI, 8, UB, NB>>(lds)) return rc;
    hipLaunchKernelGGL((gemm_w4a16_stream2_kernel<EPI, 8, UB, NB>), dim3(grid, slices), dim3(8 * 64), lds, st, a);
    return 0;
}
// K slices of the two-tile kernel for a long-K layer whose sums the following norm finishes (down_proj at 17..32 tokens): S one-pass
// slices of 4096 (UB = 4) or 2048 (UB = 2) k across the workgroups instead of S passes inside one -- 0 where no such cut exists
int gemm_w4a16_stream32_partial_slices(int M, int N, int K) {
    if (M < 17 || M > 32 || N % 16) return 0;
    for (int len : {4096, 2048})
        if (K % len == 0 && K / len >= 2 && K / len <= 8) return K / len;
    return 0;
}
int gemm_w4a16_stream32_partial(const f16* x, const int8_t* wq, float* part, int M, int N, int K, int S, hipStream_t st) {
    if (S < 2 || S != gemm_w4a16_stream32_partial_slices(M, N, K) || !part) return -1;
    StreamArgs a = stream_args(wq, nullptr, M, N, K / S);
    a.x = x; a.ldx = K; a.ldw = K / 2; a.part = part; a.nq = S;
    if (a.K == 4096) return launch_stream32_inst<SEPI_PARTIAL, 4, 1>(a, st);
    return launch_stream32_inst<SEPI_PARTIAL, 2, 1>(a, st);
}
template <int EPI>
static int launch_stream32(const StreamArgs& a, hipStream_t st) {
    if (!gemm_w4a16_stream32_supported(a.M, a.N, a.K)) return -1;
#define X(KV, UBV, NBV) if (a.K == KV) return launch_stream32_inst<EPI, UBV, NBV>(a, st);
    QS_W4A16_SHAPES32(X)
#undef X
    return -1;
}
// x: two fragment-major 16-row tiles (rows 0..15, 16..31), each 16 x K halves
int gemm_w4a16_stream32(const f16* x, const int8_t* wq, const f16* ws, f16* out, int M, int N, int K, hipStream_t st) {
    StreamArgs a = stream_args(wq, ws, M, N, K);
    a.x = x; a.out = out;
    return launch_stream32<SEPI_PLAIN>(a, st);
}
int gemm_w4a16_stream32_qkv_rope(const f16* x, const int8_t* wq, const f16* ws, f16* qkv, int M, int N, int K,
                                 const int64_t* positions, const f16* cos_sin_cache, f16* key_cache, f16* value_cache,
                                 const int64_t* slot_mapping, int nq, int nkv, int d, int rot_dim, hipStream_t st, KvQuant kq) {
    if ((d != 128 && d != 64) || rot_dim != d || N != (nq + 2 * nkv) * d) return -1;
    StreamArgs a = with_qkv(stream_args(wq, ws, M, N, K), positions, cos_sin_cache, key_cache, value_cache, slot_mapping, nq, nkv, d, kq);
    a.x = x; a.out = qkv;
    return launch_stream32<SEPI_QKV>(a, st);
}
int gemm_w4a16_stream32_gate_up_silu(const f16* x, const int8_t* wq, const f16* ws, f16* act, int M, int I, int K, hipStream_t st) {
    if (I % 8) return -1;
    StreamArgs a = stream_args(wq, ws, M, 2 * I, K);
    a.x = x; a.out = act; a.I = I;
    return launch_stream32<SEPI_GATEUP>(a, st);
}

// Shapes of the 16-row kernel, X(NW, UB, XPERM): one batch per tile only (the activation fragments of a wave's K slice live in
// registers), K = 128 * NW * UB; XPERM = also built for the fragment-major activation layout (the Llama-3-8B / Llama-2-13B
// shapes: K = 4096 / 5120 / 3584 / 4608).  Walked by the predicates and by the launch switch: a new K is one X() here.
// (16, 7) = K 14336 is NOT here: 16 rows x 14336 k of fp16 activations (458 KB) do not fit one CU's registers
// (16 waves x 112 VGPRs would leave nothing else); that layer stays on gemm.hip's 2-D kernel
// (4, 9) = K 4608: a third of Llama-2-13B's down_proj (13824 = 3 x 4608, gemm_w4a16_stream_partial_slices); the
// activation staging buffer is 2 x 16 rows x NW x 512 B, so NW stays <= 8 (12 waves x 3 steps would need 222 KB of LDS)
// (4, 11) = K 5632: TinyLlama's down_proj
#define QS_W4A16_SHAPES16(X) \
    X(8, 4, 1) X(8, 8, 0) X(8, 5, 1) X(4, 4, 0) X(4, 2, 0) X(8, 7, 0) X(4, 7, 1) X(4, 1, 0) X(4, 9, 1) X(4, 11, 0)
static bool stream16_shape(int K, bool* xperm = nullptr) {
    if (K % 128) return false;
#define X(NWV, UBV, XP) if (K / 128 == NWV * UBV) { if (xperm) *xperm = XP; return true; }
    QS_W4A16_SHAPES16(X)
#undef X
    return false;
}

template <int EPI, int NW, int UB, bool XPERM>
static int launch_stream16_inst(const StreamArgs& a, hipStream_t st) {
    const size_t lds = (size_t)2 * NW * 1024 + 1024 + (size_t)2 * 16 * NW * 512;   // reduction + activation staging
    if (const int rc = lds_optin<gemm_w4a16_stream_kernel<EPI, NW, UB, false>>(lds)) return rc;
    const int cap = stream_cap();
    int grid = stream_grid(a.ntiles, cap);
    const int slices = EPI == SEPI_PARTIAL ? a.nq : 1;   // (nq carries the slice count for SEPI_PARTIAL)
    if (slices > 1) {   // one workgroup per CU in total: the tile groups share the grid with the slices
        const int per_slice = cap / slices > 0 ? cap / slices : 1;
        if (grid > per_slice) grid = stream_grid(a.ntiles, per_slice);
    }
    if constexpr (XPERM) {
        if (a.xperm) {
            hipLaunchKernelGGL((gemm_w4a16_stream_kernel<EPI, NW, UB, true>), dim3(grid, slices), dim3(NW * 64),
                               (size_t)2 * NW * 1024 + 1024, st, a);
            return 0;
        }
    }
    if (a.xperm) return -1;
    hipLaunchKernelGGL((gemm_w4a16_stream_kernel<EPI, NW, UB, false>), dim3(grid, slices), dim3(NW * 64), lds, st, a);
    return 0;
}

bool gemm_w4a16_stream_supported(int M, int N, int K) { return M >= 1 && M <= 16 && N % 16 == 0 && stream16_shape(K); }

template <int EPI>
static int launch_stream16(const StreamArgs& a, hipStream_t st) {
    if (a.M < 1 || a.M > 16 || a.K % 128) return -1;
#define X(NWV, UBV, XP) if (a.K / 128 == NWV * UBV) return launch_stream16_inst<EPI, NWV, UBV, XP != 0>(a, st);
    QS_W4A16_SHAPES16(X)
#undef X
    return -1;
}

// xperm (every entry below): x is the 16-row activation tile in fragment-major layout (common.cuh: w4a16_xperm_offset; the
// producers write it: norm_quant.hip ln_kernel, hadamard.hip spread forms) -- built for the shapes gemm_w4a16_xperm_supported names
bool gemm_w4a16_xperm_supported(int M, int K) {
    bool xperm = false;
    return M >= 1 && M <= 16 && stream16_shape(K, &xperm) && xperm;
}
int gemm_w4a16_stream(const f16* x, int64_t ldx, const int8_t* wq, int64_t ldw, const f16* ws, f16* out, int M, int N,
                      int K, hipStream_t st, int xperm) {
    if (!gemm_w4a16_stream_supported(M, N, K) || (ldx && ldx % 8) || (ldw && ldw % 16)) return -1;
    if (xperm && (ldx || !gemm_w4a16_xperm_supported(M, K))) return -1;
    StreamArgs a = stream_args(wq, ws, M, N, K);
    a.x = x; a.ldx = ldx; a.ldw = ldw; a.out = out; a.xperm = xperm;
    return launch_stream16<SEPI_PLAIN>(a, st);
}

// Long-K layers (down_proj, K = 14336): 16 rows x K of fp16 activations do not fit one CU's registers, so K is cut
// into S slices of a built length (14336 = 2 x 7168), slice s on workgroups (tile group, s); raw fp32 sums per slice
// go to part [S][M][N].  Returns the slice count to use for (M, N, K), 0 if the shape is not covered.
int gemm_w4a16_stream_partial_slices(int M, int N, int K) {
    if (gemm_w4a16_stream_supported(M, N, K)) return 0;   // fits unsliced: use the plain entry
    static const int forced = QS_DEV_KNOB("QSPEC_W4A16_SLICES", 0);   // (dev knob for sweeps)
    if (forced >= 2 && forced <= 4 && K % forced == 0 && gemm_w4a16_stream_supported(M, N, K / forced)) return forced;
    // Four slices first: a workgroup stages the whole [16, K / S] fp16 activation slice (16 * K / S * 2 bytes) for
    // tiles-per-workgroup * 16 * K / S / 2 bytes of weights, and the grid is one workgroup per CU in all, so S slices mean
    // S tiles per workgroup at N = 4096: S = 2 moves 229 KB of activations for 115 KB of weights per workgroup, S = 4
    // 115 KB for 115 KB (Llama-3-8B down_proj, verify pass: cycle 7.66 -> 7.61 ms).
    static const int order[3] = {4, 2, 3};
    for (int S : order)
        if (K % S == 0 && gemm_w4a16_stream_supported(M, N, K / S)) return S;
    return 0;
}
int gemm_w4a16_stream_partial(const f16* x, int64_t ldx, const int8_t* wq, int64_t ldw, float* part, int M, int N, int K,
                              int S, hipStream_t st, int xperm) {
    if (S < 1 || K % S || !gemm_w4a16_stream_supported(M, N, K / S) || !part) return -1;
    if (xperm && (ldx || (K / S) % 128 || !gemm_w4a16_xperm_supported(M, K / S))) return -1;
    StreamArgs a = stream_args(wq, nullptr, M, N, K / S);
    a.xperm = xperm;
    a.x = x; a.ldx = ldx ? ldx : K; a.ldw = ldw ? ldw : K / 2; a.part = part; a.nq = S;
    return launch_stream16<SEPI_PARTIAL>(a, st);
}
int gemm_w4a16_partial_finish(const float* part, const f16* ws, f16* out, int M, int N, int S, hipStream_t st) {
    const int MN = M * N;
    hipLaunchKernelGGL(w4a16_partial_finish_kernel, dim3((MN + 255) / 256), dim3(256), 0, st, part, ws, out, MN, N, S);
    return 0;
}

int gemm_w4a16_stream_qkv_rope(const f16* x, const int8_t* wq, const f16* ws, f16* qkv, int M, int N, int K,
                               const int64_t* positions, const f16* cos_sin_cache, f16* key_cache, f16* value_cache,
                               const int64_t* slot_mapping, int nq, int nkv, int d, int rot_dim, hipStream_t st, int xperm,
                               KvQuant kq) {
    if ((d != 128 && d != 64) || rot_dim != d || N != (nq + 2 * nkv) * d || !gemm_w4a16_stream_supported(M, N, K)) return -1;
    if (xperm && !gemm_w4a16_xperm_supported(M, K)) return -1;
    StreamArgs a = with_qkv(stream_args(wq, ws, M, N, K), positions, cos_sin_cache, key_cache, value_cache, slot_mapping, nq, nkv, d, kq);
    a.x = x; a.out = qkv; a.xperm = xperm;
#ifdef QS_EXPERIMENTAL
    if (const int L = d == 128 ? qkv_level_workgroups(nq, nkv, N) : 0) {   // twelve RoPE pairs per workgroup: a full + a half tile
        a.I = L;
        a.ntiles = 2 * L;
    }
#endif
    return launch_stream16<SEPI_QKV>(a, st);
}

int gemm_w4a16_stream_gate_up_silu(const f16* x, const int8_t* wq, const f16* ws, f16* act, int M, int I, int K, int ch0,
                                   int nch, hipStream_t st, int xperm) {
    if (I % 8 || ch0 % 8 || nch % 8 || ch0 + nch > I || !gemm_w4a16_stream_supported(M, 2 * I, K)) return -1;
    if (xperm && !gemm_w4a16_xperm_supported(M, K)) return -1;
    StreamArgs a = stream_args(wq, ws, M, 2 * I, K);
    a.x = x; a.out = act; a.xperm = xperm; a.I = I; a.tile0 = ch0 / 8; a.ntiles = nch / 8;
    return launch_stream16<SEPI_GATEUP>(a, st);
}

}  // namespace qspec
