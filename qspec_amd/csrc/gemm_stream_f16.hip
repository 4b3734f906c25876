// The lm_head: fp16 x fp16^T for decode-sized M on the streaming skeleton of gemm_stream_w4a4.hip (see that file's header).
//   * gemm_f16_stream_kernel / gemm_f16_longk_kernel: the register-streaming forms (one / several batches per tile);
//   * gemm_f16_sdma_kernel: the 1 GB vocabulary stream through self-service LDS-DMA -- what the cycle launches (K = 4096);
//     gemm_f16_sdma2_kernel: the same for 17..32 tokens, two token tiles over one pass of the weights.
// All bit-identical to each other and to gemm.hip's gemm_f16_kernel; every form also leaves the per-workgroup row maxima
// (HeadMax) that the sampler front end starts from.  The shared pieces: stream_common.cuh.
#include "stream_common.cuh"

namespace qspec {

#ifdef QS_EXPERIMENTAL
#include "experimental/prefetch.inc"      // weight prefetch launches: qspec_prefetch / qspec_prefetch_tiles
#endif

// ------------------------------------------------------------------ fp16 x fp16^T (lm_head), same skeleton
// out[m,n] = h( sum_k f(x[m,k]) f(w[n,k]) ), fp32 accumulate  (nn.Linear lm_head, logits_processor.py:92-97).
// K = 32 * NW * UB: a wave keeps UB loads (UB KiB) of the 1 GB vocabulary matrix in flight and its activation
// fragments in registers; a workgroup walks over its tiles with the refill-behind-use pipeline of the kernels above.
// part_max (may be NULL; the sampler front end, sampler.hip): every workgroup also leaves, per token row, the largest
// fp16 logit among ITS tiles and the first column holding it -- part_max[m * gridDim.x + blockIdx.x] = {value, column}
// -- so that the softmax that follows does not have to read the logits once more just to find the row maximum.
struct HeadMax {
    float v;
    int i;
};
template <int NW, int UB>
__global__ __launch_bounds__(NW * 64) void gemm_f16_stream_kernel(const f16* __restrict__ x, const f16* __restrict__ wt,
                                                                  f16* __restrict__ out, int M, int N, int K,
                                                                  int ntiles, HeadMax* __restrict__ part_max) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* red = reinterpret_cast<float*>(smem);   // [2][NW][256]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int c = tid & 15, m = tid >> 4;   // epilogue thread -> (token, tile column), as in the kernels above
    const bool ethread = m < M;
    const int ridx = (m & 3) * 64 + ((m >> 2) & 3) * 16 + c;
    // step u of this wave = bytes [step_off(wave, u) + 16 g, +16) of a weight row = k (halves) offset / 2
    f16x8 af[UB];
    {
        const f16* xrow = x + (size_t)(r < M ? r : 0) * K + g * 8;
#pragma unroll
        for (int u = 0; u < UB; u++) af[u] = *reinterpret_cast<const f16x8*>(xrow + step_off<NW, UB>(wave, u) / 2);
    }
    int tile = blockIdx.x, par = 0;
    const int my_tiles = (ntiles - tile + (int)gridDim.x - 1) / (int)gridDim.x;
    auto wptr = [&](int t) -> const unsigned char* {
        return reinterpret_cast<const unsigned char*>(wt + (size_t)(t * 16 + r) * K) + g * 16;
    };
    f16x8 w[UB];
    __builtin_amdgcn_sched_barrier(0);
    {
        const unsigned char* wp0 = wptr(tile);
#pragma unroll
        for (int u = 0; u < UB; u++) w[u] = wload<f16x8>(wp0 + step_off<NW, UB>(wave, u));
    }
    __builtin_amdgcn_sched_barrier(0);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float best_v = -__builtin_inff();
    int best_i = 0x7fffffff;
    auto finish = [&](int t, int par) {
        float* rb = red + par * NW * 256;
#pragma unroll
        for (int i = 0; i < 4; i++) rb[wave * 256 + i * 64 + lane] = acc[i];
        acc = f32x4{0.f, 0.f, 0.f, 0.f};
        __syncthreads();
        if (ethread) {
            float sum = rb[ridx];
#pragma unroll
            for (int w2 = 1; w2 < NW; w2++) sum = sum + rb[w2 * 256 + ridx];
            const f16 hv = f2h(sum);
            out[(size_t)m * N + t * 16 + c] = hv;
            const float fv = h2f(hv);
            if (fv > best_v) {          // tiles come in increasing column order: a tie keeps the first column
                best_v = fv;
                best_i = t * 16 + c;
            }
        }
    };
    for (int q = 0; q < my_tiles - 1; q++) {
        const int nt = tile + gridDim.x;
        const unsigned char* wp = wptr(nt);
#pragma unroll
        for (int u = 0; u < UB; u++) {
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[u], w[u], acc, 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            w[u] = wload<f16x8>(wp + step_off<NW, UB>(wave, u));
            __builtin_amdgcn_sched_barrier(0);
        }
        finish(tile, par);
        par ^= 1;
        tile = nt;
    }
#pragma unroll
    for (int u = 0; u < UB; u++) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[u], w[u], acc, 0, 0, 0);
    finish(tile, par);
    if (part_max) {   // the 16 columns of a row sit in 16 consecutive lanes: larger value, then smaller column, wins
#pragma unroll
        for (int mk = 1; mk < 16; mk <<= 1) {
            const float ov = __shfl_xor(best_v, mk, 64);
            const int oi = __shfl_xor(best_i, mk, 64);
            if (ov > best_v || (ov == best_v && oi < best_i)) {
                best_v = ov;
                best_i = oi;
            }
        }
        if (ethread && c == 0) part_max[(size_t)m * gridDim.x + blockIdx.x] = HeadMax{best_v, best_i};
    }
}

// ---- long rows (K = 8192, Llama-3-70B's lm_head: 2.1 GB): NB batches of NW x UB steps per tile, as gemm_w4a4_longk_kernel
// does for the int4 GEMM -- 16 waves x 16 steps of fp16 fragments do not fit the 128-VGPR budget of 1024 threads, two batches
// of 8 do (64 VGPRs of activation fragments + 32 of weights).  Each weight register is refilled with the same step of the next
// batch (the next tile's first batch behind the last one) right behind its consumer.  Same sums per output in the same wave
// order as gemm_f16_kernel's, fp32; same HeadMax partials as gemm_f16_stream_kernel.
template <int NW, int UB, int NB>
__global__ __launch_bounds__(NW * 64) void gemm_f16_longk_kernel(const f16* __restrict__ x, const f16* __restrict__ wt,
                                                                 f16* __restrict__ out, int M, int N, int K, int ntiles,
                                                                 HeadMax* __restrict__ part_max) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* red = reinterpret_cast<float*>(smem);   // [2][NW][256]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int c = tid & 15, m = tid >> 4;
    const bool ethread = m < M;
    const int ridx = (m & 3) * 64 + ((m >> 2) & 3) * 16 + c;
    constexpr int BB = UB * NW * 64;               // bytes of a weight row per batch
    f16x8 af[NB][UB];
    {
        const unsigned char* xrow = reinterpret_cast<const unsigned char*>(x + (size_t)(r < M ? r : 0) * K) + g * 16;
#pragma unroll
        for (int b = 0; b < NB; b++)
#pragma unroll
            for (int u = 0; u < UB; u++) af[b][u] = *reinterpret_cast<const f16x8*>(xrow + (size_t)b * BB + step_off<NW, UB>(wave, u));
    }
    int tile = blockIdx.x, par = 0;
    const int my_tiles = (ntiles - tile + (int)gridDim.x - 1) / (int)gridDim.x;
    auto wptr = [&](int t, int b) -> const unsigned char* {
        return reinterpret_cast<const unsigned char*>(wt + (size_t)(t * 16 + r) * K) + (size_t)b * BB + g * 16;
    };
    f16x8 w[UB];
    __builtin_amdgcn_sched_barrier(0);
    {
        const unsigned char* wp0 = wptr(tile, 0);
#pragma unroll
        for (int u = 0; u < UB; u++) w[u] = wload<f16x8>(wp0 + step_off<NW, UB>(wave, u));
    }
    __builtin_amdgcn_sched_barrier(0);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float best_v = -__builtin_inff();
    int best_i = 0x7fffffff;
    auto finish = [&](int t, int par) {
        float* rb = red + par * NW * 256;
#pragma unroll
        for (int i = 0; i < 4; i++) rb[wave * 256 + i * 64 + lane] = acc[i];
        acc = f32x4{0.f, 0.f, 0.f, 0.f};
        __syncthreads();
        if (ethread) {
            float sum = rb[ridx];
#pragma unroll
            for (int w2 = 1; w2 < NW; w2++) sum = sum + rb[w2 * 256 + ridx];
            const f16 hv = f2h(sum);
            out[(size_t)m * N + t * 16 + c] = hv;
            const float fv = h2f(hv);
            if (fv > best_v) {          // tiles come in increasing column order: a tie keeps the first column
                best_v = fv;
                best_i = t * 16 + c;
            }
        }
    };
    for (int q = 0; q < my_tiles - 1; q++) {
        const int nt = tile + gridDim.x;
#pragma unroll
        for (int b = 0; b < NB; b++) {
            const unsigned char* wp = b + 1 < NB ? wptr(tile, b + 1) : wptr(nt, 0);
#pragma unroll
            for (int u = 0; u < UB; u++) {
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[b][u], w[u], acc, 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
                w[u] = wload<f16x8>(wp + step_off<NW, UB>(wave, u));
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        finish(tile, par);
        par ^= 1;
        tile = nt;
    }
#pragma unroll
    for (int b = 0; b < NB; b++) {
#pragma unroll
        for (int u = 0; u < UB; u++) {
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[b][u], w[u], acc, 0, 0, 0);
            if (b + 1 < NB) {
                __builtin_amdgcn_sched_barrier(0);
                w[u] = wload<f16x8>(wptr(tile, b + 1) + step_off<NW, UB>(wave, u));
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
    finish(tile, par);
    if (part_max) {   // the 16 columns of a row sit in 16 consecutive lanes: larger value, then smaller column, wins
#pragma unroll
        for (int mk = 1; mk < 16; mk <<= 1) {
            const float ov = __shfl_xor(best_v, mk, 64);
            const int oi = __shfl_xor(best_i, mk, 64);
            if (ov > best_v || (ov == best_v && oi < best_i)) {
                best_v = ov;
                best_i = oi;
            }
        }
        if (ethread && c == 0) part_max[(size_t)m * gridDim.x + blockIdx.x] = HeadMax{best_v, best_i};
    }
}

// ---- the same lm_head with its 1 GB weight stream through self-service LDS-DMA (K = 4096, M <= 16).
// The draft GEMMs did not gain from LDS-DMA (what is above their floor is the launch's fixed
// sequence, not stream time); THIS launch is 99 % stream: 31 tiles of 128 KB per workgroup, where the register path's
// pure read reaches 6.2 TB/s and four or more issuing waves per CU with `global_load_lds_dwordx4 ... nt` 6.9 TB/s
// (scripts/micro/ldsdma.hip: 168 -> 151 us for these bytes).  Stream wave w owns the k range [512 w, 512 w + 512) of
// every weight row (1 KiB per row) and walks it in GROUPS of four 64-byte steps: one group = 16 rows x 256 B = four loads
// (4 rows x 256 B each, lane l -> row 4 q + l / 16, 16-byte piece (l % 16) ^ row: the LDS image stays lane-linear, the
// fragment reads are conflict-free).  A wave keeps a rolling window of four groups (16 KiB of its own LDS, 16 loads) in
// flight -- 128 KB per CU -- and learns that a group has landed from its own `s_waitcnt vmcnt(12)`: no loader waves, no
// flags.  The epilogue (sum of the eight waves' fp32 partials in wave order, one rounding, store, running row maximum)
// belongs to four waves that stream nothing; they meet the stream waves at one barrier per tile.
template <int MT /* 16-token tiles: M <= 16 MT */>
__global__ __launch_bounds__(12 * 64) void gemm_f16_sdma_kernel(const f16* __restrict__ x, const f16* __restrict__ wt,
                                                                f16* __restrict__ out, int M, int N, int ntiles,
                                                                HeadMax* __restrict__ part_max) {
    constexpr int NW = 8, K = 4096, WIN = 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* red = reinterpret_cast<float*>(smem);                 // [2][NW][MT][256]
    unsigned char* ring = smem + (size_t)2 * NW * MT * 1024;     // [NW][WIN][4 KiB]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int my_tiles = (ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;

    if (wave >= NW) {   // ---------------------------------------------------------------- epilogue waves
        const int et = tid - NW * 64;                            // 0..255 -> (token m (+ 16 mt), tile column c)
        const int c = et & 15, m0 = et >> 4;
        const int ridx = (m0 & 3) * 64 + ((m0 >> 2) & 3) * 16 + c;
        float best_v[MT];
        int best_i[MT];
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
            best_v[mt] = -__builtin_inff();
            best_i[mt] = 0x7fffffff;
        }
        int tile = blockIdx.x, par = 0;
        for (int ti = 0; ti < my_tiles; ti++) {
            __syncthreads();                                     // A(ti): the stream waves have posted the tile's partials
            const float* rb = red + par * NW * MT * 256;
#pragma unroll
            for (int mt = 0; mt < MT; mt++) {
                const int m = m0 + 16 * mt;
                if (m < M) {
                    float sum = rb[mt * 256 + ridx];
#pragma unroll
                    for (int w2 = 1; w2 < NW; w2++) sum = sum + rb[(w2 * MT + mt) * 256 + ridx];
                    const f16 hv = f2h(sum);
                    out[(size_t)m * N + tile * 16 + c] = hv;
                    const float fv = h2f(hv);
                    if (fv > best_v[mt]) {          // tiles come in increasing column order: a tie keeps the first column
                        best_v[mt] = fv;
                        best_i[mt] = tile * 16 + c;
                    }
                }
            }
            par ^= 1;
            tile += gridDim.x;
        }
        if (part_max) {   // the 16 columns of a row sit in 16 consecutive lanes: larger value, then smaller column, wins
#pragma unroll
            for (int mt = 0; mt < MT; mt++) {
                float bv = best_v[mt];
                int bi = best_i[mt];
#pragma unroll
                for (int mk = 1; mk < 16; mk <<= 1) {
                    const float ov = __shfl_xor(bv, mk, 64);
                    const int oi = __shfl_xor(bi, mk, 64);
                    if (ov > bv || (ov == bv && oi < bi)) {
                        bv = ov;
                        bi = oi;
                    }
                }
                const int m = m0 + 16 * mt;
                if (m < M && c == 0) part_max[(size_t)m * gridDim.x + blockIdx.x] = HeadMax{bv, bi};
            }
        }
        return;
    }

    // ---------------------------------------------------------------- stream waves
    const int r = lane & 15, g = lane >> 4;
    // activation fragments of this wave's k range: step s = halves [512 w + 32 s + 8 g, + 8) of row r + 16 mt (rows >= M: row 0)
    f16x8 af[MT][16];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) {
        const int row = r + 16 * mt;
        const f16* xrow = x + (size_t)(row < M ? row : 0) * K + wave * 512 + g * 8;
#pragma unroll
        for (int s2 = 0; s2 < 16; s2++) af[mt][s2] = *reinterpret_cast<const f16x8*>(xrow + s2 * 32);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // before the first LDS-DMA load: hipcc's own waits do not know them
    const u32 my0 = (u32)(unsigned long long)(__attribute__((address_space(3))) unsigned char*)ring + (u32)wave * (WIN * 4096);
    // source of this lane inside a group: row 4 q + (lane >> 4) of the tile, 16-byte piece ((lane & 15) ^ row) of the group's
    // 256-byte segment of the wave's KiB
    const int lrow = lane >> 4;
    auto issue_group = [&](int gi) {   // group gi = (tile gi / 4, segment gi % 4) of this workgroup's sequence
        const int t = blockIdx.x + (gi >> 2) * (int)gridDim.x;
        const unsigned char* base = reinterpret_cast<const unsigned char*>(wt + (size_t)t * 16 * K) + wave * 1024 + (gi & 3) * 256;
        const u32 dst = my0 + (u32)(gi & (WIN - 1)) * 4096u;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int row = 4 * q + lrow;
            glds16<1>(base + (size_t)row * (K * 2) + (((lane & 15) ^ row) << 4), dst + (u32)q * 1024u);
        }
    };
    const int n_groups = my_tiles * 4;
#pragma unroll
    for (int gi = 0; gi < WIN; gi++)
        if (gi < n_groups) issue_group(gi);
    typedef __attribute__((address_space(3))) u32x4 lds_u32x4_t;
    const __attribute__((address_space(3))) unsigned char* my3 =
        (const __attribute__((address_space(3))) unsigned char*)ring + (size_t)wave * (WIN * 4096);
    // fragment of step q2 (0..3) of a group, lane (r, g): load r / 4, lane (r % 4) * 16 + ((4 q2 + g) ^ r)
    u32 foff[4];
#pragma unroll
    for (int q2 = 0; q2 < 4; q2++) foff[q2] = (u32)(r >> 2) * 1024u + (u32)((((r & 3) << 4) | ((q2 * 4 + g) ^ r)) << 4);
    f32x4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    int par = 0, gi = 0;
    for (int ti = 0; ti < my_tiles; ti++) {
        const bool last = ti == my_tiles - 1;   // (wave-uniform) the window runs empty behind the last tile
#pragma unroll
        for (int seg = 0; seg < 4; seg++, gi++) {   // unrolled: the fragment registers are indexed statically
            if (!last) vmcnt_le<12>();              // three groups issued behind this one
            else if (seg == 0) vmcnt_le<12>();
            else if (seg == 1) vmcnt_le<8>();
            else if (seg == 2) vmcnt_le<4>();
            else vmcnt_le<0>();
            u32x4 wv[4];
#pragma unroll
            for (int q2 = 0; q2 < 4; q2++)
                wv[q2] = *reinterpret_cast<const volatile lds_u32x4_t*>(my3 + (size_t)seg * 4096 + foff[q2]);   // slot = gi % WIN = seg
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (gi + WIN < n_groups) issue_group(gi + WIN);   // into the slot just read
#pragma unroll
            for (int q2 = 0; q2 < 4; q2++)
#pragma unroll
                for (int mt = 0; mt < MT; mt++)
                    acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[mt][seg * 4 + q2], __builtin_bit_cast(f16x8, wv[q2]), acc[mt], 0, 0, 0);
        }
        // tile complete: post the partial sums, meet the epilogue waves
        float* rb = red + par * NW * MT * 256;
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
#pragma unroll
            for (int i = 0; i < 4; i++) rb[(wave * MT + mt) * 256 + i * 64 + lane] = acc[mt][i];
            acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();   // A (raw: no vmcnt drain)
        par ^= 1;
    }
}
// ---- 17..32 tokens (config 3's draft steps): two token tiles over ONE pass of the weight stream.
// The 12-wave form above has no room for a second tile's 64 fragment registers (three waves per SIMD: 170 VGPRs; it was built
// and spilled: 240 us against the M-tiled kernel's 230).  Here ALL eight waves stream -- two per SIMD, 256 VGPRs, 128 of them
// activation fragments -- with the same ring (four 4-KiB groups per wave in flight, 128 KB per CU), and the epilogue is theirs
// too: 8 x 64 lanes = the tile's 32 x 16 outputs, one per lane, summed over the waves' partials in wave order.  The partials
// are single-buffered (16 KB: ring + partials = 144 KB): barrier B in front of the post, barrier A behind it; the LDS-DMA
// window keeps filling across both (raw s_barrier, no vmcnt drain).
__global__ __launch_bounds__(8 * 64) void gemm_f16_sdma2_kernel(const f16* __restrict__ x, const f16* __restrict__ wt,
                                                                f16* __restrict__ out, int M, int N, int ntiles,
                                                                HeadMax* __restrict__ part_max) {
    constexpr int NW = 8, K = 4096, WIN = 4, MT = 2;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* red = reinterpret_cast<float*>(smem);                 // [NW][MT][256]
    unsigned char* ring = smem + (size_t)NW * MT * 1024;         // [NW][WIN][4 KiB]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int my_tiles = (ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
    // epilogue role of this lane: output (token em, tile column ec); its partial sits at index eidx of tile emt of every wave
    const int ec = tid & 15, em = tid >> 4, emt = em >> 4;
    const int eidx = (em & 3) * 64 + ((em >> 2) & 3) * 16 + ec;
    float best_v = -__builtin_inff();
    int best_i = 0x7fffffff;

    const int r = lane & 15, g = lane >> 4;
    f16x8 af[MT][16];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) {
        const int row = r + 16 * mt;
        const f16* xrow = x + (size_t)(row < M ? row : 0) * K + wave * 512 + g * 8;
#pragma unroll
        for (int s2 = 0; s2 < 16; s2++) af[mt][s2] = *reinterpret_cast<const f16x8*>(xrow + s2 * 32);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // before the first LDS-DMA load: hipcc's own waits do not know them
    const u32 my0 = (u32)(unsigned long long)(__attribute__((address_space(3))) unsigned char*)ring + (u32)wave * (WIN * 4096);
    const int lrow = lane >> 4;
    auto issue_group = [&](int gi) {   // as in gemm_f16_sdma_kernel
        const int t = blockIdx.x + (gi >> 2) * (int)gridDim.x;
        const unsigned char* base = reinterpret_cast<const unsigned char*>(wt + (size_t)t * 16 * K) + wave * 1024 + (gi & 3) * 256;
        const u32 dst = my0 + (u32)(gi & (WIN - 1)) * 4096u;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int row = 4 * q + lrow;
            glds16<1>(base + (size_t)row * (K * 2) + (((lane & 15) ^ row) << 4), dst + (u32)q * 1024u);
        }
    };
    const int n_groups = my_tiles * 4;
#pragma unroll
    for (int gi = 0; gi < WIN; gi++)
        if (gi < n_groups) issue_group(gi);
    typedef __attribute__((address_space(3))) u32x4 lds_u32x4_t;
    const __attribute__((address_space(3))) unsigned char* my3 =
        (const __attribute__((address_space(3))) unsigned char*)ring + (size_t)wave * (WIN * 4096);
    u32 foff[4];
#pragma unroll
    for (int q2 = 0; q2 < 4; q2++) foff[q2] = (u32)(r >> 2) * 1024u + (u32)((((r & 3) << 4) | ((q2 * 4 + g) ^ r)) << 4);
    f32x4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; mt++) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    int gi = 0, tile = blockIdx.x;
    for (int ti = 0; ti < my_tiles; ti++) {
        const bool last = ti == my_tiles - 1;   // (wave-uniform) the window runs empty behind the last tile
#pragma unroll
        for (int seg = 0; seg < 4; seg++, gi++) {
            if (!last) vmcnt_le<12>();
            else if (seg == 0) vmcnt_le<12>();
            else if (seg == 1) vmcnt_le<8>();
            else if (seg == 2) vmcnt_le<4>();
            else vmcnt_le<0>();
            u32x4 wv[4];
#pragma unroll
            for (int q2 = 0; q2 < 4; q2++)
                wv[q2] = *reinterpret_cast<const volatile lds_u32x4_t*>(my3 + (size_t)seg * 4096 + foff[q2]);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (gi + WIN < n_groups) issue_group(gi + WIN);   // into the slot just read
#pragma unroll
            for (int q2 = 0; q2 < 4; q2++)
#pragma unroll
                for (int mt = 0; mt < MT; mt++)
                    acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[mt][seg * 4 + q2], __builtin_bit_cast(f16x8, wv[q2]), acc[mt], 0, 0, 0);
        }
        __builtin_amdgcn_s_barrier();   // B: every lane has read the previous tile's partials
#pragma unroll
        for (int mt = 0; mt < MT; mt++) {
#pragma unroll
            for (int i = 0; i < 4; i++) red[(wave * MT + mt) * 256 + i * 64 + lane] = acc[mt][i];
            acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();   // A: the tile's partials are posted
        if (em < M) {
            float sum = red[emt * 256 + eidx];
#pragma unroll
            for (int w2 = 1; w2 < NW; w2++) sum = sum + red[(w2 * MT + emt) * 256 + eidx];
            const f16 hv = f2h(sum);
            out[(size_t)em * N + tile * 16 + ec] = hv;
            const float fv = h2f(hv);
            if (fv > best_v) {          // tiles come in increasing column order: a tie keeps the first column
                best_v = fv;
                best_i = tile * 16 + ec;
            }
        }
        tile += gridDim.x;
    }
    if (part_max) {   // the 16 columns of a row sit in 16 consecutive lanes: larger value, then smaller column, wins
#pragma unroll
        for (int mk = 1; mk < 16; mk <<= 1) {
            const float ov = __shfl_xor(best_v, mk, 64);
            const int oi = __shfl_xor(best_i, mk, 64);
            if (ov > best_v || (ov == best_v && oi < best_i)) {
                best_v = ov;
                best_i = oi;
            }
        }
        if (em < M && ec == 0) part_max[(size_t)em * gridDim.x + blockIdx.x] = HeadMax{best_v, best_i};
    }
}
// (dev knob QSPEC_HEAD_SDMA=0: the register-streaming lm_head)
static bool head_sdma_on() {
    static const int v = QS_DEV_KNOB("QSPEC_HEAD_SDMA", 1);
    return v != 0;
}

// (MT = 2 of THIS kernel -- 17..32 tokens as two token tiles over one weight pass -- was built and measured in round 3: 240 us
// against 245 for the M-tiled kernel at M = 32: the second tile's 64 fragment registers push the kernel to 168 VGPRs + scratch
// at 12 waves, and scratch traffic shares the vmcnt queue with the LDS-DMA window.  gemm_f16_sdma2_kernel -- eight waves, all
// streaming, 184 VGPRs -- is what 17..32 tokens launch: 183 us.)
static int gemm_f16_sdma_launch(const f16* x, const f16* w, f16* out, int M, int N, int ntiles, int grid, HeadMax* pm,
                                hipStream_t st) {
    if (M > 16) {   // two token tiles: gemm_f16_sdma2_kernel
        const size_t lds = (size_t)8 * 2 * 1024 + (size_t)8 * 4 * 4096;
        if (const int rc = lds_optin<gemm_f16_sdma2_kernel>(lds, true)) return rc;
        hipLaunchKernelGGL(gemm_f16_sdma2_kernel, dim3(grid), dim3(8 * 64), lds, st, x, w, out, M, N, ntiles, pm);
        return 0;
    }
    const size_t lds = (size_t)2 * 8 * 1024 + (size_t)8 * 4 * 4096;
    if (const int rc = lds_optin<gemm_f16_sdma_kernel<1>>(lds, true)) return rc;
    hipLaunchKernelGGL(gemm_f16_sdma_kernel<1>, dim3(grid), dim3(12 * 64), lds, st, x, w, out, M, N, ntiles, pm);
    return 0;
}
// The register-streaming shapes, X(K, NW, UB, NB): K = 32 * NW * UB * NB; NB > 1 = several batches per tile
// (gemm_f16_longk_kernel; K = 8192: 256 steps of 64 bytes per row = 16 waves x 4 steps x 4 batches -- 8 x 2: 20 VGPRs spilled at
// 1024 threads).  Walked by gemm_f16_stream_supported and by the launch switch: a new K is one X() here.
#define QS_F16_SHAPES(X) X(4096, 8, 16, 1) X(2048, 8, 8, 1) X(1024, 4, 8, 1) X(5120, 8, 20, 1) X(8192, 16, 4, 4)
template <int NW, int UB, int NB>
static int gemm_f16_launch_inst(const f16* x, const f16* w, f16* out, int M, int N, int K, int ntiles, int grid, HeadMax* pm,
                                hipStream_t st) {
    if constexpr (NB > 1)
        hipLaunchKernelGGL((gemm_f16_longk_kernel<NW, UB, NB>), dim3(grid), dim3(NW * 64), (size_t)2 * NW * 1024, st, x, w, out, M,
                           N, K, ntiles, pm);
    else
        hipLaunchKernelGGL((gemm_f16_stream_kernel<NW, UB>), dim3(grid), dim3(NW * 64), (size_t)2 * NW * 1024, st, x, w, out, M, N,
                           K, ntiles, pm);
    return 0;
}
static bool f16_stream_shape(int K) {
#define X(KV, NWV, UBV, NBV) if (K == KV) return true;
    QS_F16_SHAPES(X)
#undef X
    return false;
}
// 17..32 tokens: the two-token-tile LDS-DMA form, for a long stream only (the lm_head: >= 4 tiles per workgroup)
static bool gemm_f16_stream2_supported(int M, int N, int K) {
    return M > 16 && M <= 32 && K == 4096 && N % 16 == 0 && N / 16 >= 4 * gemm_f16_stream_grid(N) && head_sdma_on();
}
bool gemm_f16_stream_supported(int M, int N, int K) {
    if (gemm_f16_stream2_supported(M, N, K)) return true;
    return M >= 1 && M <= 16 && N % 16 == 0 && f16_stream_shape(K);
}
int gemm_f16_stream_grid(int N) { return stream_grid(N / 16, 256); }
// part_max != NULL: the grid is gemm_f16_stream_grid(N) (<= 256) and part_max holds [M][grid] {float, int} pairs.
int gemm_f16_stream(const f16* x, const f16* w, f16* out, int M, int N, int K, void* part_max, hipStream_t st) {
    if (!gemm_f16_stream_supported(M, N, K)) return -1;
    const int ntiles = N / 16;
    static const int cap_knob = QS_DEV_KNOB("QSPEC_HEAD_CAP", 256);   // one workgroup per CU: 6.3 TB/s measured (512: 6.1, 1024: 5.9)
    const int cap = cap_knob < 1 ? 256 : cap_knob;
    const int grid = (part_max || M > 16) ? gemm_f16_stream_grid(N) : stream_grid(ntiles, cap);
    HeadMax* pm = reinterpret_cast<HeadMax*>(part_max);
    if (K == 4096 && ntiles >= 4 * grid && head_sdma_on()) {   // a long stream: LDS-DMA (see gemm_f16_sdma_kernel)
        return gemm_f16_sdma_launch(x, w, out, M, N, ntiles, grid, pm, st);
    }
#define X(KV, NWV, UBV, NBV) if (K == KV) return gemm_f16_launch_inst<NWV, UBV, NBV>(x, w, out, M, N, K, ntiles, grid, pm, st);
    QS_F16_SHAPES(X)
#undef X
    return -1;
}

}  // namespace qspec
