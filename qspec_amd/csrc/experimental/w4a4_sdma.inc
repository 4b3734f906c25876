// EXPERIMENTAL -- not part of libqspec_hip.so.  Measured and rejected variants (DESIGN.md section 4, "Measured and rejected");
// included into gemm_stream_w4a4.hip only under -DQS_EXPERIMENTAL (make -C qspec_amd/csrc experimental -> libqspec_hip_experimental.so),
// kept with their tests (which select that library through QSPEC_HIP_LIB) for the record.

// ------------------------------------------------------------------ self-service LDS-DMA form, M <= 4, K = 4096
// The register-streaming kernel above with its weight loads replaced by LDS-DMA that every stream wave issues FOR ITSELF:
// wave w brings its own four 1-KiB pieces of a tile (its K steps of the 16 rows: exactly the bytes its four register loads
// fetched) into a private quarter of an LDS slot with `global_load_lds_dwordx4 ... nt`, R tiles ahead, and learns that they
// have landed from its OWN `s_waitcnt vmcnt(4 (R - 1))` -- no loader waves, no flags, no cross-wave hand-off of data.
// Why it is faster than registers: a register-streaming CU holds ~32 KB of loads in flight (a wave stalls at the issue
// beyond that) and every tile in flight costs 4 VGPRs x 4 steps; LDS-DMA loads are subject to neither, so R = 4 tiles =
// 128 KB per CU are requested before the norm prologue has even started, and the stream runs underneath the prologue, the
// reductions and the epilogues at what the memory system delivers (scripts/micro/ldsdma.hip: 7.3 TB/s with four issuing
// waves per CU against 6.6 for the register path's pure read).  Why it is simpler than the loader / consumer engine above:
// the wave that waits for the bytes is the wave that uses them.
// The stream waves issue NO compiler-visible vector-memory operation after the prologue (hipcc's own vmcnt bookkeeping
// does not know the asm loads; a tracked load or store in the loop would make it wait for the run-ahead tiles): the
// epilogue -- channel scales, cos / sin, residual, stores -- belongs to one wave that streams nothing: norm wave 0 after
// the prologue (split-norm forms) or a wave of its own.  It meets the stream waves at ONE barrier per tile (partial sums
// posted -> summed; double buffered) and exchanges the rotary / gate partner by a lane shuffle.
template <int EPI, int PRO, int NI, int R>
__global__ __launch_bounds__(8 * 64 + 256) void gemm_w4a4_sdma_kernel(StreamArgs a) {
    static_assert(PRO == PRO_LN1S || PRO == PRO_LNS, "prologues built so far");
    static_assert(EPI == SEPI_GATEUP || EPI == SEPI_QKV, "epilogues built so far");
    static_assert(R >= 2 && R <= 4, "tiles in flight");
    constexpr int NW = 8, UB = 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 15, g = lane >> 4;
    const int Kb = a.K >> 1, RS = Kb + 32;
    unsigned char* xq_lds = smem;                                        // [4][RS]
    float* xs_lds = reinterpret_cast<float*>(smem + (size_t)4 * RS);     // [16]
    int* red = reinterpret_cast<int*>(xs_lds + 16);                      // [2][NW][64]: (token m < 4, column c) at m * 16 + c
    unsigned char* ring = smem + (((size_t)4 * RS + 64 + 2 * NW * 256 + 1023) & ~(size_t)1023);   // [R][32 KiB]
    const int my_tiles = (a.ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;      // >= 1
    constexpr bool HASD = PRO == PRO_LNS;

    if (tid >= NW * 64) {   // ---------------------------------------------------------------- norm waves; wave NW = epilogue
        const int row = wave - NW;
        LnwRegs<NI> rg;
        lnw_load<NI, HASD>(a, row, rg);
        // epilogue operands of ALL this workgroup's tiles, requested now (before the stream fills the CU's memory queue)
        const int c = lane & 15, m = lane >> 4;
        const int mc = m < a.M ? m : 0;
        constexpr int MAXT = EPI == SEPI_QKV ? 2 : 8;   // tiles per workgroup (host-checked)
        f16 swn[MAXT], cf[MAXT], sf[MAXT];
        int64_t pos_m = 0, slot_m = -1;
        if (row == 0) {
            if (EPI == SEPI_QKV) {
                pos_m = a.positions[mc];
                slot_m = a.slot_mapping[mc];
            }
#pragma unroll
            for (int i = 0; i < MAXT; i++) {
                const int tl = min((int)blockIdx.x + i * (int)gridDim.x, a.ntiles - 1);   // clamped: no branch around a load
                swn[i] = a.ws[stile_row<EPI>(tl, c, a.I, a.hdl)];
                if (EPI == SEPI_QKV) {
                    const int o = (tl & 7) * 8 + (c & 7);
                    const f16* cs = a.cos_sin_cache + pos_m * 128;
                    cf[i] = cs[o];
                    sf[i] = cs[64 + o];
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();   // #0: every row request is out before any weight request (in-order L1)
        __builtin_amdgcn_sched_barrier(0);
        if (row < a.M) lnw_compute<NI, HASD>(a, row, rg, xq_lds, RS, xs_lds, blockIdx.x == 0 && a.hidden_out != nullptr);
        __syncthreads();                // #1: publishes xq_lds / xs_lds
        if (row != 0) return;           // retired waves leave the workgroup's later barriers
        // ---- the epilogue wave: lane = (token m, tile column c)
        const bool ethread = m < a.M;
        const float xs_m = xs_lds[mc];
        int tile = blockIdx.x, par = 0;
#pragma unroll
        for (int i = 0; i < MAXT; i++) {
            if (i >= my_tiles) break;
            __syncthreads();            // A(i): the stream waves have posted tile i's partial sums
            const int* rb = red + par * NW * 64;
            int sum = 0;
#pragma unroll
            for (int w2 = 0; w2 < NW; w2++) sum += rb[w2 * 64 + lane];
            const float v = ((float)(sum >> 8) * xs_m) * h2f(swn[i]);  // both operands carried a factor 16
            const f16 hv = f2h(v);
            const f16 partner = u2h((uint16_t)__shfl_xor((int)h2u(hv), 8, 64));
            if constexpr (EPI == SEPI_GATEUP) {
                if (ethread) stream_epilogue_pair<EPI>(a, tile, m, c, hv, partner, cf[i], sf[i], slot_m);
            } else {   // SEPI_QKV: classic tiles, head size 128, fp16 caches only (the host checks) -- kept as its own text: the
                       // general tail of stream_common.cuh costs this kernel 2-4 more SGPRs
                const int head = tile >> 3, o = (tile & 7) * 8 + (c & 7);
                const int n = head * 128 + (c >> 3) * 64 + o;
                f16 res = hv;
                if (head < a.nq + a.nkv) {
                    const float cff = h2f(cf[i]), sff = h2f(sf[i]);
                    const float xf = h2f(c < 8 ? hv : partner), yf = h2f(c < 8 ? partner : hv);
                    res = c < 8 ? f2h(h2f(f2h(xf * cff)) - h2f(f2h(yf * sff))) : f2h(h2f(f2h(yf * cff)) + h2f(f2h(xf * sff)));
                }
                if (ethread) {
                    a.out[(size_t)m * a.N + n] = res;
                    if (head >= a.nq && slot_m >= 0) {
                        const bool is_k = head < a.nq + a.nkv;
                        const int kvh = is_k ? head - a.nq : head - a.nq - a.nkv;
                        f16* cache = is_k ? a.key_cache : a.value_cache;
                        cache[(slot_m * a.nkv + kvh) * 128 + (c >> 3) * 64 + o] = res;
                    }
                }
            }
            par ^= 1;
            tile += gridDim.x;
        }
        return;
    }

    // ---------------------------------------------------------------- stream waves
    const u32 ring0 = (u32)(unsigned long long)(__attribute__((address_space(3))) unsigned char*)ring;
    const u32 my_lds = ring0 + (u32)(wave * UB) * 1024u;    // this wave's quarter-KiB-pieces of slot 0 (+ slot * 32 KiB + u * 1 KiB)
    auto issue_tile = [&](int ti) {   // this wave's four pieces of the workgroup's ti-th tile
        const int t = blockIdx.x + ti * (int)gridDim.x;
        const uint8_t* wp = a.wq + (size_t)stile_row<EPI>(t, r, a.I, a.hdl) * Kb + g * 16;
        const u32 dst = my_lds + (u32)(ti % R) * 32768u;
#pragma unroll
        for (int u = 0; u < UB; u++) glds16<1>(wp + step_off<NW, UB>(wave, u), dst + (u32)u * 1024u);
    };
    __builtin_amdgcn_s_barrier();       // #0
#pragma unroll
    for (int ti = 0; ti < R; ti++)
        if (ti < my_tiles) issue_tile(ti);
    __builtin_amdgcn_s_barrier();       // #1: the packed rows and their scales are in LDS
    asm volatile("" ::: "memory");
    // A wave owns the same K steps of every tile: its activation fragments are widened once and stay in registers
    i32x4 af0[UB], af1[UB];
    {
        const unsigned char* arow = xq_lds + (size_t)(r & 3) * RS + g * 16;
#pragma unroll
        for (int u = 0; u < UB; u++) {
            const u32x4 av = *reinterpret_cast<const u32x4*>(arow + step_off<NW, UB>(wave, u));
            af0[u] = widen16(av[0], av[1]);
            af1[u] = widen16(av[2], av[3]);
        }
    }
    typedef __attribute__((address_space(3))) u32x4 lds_u32x4_t;
    const __attribute__((address_space(3))) unsigned char* my3 =
        (const __attribute__((address_space(3))) unsigned char*)ring + (size_t)(wave * UB) * 1024 + lane * 16;
    int par = 0;
    for (int ti = 0; ti < my_tiles; ti++) {
        // tile ti's four loads are the oldest of this wave's (4 per tile in flight, in issue order)
        const int ahead = min(R - 1, my_tiles - 1 - ti);   // tiles issued behind tile ti
        if (ahead >= 3) vmcnt_le<12>();
        else if (ahead == 2) vmcnt_le<8>();
        else if (ahead == 1) vmcnt_le<4>();
        else vmcnt_le<0>();
        u32x4 w[UB];
#pragma unroll
        for (int u = 0; u < UB; u++)
            w[u] = *reinterpret_cast<const volatile lds_u32x4_t*>(my3 + (size_t)(ti % R) * 32768 + u * 1024);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#ifndef QS_SDMA_LATE_ISSUE
        if (ti + R < my_tiles) issue_tile(ti + R);   // into the slot just read
#endif
        i32x4 acc = {0, 0, 0, 0};
#pragma unroll
        for (int u = 0; u < UB; u++) {
            const i32x4 b0 = widen16(w[u][0], w[u][1]), b1 = widen16(w[u][2], w[u][3]);
            acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(af0[u], b0, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(af1[u], b1, acc, 0, 0, 0);
        }
        // (the MFMA leaves (token m, column c) in acc[m & 3] of lane (m >> 2) * 16 + c: M <= 4 -> lanes 0..15 hold it all)
        int* rb = red + par * NW * 64;
        if (lane < 16) {
#pragma unroll
            for (int i = 0; i < 4; i++) rb[wave * 64 + i * 16 + lane] = acc[i];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();   // A(ti) (raw: a __syncthreads() here would wait for vmcnt(0), i.e. for the run-ahead tiles)
#ifdef QS_SDMA_LATE_ISSUE
        if (ti + R < my_tiles) issue_tile(ti + R);   // into the slot read above
#endif
        par ^= 1;
    }
}

template <int EPI, int PRO, int NI, int R>
static int launch_sdma_inst(const StreamArgs& a, hipStream_t st) {
    const size_t lds = (((size_t)4 * (a.K / 2 + 32) + 64 + 2 * 8 * 256 + 1023) & ~(size_t)1023) + (size_t)R * 32768;
    if (lds > 160 * 1024) return -7;
    auto kern = gemm_w4a4_sdma_kernel<EPI, PRO, NI, R>;
    if (const int rc = lds_optin<gemm_w4a4_sdma_kernel<EPI, PRO, NI, R>>(lds, true)) return rc;
    const int grid = a.ntiles < 256 ? a.ntiles : 256;   // one workgroup per CU
    if ((a.ntiles + grid - 1) / grid > (EPI == SEPI_QKV ? 2 : 8)) return -9;   // epilogue operands held per workgroup
    hipLaunchKernelGGL(kern, dim3(grid), dim3(8 * 64 + 256), lds, st, a);
    return 0;
}
#ifndef QS_SDMA_R
#define QS_SDMA_R 2
#endif
// QSPEC_SDMA=1 selects the self-service LDS-DMA forms (gate_up / qkv with the norm prologue, M <= 4, K = 4096).  OFF by
// default: measured in round 3, launches of ONE shape back to back run 12.9 us (R = 2; 13.5 / 13.9 with R = 3 / 4) against
// 13.65 for the register kernel, and qkv 5.9-6.3 against 6.7-6.8 -- but inside the cycle (and in bench.py's four-shape
// graph) gate_up does not gain (13.4-13.7 against 13.2-13.4) and the cycle LOSES 1.5 % (7.73-7.76 against 7.62 ms).
// More run-ahead is worse, not better: what a CU draws is not raised by requesting more (rounds 1 and 2 found the same
// for register loads), and the waves that issue the run-ahead loads sit in the issue while the queue is full.
static int g_sdma = -1;   // 0 off, 1 both shapes, 2 qkv only, 3 gate_up only
template <int EPI>
static bool sdma_on() {
    if (g_sdma < 0) {
        const char* e = getenv("QSPEC_SDMA");
        g_sdma = (e && e[0] >= '1' && e[0] <= '3') ? e[0] - '0' : 0;
    }
    return g_sdma == 1 || (g_sdma == 2 && EPI == SEPI_QKV) || (g_sdma == 3 && EPI == SEPI_GATEUP);
}

