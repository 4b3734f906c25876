// EXPERIMENTAL -- not part of libqspec_hip.so.  Measured and rejected variants (DESIGN.md section 4, "Measured and rejected");
// included into gemm_stream_w4a4.hip only under -DQS_EXPERIMENTAL (make -C qspec_amd/csrc experimental -> libqspec_hip_experimental.so),
// kept with their tests (which select that library through QSPEC_HIP_LIB) for the record.

// ------------------------------------------------------------------ loader / consumer form ("engine"), M <= 4
// The same GEMM with the weights brought in by LDS-DMA (global_load_lds_dwordx4 nt) instead of register loads:
//   * waves 4..7 = LOADERS, one per SIMD.  They do nothing but issue 1-KiB LDS-DMA loads of the workgroup's weight tiles
//     into a ring of 16-KiB fills in LDS (fill = the f-th KiB of each of a tile's 16 rows; loader lw moves rows lw, lw+4,
//     lw+8, lw+12), run ahead of the consumers by up to the ring, and publish per-loader `landed` counters behind counted
//     `s_waitcnt vmcnt`.  A loader that blocks at the issue (a CU holds ~32 KB of loads in flight) blocks nobody else.
//     Measured floor (scripts/micro/ldsdma.hip, nobody consuming, launch boundary included): gate_up 9.65 us, qkv 3.6,
//     o 2.75, down 5.6 -- against 10.5 / 3.9 / 3.0 / 6.7 for the register path's PURE read of the same bytes and
//     13.3 / 6.7 / 4.85 / 8.4 for the register kernels as the cycle runs them.  ONE loader wave per CU reaches only 2.5 TB/s.
//   * waves 0..3 = CONSUMERS: first the prologue (norm + int4 quant of row `wave`, one wave per row, no barrier inside:
//     lnw_*), then per fill: wait for the four `landed` counters, four ds_read_b128 fragments (conflict-free: the row
//     XOR swizzle sits on the loaders' SOURCE addresses, the LDS image stays lane-linear), publish `consumed`, 8 MFMAs.
//     Consumer cw owns K steps cw, cw+4, cw+8, cw+12 of every fill; its activation fragments stay in registers.
//   * no s_barrier after the first one (row requests before weight requests): everything else is LDS counters, so a
//     loader never waits for a consumer except for ring space and a consumer never waits for a loader except for data.
//   * wave 0 is also the epilogue wave (M <= 4: 64 (token, column) pairs): it sums the four int32 partials (exact: same
//     bits as any other partition of K) once waves 1..3 have posted theirs and applies the same epilogue expressions.
// Every spin is bounded (a lost partner ends in wrong results and a failed test, not in a hung GPU).
// Flag words live in LDS and are accessed through address-space-3 pointers: a VOLATILE access through a generic pointer
// is not rewritten by hipcc's address-space inference and becomes flat_load / flat_store (sc0 sc1) + s_waitcnt vmcnt(0) --
// on a loader that drains every LDS-DMA load in flight at each publish (first version of this kernel: 15.9 us).
typedef __attribute__((address_space(3))) int lds_int_t;
typedef __attribute__((address_space(3))) i32x4 lds_i32x4_t;
__device__ __forceinline__ int lds_min4(const int* p) {   // four counters, one broadcast ds_read_b128
    const i32x4 v = *reinterpret_cast<const volatile lds_i32x4_t*>((const lds_int_t*)p);
    return min(min(v[0], v[1]), min(v[2], v[3]));
}
__device__ __forceinline__ int lds_flag_load(const int* p) { return *reinterpret_cast<const volatile lds_int_t*>((const lds_int_t*)p); }
__device__ __forceinline__ void lds_flag_store(int* p, int v) { *reinterpret_cast<volatile lds_int_t*>((lds_int_t*)p) = v; }
#define QS_ENG_SPIN_GUARD (1 << 20)
#ifndef QS_ENG_RING
#define QS_ENG_RING 8    // fills of 16 KiB
#endif
#ifndef QS_ENG_DEPTH
#define QS_ENG_DEPTH 5   // fills a loader keeps in flight behind the one it publishes (4 KiB each): throughput = bytes in
                         // flight / latency (~3 us under load), and what LDS-DMA can keep in flight is bounded by ring space
                         // only -- 64 KB per CU in flight gave 20 GB/s per CU, the floor needs >= 90 KB
#endif
#ifndef QS_ENG_NT
#define QS_ENG_NT 1
#endif
#ifndef QS_ENG_EARLY
#define QS_ENG_EARLY 1   // 1: the loaders start at once (one barrier, right at the start, publishes the zeroed flags);
#endif                   // 0: they wait until the consumers' row requests are out
#define QS_ENG_BARRIER() do { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_s_barrier(); } while (0)
enum { ENG_FLAGS = 0, ENG_XS = 256, ENG_XQ = 512 };
__host__ __device__ inline size_t eng_red_off(int K) { return ENG_XQ + (size_t)4 * (K / 2 + 32); }
__host__ __device__ inline size_t eng_ring_off(int K) { return (eng_red_off(K) + 4 * 4 * 256 + 1023) & ~(size_t)1023; }
#ifdef QS_ENG_STAMPS
__host__ __device__ inline size_t eng_lds_bytes(int K, int R) { return eng_ring_off(K) + (size_t)R * 16384 + 6 * 64 * 8; }
#else
__host__ __device__ inline size_t eng_lds_bytes(int K, int R) { return eng_ring_off(K) + (size_t)R * 16384; }
#endif

#ifdef QS_ENG_STAMPS
__device__ long long g_engst[6][64];   // [consumer wave 0 | loaders 0..3 | epilogue wave] of workgroup 100, s_memrealtime (100 MHz)
// stamps go to LDS (no vector-memory traffic of their own: a global store would count in the loaders' vmcnt) and are
// copied out at the end
#define QS_ESTAMP(who, i) do { long long t_; asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory"); \
                               if (lane == 0 && (i) < 64) est[(who) * 64 + (i)] = t_; } while (0)
#define QS_ESTAMP_DUMP(who) do { if (blockIdx.x == 100) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); g_engst[who][lane] = est[(who) * 64 + lane]; } } while (0)
#else
#define QS_ESTAMP(who, i)
#define QS_ESTAMP_DUMP(who)
#endif
#ifndef QS_ENG_NC
#define QS_ENG_NC 4      // consumer waves
#endif
#ifndef QS_ENG_NE
#define QS_ENG_NE 2      // epilogue waves, tile ti -> wave ti % NE (an epilogue is a ~0.4 us dependent chain per tile)
#endif
template <int EPI, int PRO, int NI, int FPT /* fills per tile = K / 2048 */, int R /* ring, in fills */>
__global__ __launch_bounds__((QS_ENG_NC + 4 + QS_ENG_NE) * 64) void gemm_w4a4_engine_kernel(StreamArgs a) {
    static_assert(PRO == PRO_LN1S || PRO == PRO_LNS || PRO == PRO_Q, "prologues built so far");
    static_assert(EPI == SEPI_GATEUP || EPI == SEPI_RESID, "epilogues built so far");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int NC = QS_ENG_NC, NE = QS_ENG_NE;
    constexpr bool AF_REGS = FPT * 4 <= 8;   // the wave's activation fragments live in registers (else: read per step from LDS)
    constexpr int SPF = 16 / NC;   // K steps of a fill per consumer wave
    static_assert(R >= 7 && R <= 9, "ring: two fills per loader in flight");
    static_assert(NC == 4, "consumer cw takes unit cw (K steps 4 cw .. 4 cw + 3) of every fill");
    static_assert(NE == 1 || NE == 2 || NE == 4, "epilogue waves (4 slots of partial sums)");
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Kb = a.K >> 1, RS = Kb + 32;
    int* flags = reinterpret_cast<int*>(smem + ENG_FLAGS);
    int* landed = flags;          // [4] fills of loader lw that have landed
    int* consumed = flags + 4;    // [8] fills whose fragments consumer cw holds in registers
    int* done = flags + 12;       // [8] tiles whose partial sums consumer cw has posted
    int* rows_done = flags + 20;  // [4] row r is quantised
    int* epi_done = flags + 24;   // [4] per slot of `red`: tiles of that slot the epilogue has taken out
    float* xs_lds = reinterpret_cast<float*>(smem + ENG_XS);
    unsigned char* xq_lds = smem + ENG_XQ;
    int* red = reinterpret_cast<int*>(smem + eng_red_off(a.K));   // [4 tile slots][NC waves][64]: (token m < 4, column c) at m * 16 + c
    unsigned char* ring = smem + eng_ring_off(a.K);
#ifdef QS_ENG_STAMPS
    long long* est = reinterpret_cast<long long*>(ring + (size_t)R * 16384);
#endif
    static_assert(FPT <= R, "");
    const int my_tiles = (a.ntiles - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;   // >= 1
    const int n_fills = my_tiles * FPT;
    auto min_consumed = [&]() { return NC == 8 ? min(lds_min4(consumed), lds_min4(consumed + 4)) : lds_min4(consumed); };
    auto min_done = [&]() { return NC == 8 ? min(lds_min4(done), lds_min4(done + 4)) : lds_min4(done); };
    if (tid < 32) flags[tid] = 0;
    QS_ENG_BARRIER();   // the zeroed flags are visible to every wave

    if (wave >= NC && wave < NC + 4) {   // ---------------------------------------------------------------- loaders
        const int lw = wave - NC;
        const u32 ring0 = (u32)(unsigned long long)(__attribute__((address_space(3))) unsigned char*)ring;
#ifdef QS_ENG_LOADER_PRIO
        __builtin_amdgcn_s_setprio(QS_ENG_LOADER_PRIO);   // (measured: prio 3 starves the norm wave on the same SIMD)
#endif
        QS_ESTAMP(1 + lw, 0);
        if (!QS_ENG_EARLY) QS_ENG_BARRIER();   // the consumers' row requests are out (the CU's L1 returns in request order)
        QS_ESTAMP(1 + lw, 1);
        // Loader lw moves fills lw, lw + 4, lw + 8, ... WHOLE, as four UNITS of four LDS-DMA loads: unit u = K steps 4u .. 4u+3
        // (256 bytes of each of the 16 rows; one load = 4 rows x 256 B, lane l -> row l / 16, 16-byte piece (l % 16) ^ row),
        // which is exactly what consumer u needs of the fill.  It keeps 16 loads in flight and publishes in units: what it
        // learns from `vmcnt(16)` behind unit j is that unit j - 4 has landed -- and since the memory system paces the issue
        // (a new load goes out when an old one completes) that is within one unit of the landing itself, at every point of
        // the stream including its end (drained with vmcnt 12, 8, 4, 0).  Four loaders x 16 KB in flight = what the CU's
        // queues hold anyway.  (Earlier forms published whole fills behind the issue of the NEXT whole fill: the last two
        // fills of every loader became visible in one burst at the very end and the consumers needed 1.3 us to work it off.)
        int units = 0;   // own units issued
        for (int n = lw; n < n_fills; n += 4) {
            if (n >= R) {   // ring space: every consumer has taken fill n - R out
                int guard = 0;
                while (min_consumed() < n - R + 1 && ++guard < QS_ENG_SPIN_GUARD) __builtin_amdgcn_s_sleep(1);
            }
            const int ti = n / FPT, f = n - ti * FPT;
            const int tile = blockIdx.x + ti * (int)gridDim.x;
            const u32 dst = ring0 + (u32)(n % R) * 16384u;
#pragma unroll
            for (int u = 0; u < 4; u++) {
#pragma unroll
                for (int gq = 0; gq < 4; gq++) {
                    const int row = 4 * gq + (lane >> 4);
                    const uint8_t* src = a.wq + (size_t)stile_row<EPI>(tile, row, a.I, a.hdl) * Kb + (size_t)f * 1024 + u * 256 +
                                         (((lane & 15) ^ row) << 4);
                    glds16<QS_ENG_NT>(src, dst + (u32)(u * 4 + gq) * 1024u);
                }
                units++;
                if (units > 4) {
                    asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
                    if (lane == 0) lds_flag_store(landed + lw, units - 4);
                }
            }
            QS_ESTAMP(1 + lw, 2 + (units >> 2));       // own fill issued
        }
        asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
        if (lane == 0) lds_flag_store(landed + lw, units - 3);
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        if (lane == 0) lds_flag_store(landed + lw, units - 2);
        asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        if (lane == 0) lds_flag_store(landed + lw, units - 1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) lds_flag_store(landed + lw, units);
        const int own = units >> 2;
        QS_ESTAMP(1 + lw, 3 + own);
        QS_ESTAMP_DUMP(1 + lw);
        return;
    }

    const int c = lane & 15, m = lane >> 4;   // epilogue lanes: (token m, tile column c)
    if (wave >= NC + 4) {   // ---------------------------------------------------------------- epilogue waves
        const int ew = wave - (NC + 4);
        if (!QS_ENG_EARLY) QS_ENG_BARRIER();
        const bool ethread = m < a.M;
        const int mc = m < a.M ? m : 0;
        int tile = blockIdx.x + ew * (int)gridDim.x;
        // The channel scales of ALL this wave's tiles are requested now, before the loaders have filled the CU's memory
        // queue: the vector L1 returns in request order across waves, a 2-byte load issued mid-stream waits behind ~64 KB
        // of LDS-DMA (2 us; first version: every epilogue sat in s_waitcnt vmcnt(0) for its scale).
        constexpr int MAXE = EPI == SEPI_RESID ? 2 : 8;   // tiles per epilogue wave (host: ntiles <= 256 * NE * MAXE)
        f16 swn_all[MAXE], res_all[MAXE];
#pragma unroll
        for (int i = 0; i < MAXE; i++) {
            const int tl = min(blockIdx.x + (ew + i * NE) * (int)gridDim.x, a.ntiles - 1);   // clamped: no branch around a load
            swn_all[i] = a.ws[stile_row<EPI>(tl, c, a.I, a.hdl)];
            if (EPI == SEPI_RESID) res_all[i] = a.resid_in[(size_t)mc * a.N + tl * 16 + c];   // the residual element
        }
        float xs_pre = 0.0f;
        if (PRO == PRO_Q) xs_pre = h2f(a.xs[mc]);
        {
            int guard = 0;
            while (lds_min4(rows_done) < 1 && ++guard < QS_ENG_SPIN_GUARD) __builtin_amdgcn_s_sleep(2);
            asm volatile("" ::: "memory");
        }
        const float xs_m = PRO == PRO_Q ? xs_pre : xs_lds[mc];
        int taken = 0;
#pragma unroll
        for (int i = 0; i < MAXE; i++) {
            const int ti = ew + i * NE;
            if (ti >= my_tiles) break;
            const f16 swn = swn_all[i];
            int guard = 0;
            while (min_done() < ti + 1 && ++guard < QS_ENG_SPIN_GUARD) __builtin_amdgcn_s_sleep(1);
            asm volatile("" ::: "memory");
            const int* rb = red + (ti & 3) * (NC * 64);
            int sum = 0;
#pragma unroll
            for (int w2 = 0; w2 < NC; w2++) sum += rb[w2 * 64 + lane];
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            // the slot's sums are in registers.  (NE < 4: a wave serves slots ti & 3 = ew, ew + NE, ...; each slot's counter
            // counts the tiles taken out of THAT slot: tile ti is number ti / 4 + 1 of slot ti & 3)
            if (lane == 0) lds_flag_store(epi_done + (ti & 3), (ti >> 2) + 1);
            taken++;
            const float v = ((float)(sum >> 8) * xs_m) * h2f(swn);  // both operands carried a factor 16
            const f16 hv = f2h(v);
            if (EPI == SEPI_RESID) {   // hidden = residual + proj_out, an fp16 add of two fp16 tensors (quarot_llama.py:380,390)
                if (ethread) a.resid_out[(size_t)m * a.N + tile * 16 + c] = f2h(h2f(res_all[i]) + h2f(hv));
            }
            if (EPI == SEPI_GATEUP) {
                const f16 partner = u2h((uint16_t)__shfl_xor((int)h2u(hv), 8, 64));
                if (ethread) stream_epilogue_pair<SEPI_GATEUP>(a, tile, m, c, hv, partner, swn, swn, 0);   // (cf / sf: unused)
            }
            if (ew == 0) QS_ESTAMP(5, ti);
            tile += NE * (int)gridDim.x;
        }
        if (ew == 0) QS_ESTAMP_DUMP(5);
        return;
    }

    // ---------------------------------------------------------------- consumers
    const int cw = wave;
    const int r = lane & 15, g = lane >> 4;
    if constexpr (PRO == PRO_Q) {   // (xq, xs) given: consumer cw copies packed row cw into LDS (16 bytes per lane and pass)
        const int row = cw < a.M ? cw : 0;
        const unsigned char* src = reinterpret_cast<const unsigned char*>(a.xq) + (size_t)row * Kb;
        for (int o = lane * 16; o < Kb; o += 1024)
            *reinterpret_cast<u32x4*>(xq_lds + (size_t)cw * RS + o) = *reinterpret_cast<const u32x4*>(src + o);
        if (!QS_ENG_EARLY) QS_ENG_BARRIER();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (lane == 0) lds_flag_store(rows_done + cw, 1);
        int guard = 0;
        while (lds_min4(rows_done) < 1 && ++guard < QS_ENG_SPIN_GUARD) __builtin_amdgcn_s_sleep(1);
        asm volatile("" ::: "memory");
    } else {   // prologue: norm + int4 quant of row cw (consumers 0..3; the others only wait)
        constexpr bool HASD = PRO == PRO_LNS;
        LnwRegs<NI> rg;
        if (cw == 0) QS_ESTAMP(0, 0);
        if (cw < 4) lnw_load<NI, HASD>(a, cw, rg);   // (wave-uniform branch; the loads it guards are this wave's first)
        __builtin_amdgcn_sched_barrier(0);
        if (cw == 0) QS_ESTAMP(0, 1);
        if (!QS_ENG_EARLY) QS_ENG_BARRIER();
        if (cw == 0) QS_ESTAMP(0, 2);
        __builtin_amdgcn_sched_barrier(0);
        if (cw < 4) {
            if (cw < a.M) lnw_compute<NI, HASD>(a, cw, rg, xq_lds, RS, xs_lds, blockIdx.x == 0 && a.hidden_out != nullptr);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            if (cw == 0) QS_ESTAMP(0, 3);     // own row quantised
            if (lane == 0) lds_flag_store(rows_done + cw, 1);
        }
        int guard = 0;
        while (lds_min4(rows_done) < 1 && ++guard < QS_ENG_SPIN_GUARD) __builtin_amdgcn_s_sleep(1);
        asm volatile("" ::: "memory");
        if (cw == 0) QS_ESTAMP(0, 4);     // all rows there
    }
    // this wave's activation fragments: steps cw, cw + NC, ... of every KiB piece of the row
    const unsigned char* arow = xq_lds + (size_t)(r & 3) * RS + g * 16 + (4 * cw) * 64;   // + f * 1024 + q * 64
    constexpr int NAF = AF_REGS ? FPT * SPF : 1;
    i32x4 af0[NAF], af1[NAF];
    if constexpr (AF_REGS) {
#pragma unroll
        for (int f = 0; f < FPT; f++)
#pragma unroll
            for (int q = 0; q < SPF; q++) {
                const u32x4 av = *reinterpret_cast<const u32x4*>(arow + f * 1024 + q * 64);
                af0[f * SPF + q] = widen16(av[0], av[1]);
                af1[f * SPF + q] = widen16(av[2], av[3]);
            }
    }
    // fragment address inside a fill: unit cw, load r / 4 of the unit, lane (r % 4) * 16 + ((step q * 4 + g) ^ r)
    u32 foff[SPF];
#pragma unroll
    for (int q = 0; q < SPF; q++)
        foff[q] = (u32)(cw * 4 + (r >> 2)) * 1024u + (u32)((((r & 3) << 4) | ((q * 4 + g) ^ r)) << 4);
    if (cw == 0) QS_ESTAMP(0, 5);
    // Software pipeline over the fills: the flags AND the fragments of fill n + 1 are read speculatively (flags first:
    // LDS executes a wave's accesses in order, so fragments read behind flags that already said "landed" are the landed
    // bytes) while fill n is widened and multiplied; only a fill that had not landed yet is polled for and read again.
    // One LDS round trip per fill on the critical path instead of three; FPT independent accumulator chains.
    typedef __attribute__((address_space(3))) u32x4 lds_u32x4_t;
    const __attribute__((address_space(3))) unsigned char* ring3 = (const __attribute__((address_space(3))) unsigned char*)ring;
    struct Spec {
        i32x4 fl;
        u32x4 w[SPF];
    };
    auto spec_load = [&](Spec& x, int slot_i) {
        x.fl = *reinterpret_cast<const volatile lds_i32x4_t*>((const lds_int_t*)landed);
#pragma unroll
        for (int q = 0; q < SPF; q++)
            x.w[q] = *reinterpret_cast<const volatile lds_u32x4_t*>(ring3 + (size_t)slot_i * 16384 + foff[q]);
    };
    auto confirm = [&](Spec& x, int nn, int slot_i) {   // fill nn is in x.w when this returns
        const int who = nn & 3, need = 4 * (nn >> 2) + cw + 1;   // unit cw of own fill nn / 4 of loader nn % 4
        const int have = who == 0 ? x.fl[0] : (who == 1 ? x.fl[1] : (who == 2 ? x.fl[2] : x.fl[3]));
        if (have < need) {   // (wave-uniform)
            int guard = 0;
            while (lds_flag_load(landed + who) < need && ++guard < QS_ENG_SPIN_GUARD) __builtin_amdgcn_s_sleep(1);
#pragma unroll
            for (int q = 0; q < SPF; q++)
                x.w[q] = *reinterpret_cast<const volatile lds_u32x4_t*>(ring3 + (size_t)slot_i * 16384 + foff[q]);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (lane == 0) lds_flag_store(consumed + cw, nn + 1);
    };
    int n = 0, cslot = 0;
    Spec sp[2];
    spec_load(sp[0], 0);
    for (int ti = 0; ti < my_tiles; ti++) {
        i32x4 acc[FPT];
#pragma unroll
        for (int f = 0; f < FPT; f++) {
            acc[f] = i32x4{0, 0, 0, 0};
            Spec& cur = sp[f & 1];
#ifdef QS_ENG_STAMPS2
            if (cw == 0 && n >= 10) QS_ESTAMP(0, 20 + 5 * (n - 10) + 0);   // before confirm
#endif
            confirm(cur, n, cslot);
            if (cw == 0) QS_ESTAMP(0, 6 + n);     // fill n in registers
            cslot = cslot + 1 == R ? 0 : cslot + 1;
            n++;
            if (n < n_fills) spec_load(sp[(f + 1) & 1], cslot);
#ifdef QS_ENG_STAMPS2
            if (cw == 0 && n - 1 >= 10) QS_ESTAMP(0, 20 + 5 * (n - 11) + 1);   // next spec loads issued (+ their wait: the stamp drains lgkmcnt)
#endif
            u32x4 av[SPF];
            if constexpr (!AF_REGS) {
#pragma unroll
                for (int q = 0; q < SPF; q++) av[q] = *reinterpret_cast<const u32x4*>(arow + f * 1024 + q * 64);
            }
#pragma unroll
            for (int q = 0; q < SPF; q++) {
                const i32x4 b0 = widen16(cur.w[q][0], cur.w[q][1]), b1 = widen16(cur.w[q][2], cur.w[q][3]);
                const i32x4 a0 = AF_REGS ? af0[AF_REGS ? f * SPF + q : 0] : widen16(av[q][0], av[q][1]);
                const i32x4 a1 = AF_REGS ? af1[AF_REGS ? f * SPF + q : 0] : widen16(av[q][2], av[q][3]);
                acc[f] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, b0, acc[f], 0, 0, 0);
                acc[f] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, b1, acc[f], 0, 0, 0);
            }
#ifdef QS_ENG_STAMPS2
            if (cw == 0 && n - 1 >= 10) {
                asm volatile("" :: "v"(acc[f]));   // (the MFMAs have been issued; s_memrealtime does not wait for their results)
                QS_ESTAMP(0, 20 + 5 * (n - 11) + 2);
            }
#endif
        }
#pragma unroll
        for (int f = 1; f < FPT; f++) acc[0] = acc[0] + acc[f];
        // post this wave's partial sums into slot ti % 4 of `red` (free once the epilogue has taken tile ti - 4 out of it)
        if (ti >= 4) {
            int guard = 0;
            while (lds_flag_load(epi_done + (ti & 3)) < (ti >> 2) && ++guard < QS_ENG_SPIN_GUARD) __builtin_amdgcn_s_sleep(1);
            asm volatile("" ::: "memory");
        }
        // (the MFMA leaves (token m, column c) in acc[m & 3] of lane (m >> 2) * 16 + c: M <= 4 -> lanes 0..15 hold it all)
        int* rb = red + (ti & 3) * (NC * 64);
        if (lane < 16) {
#pragma unroll
            for (int i = 0; i < 4; i++) rb[cw * 64 + i * 16 + lane] = acc[0][i];
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (lane == 0) lds_flag_store(done + cw, ti + 1);
#ifdef QS_ENG_STAMPS2
        if (cw == 0 && n - 1 >= 10) QS_ESTAMP(0, 20 + 5 * (n - 11) + 3);   // tile posted
#endif
    }
    if (cw == 0) QS_ESTAMP_DUMP(0);
}

// QSPEC_ENGINE=1 selects the loader / consumer forms where they exist (gate_up + norm and down_proj + residual at M <= 4).
// OFF by default: measured in round 3 (same box, same graph, cold weights) the gate_up form runs 12.5-13.0 us against
// 13.2-13.4 for the register kernel and the down_proj form 10.4 against 8.5, although the loaders alone reach the LDS-DMA
// floor (9.65 / 5.6 us): the four consumer waves take ~0.45 us per 16-KiB fill where their instruction count says ~0.2,
// and run 1-2 us behind the data at the end of the stream (DESIGN.md, "Stage A").  Bit-identical to the register forms.
static int g_engine = -1;
static bool engine_on() {
    if (g_engine < 0) {
        const char* e = getenv("QSPEC_ENGINE");
        g_engine = (e && e[0] == '1') ? 1 : 0;
    }
    return g_engine != 0;
}
template <int EPI, int PRO, int NI, int FPT, int R>
static int launch_engine_inst(const StreamArgs& a, hipStream_t st) {
    const size_t lds = eng_lds_bytes(a.K, R);
    if (lds > 160 * 1024) return -7;
    auto kern = gemm_w4a4_engine_kernel<EPI, PRO, NI, FPT, R>;
    if (const int rc = lds_optin<gemm_w4a4_engine_kernel<EPI, PRO, NI, FPT, R>>(lds, true)) return rc;
    const int grid = a.ntiles < 256 ? a.ntiles : 256;   // one workgroup per CU
    if ((a.ntiles + grid - 1) / grid > (EPI == SEPI_RESID ? 2 : 8) * QS_ENG_NE) return -9;   // scales held per epilogue wave
    hipLaunchKernelGGL(kern, dim3(grid), dim3((QS_ENG_NC + 4 + QS_ENG_NE) * 64), lds, st, a);
    return 0;
}

