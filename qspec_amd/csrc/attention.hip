// Paged causal attention, host side: the launch plan (attn_form), the workspace size and paged_attention().  The kernels and
// their launchers live in attention_decode.hip (head size 128: chunk and keys-over-waves kernels), attention_prefill.hip
// (prompt-sized queries) and attention_generic.hip (other head sizes); attention_common.cuh holds what they share.
#include <algorithm>

#include "attention_common.cuh"

namespace qspec {

// context splits the generic-head-size kernel uses for a caller's n_splits (shared with the merge in hadamard.hip)
int paged_attention_generic_splits(int n_splits) { return n_splits < 1 ? 1 : (n_splits > 4 ? 4 : n_splits); }   // (TinyLlama bs = 1, 512 / 1900 keys: 1: 4.61 / 6.27 ms per cycle, 2: 4.30 / 5.08, 4: 4.25 / 4.77, 8: 4.46 / 4.78)

size_t paged_attention_ws_bytes(int T, int nq, int d, int n_splits) {
    return QS_ATT_CNT_SLOTS * sizeof(int) + (size_t)T * nq * n_splits * (d + 2) * sizeof(float);
}

static int ilog2_exact(int v) {
    if (v <= 0 || (v & (v - 1))) return -1;
    int l = 0;
    while ((1 << l) < v) l++;
    return l;
}


static AttnForm attn_no_launch(int rc) { AttnForm f{}; f.rc = rc; return f; }   // (family 0 = ATTN_NO_LAUNCH)

// The launch plan of one call, from its arguments alone (no HIP call): the refusal or the kernel family, its template
// choices, split count, grid and LDS bytes.  One rule for both cache types.  Every dev knob of the family is read here.
static AttnForm attn_form(const AttnArgs& a) {
    AttnForm f{};
    if (a.n_seqs == 0) return attn_no_launch(0);
    if (a.nq % a.nkv) return attn_no_launch(-1);
    if (a.d != 128) {   // other head sizes (TinyLlama's 64): no matrix cores; context splits + a merge (here or in the head transform)
        if (a.d > 256 || a.d % 2) return attn_no_launch(-1);
        const int max_ctx_bytes = 64 * 1024;   // scores of one row in LDS: contexts up to 16 K keys
        f.grid = dim3(a.n_seqs * a.max_q_len, a.nq);
        if (a.d % 8 == 0 && a.d >= 8) {         // vector loads
            if (a.n_splits < 1 || a.n_splits > QS_ATT_MAXSPLIT) return attn_no_launch(-3);
            const int S = paged_attention_generic_splits(a.n_splits);
            if (!a.out && !a.ws) return attn_no_launch(-1);
            const bool partials = !a.out || S > 1;
            // LDS: the scores of one split (the block table bounds a context: max_blocks * block_size keys) + the [RG][d] fp32
            // partial rows of the P.V pass (<= 8 KiB) -- sized to the launch, so that several workgroups share a CU (with the
            // 96 KB of a 16 K-key context every launch ran one workgroup per CU: the verify pass's 512 in two rounds)
            const size_t per = (((size_t)a.max_blocks * a.block_size + S - 1) / S + 15) & ~(size_t)15;
            if (per * 4 > (size_t)max_ctx_bytes) return attn_no_launch(-2);
            f.family = ATTN_GENERIC_VEC; f.S = S; f.partials = partials; f.merge = a.out && partials;
            f.grid.z = S; f.lds = ((per * 4 + 15) & ~(size_t)15) + 8192 + 16;
            return f;
        }
        if (!a.out) return attn_no_launch(-1);
        if (a.fp8) return attn_no_launch(-6);   // the scalar kernel (odd head sizes, no model uses it) has no fp8 form
        f.family = ATTN_GENERIC; f.S = 1; f.lds = max_ctx_bytes;
        return f;
    }
    if (a.n_splits < 1 || a.n_splits > QS_ATT_MAXSPLIT) return attn_no_launch(-3);
    f.S = a.n_splits;
    f.bs_log2 = ilog2_exact(a.block_size), f.group_log2 = ilog2_exact(a.nq / a.nkv);
    if (f.bs_log2 < 0 || f.group_log2 < 0) return attn_no_launch(-5);  // block size and GQA group must be powers of two
    const int rows = a.max_q_len << f.group_log2;
    static const int fa_env = QS_DEV_KNOB("QSPEC_ATTN_PREFILL", 1);
    if (fa_env && a.n_splits == 1 && rows >= 2 * QS_FA_ROWS) {   // prompt-sized queries
        f.family = ATTN_PREFILL; f.partials = true; f.n_rb = (rows + QS_FA_ROWS - 1) / QS_FA_ROWS;
        f.grid = dim3(a.n_seqs, a.nkv * f.n_rb);
        f.lds = (size_t)QS_FA_KEYS * 256 + (size_t)QS_FA_KEYS * QS_ATT_VSTRIDE * 2 + (size_t)4 * 2 * 16 * 72 * 2;
        return f;
    }
    // a prompt-sized suffix behind a cached context (prefix hit, chunked prefill): the same 64-row workgroups over grid.z
    // context splits of whole 64-key chunks; partials in the chunk kernel's layout, merged by a second launch (out != NULL) or by
    // the head transform.  No ticket counters: the -4 refusal below does not apply.
    if (fa_env && a.n_splits > 1 && rows >= 2 * QS_FA_ROWS) {
        f.family = ATTN_PREFILL_SPLIT; f.partials = true; f.merge = a.out != nullptr;
        f.n_rb = (rows + QS_FA_ROWS - 1) / QS_FA_ROWS;
        f.grid = dim3(a.n_seqs, a.nkv * f.n_rb, a.n_splits);
        f.lds = (size_t)QS_FA_KEYS * 256 + (size_t)QS_FA_KEYS * QS_ATT_VSTRIDE * 2 + (size_t)4 * 2 * 16 * 72 * 2;
        return f;
    }
    f.n_rb = (rows + QS_ATT_MAXR - 1) / QS_ATT_MAXR;
    if (a.out && (size_t)a.n_seqs * a.nkv * f.n_rb > QS_ATT_CNT_SLOTS) return attn_no_launch(-4);   // ticket counters: in-kernel merge only
    f.partials = true; f.merge = a.out != nullptr;
    f.bt = a.max_blocks <= 128;   // the block-table row fits two registers per lane
    f.grid = dim3(a.n_seqs, a.nkv * f.n_rb, a.n_splits);
    // Partials only, and a split may be longer than one 128-key chunk (large batch: one split; long contexts): the keys
    // go over the waves of a workgroup instead of through barrier-separated chunk phases (bs=32: 21.1 -> 20.3 us, 4 K
    // context: 20.8 -> 19.1 us per launch; equal at 64 keys per split).  QSPEC_ATTN_WAVES=0/1 forces either kernel.
    static const int aw_env = QS_DEV_KNOB("QSPEC_ATTN_WAVES", -1);
    const bool long_splits = ((int64_t)a.max_blocks << f.bs_log2) > (int64_t)QS_ATT_CHUNK * a.n_splits;
    if (!a.out && (aw_env >= 0 ? aw_env != 0 : long_splits)) {
        // QSPEC_ATTN_NW=8 (dev knob): eight waves, two per SIMD -- measured SLOWER (config 3: 21.6 against 19.1 us back to
        // back): the kernel is not short of bytes in flight
        static const int nw_env = QS_DEV_KNOB("QSPEC_ATTN_NW", 0);
        static const int fast_env = QS_DEV_KNOB("QSPEC_ATTN_FAST", 1);
        f.family = ATTN_WAVES;
        f.nw = nw_env == 8 ? 8 : 4;
        f.fast = f.bt && f.bs_log2 >= 4 && fast_env;   // two uniform table entries per 32-key slice
        const size_t wave_lds = QS_AW_KEYS * QS_ATT_VSTRIDE * 2 + 2 * 16 * 40 * 2;
        f.lds = std::max((size_t)f.nw * wave_lds, (size_t)f.nw * 16 * (128 + 2) * 4);
        return f;
    }
    // more workgroups than CUs: occupancy (two per CU) instead of the in-workgroup prefetch
    static const int pf_env = QS_DEV_KNOB("QSPEC_ATTN_PF", -1);
    f.family = ATTN_CHUNK;
    f.pf = pf_env >= 0 ? pf_env != 0 : (size_t)a.n_seqs * a.nkv * f.n_rb * a.n_splits <= 256;
    f.lds = QS_ATT_MAXR * QS_ATT_CHUNK * 4 + 2 * QS_ATT_MAXR * QS_ATT_CHUNK * 2 + QS_ATT_CHUNK * QS_ATT_VSTRIDE * 2 +
            (2 * QS_ATT_MAXR + QS_ATT_MAXR * QS_ATT_MAXSPLIT + 4) * 4;
    return f;
}

int paged_attention(const f16* q, int64_t q_stride, const void* key_cache, const void* value_cache,
                    const int32_t* block_tables, int max_blocks, const int32_t* ctx_lens, const int32_t* q_start,
                    int n_seqs, int max_q_len, int nq, int nkv, int d, int block_size, float sm_scale, int n_splits,
                    float* ws, f16* out, hipStream_t st, KvQuant kq) {
    // fp8: k_scale folds into the softmax scale (an fp32 product), v_scale is applied where a row's output is stored
    const AttnArgs a{q, q_stride, key_cache, value_cache, block_tables, max_blocks, ctx_lens, q_start, n_seqs, max_q_len,
                     nq, nkv, d, block_size, kq.fp8 ? sm_scale * kq.k_scale : sm_scale, n_splits, ws, out,
                     kq.fp8 ? kq.v_scale : 1.0f, kq.fp8 != 0, st};
    const AttnForm f = attn_form(a);
    switch (f.family) {
        case ATTN_NO_LAUNCH: return f.rc;
        case ATTN_PREFILL: case ATTN_PREFILL_SPLIT: return attn_launch_prefill(a, f);
        case ATTN_WAVES: return attn_launch_waves(a, f);
        case ATTN_CHUNK: return attn_launch_chunk(a, f);
        default: return attn_launch_generic(a, f);
    }
}

// The family of the plan a call with these arguments gets (0: refused or nothing to launch): attn_form() itself, which makes
// no HIP call, so this works without a device.
int paged_attention_family(int n_seqs, int max_q_len, int nq, int nkv, int d, int block_size, int max_blocks, int n_splits,
                           bool merged) {
    if (nq <= 0 || nkv <= 0) return ATTN_NO_LAUNCH;
    static float ws_tag;   // attn_form() only asks whether ws / out are given
    static f16 out_tag;
    AttnArgs a{};
    a.max_blocks = max_blocks; a.n_seqs = n_seqs; a.max_q_len = max_q_len; a.nq = nq; a.nkv = nkv; a.d = d;
    a.block_size = block_size; a.n_splits = n_splits; a.ws = &ws_tag; a.out = merged ? &out_tag : nullptr;
    return attn_form(a).family;
}

}  // namespace qspec
