// KV-cache block moves (include/qspec_hip.h, "KV block operations"): what the reference does in front of every step with
// copy_blocks / swap_blocks (csrc/cache_kernels.cu; vllm/worker/worker.py, execute_worker).  A block is an opaque run of
// block_bytes bytes (a multiple of 16) inside each of the 2 * num_layers cache tensors (K and V of every layer: the "planes"),
// so the fp16 and the e4m3 cache share these kernels.  Three forms of ONE kernel, each ONE launch for all layers:
//
//   copy     plane[dst] = plane[src] for every (src, dst) pair                  (copy-on-write, fork)
//   gather   staging[i][plane] = plane[ids[i]]: a block's K and V of every layer become one contiguous record (swap out)
//   scatter  the reverse                                                          (swap in)
//
// Pure copies, bound by HBM bandwidth alone: every lane moves 16 bytes per access (1 KiB per wave instruction), BM_UNROLL loads
// are in flight per lane before the first store, a work unit is BM_CHUNK consecutive vectors (16 KiB) of one plane of one
// block, units are numbered chunk-fastest so that neighbouring workgroups stream neighbouring lines, and a capped grid strides
// over them.  Plain vector stores, no atomics, no workspace, no LDS.  The copy form relies on what the host has checked: no dst
// is a src of the same call and the dsts are distinct (include/qspec_hip.h), so no unit reads what another writes.
#include "common.cuh"
#include "kernels.h"

namespace qspec {
namespace {

constexpr int BM_THREADS = 256;
constexpr int BM_UNROLL = 4;                        // 16-byte loads in flight per lane
constexpr int BM_CHUNK = BM_THREADS * BM_UNROLL;    // vectors per work unit
constexpr int BM_MAX_GRID = 256 * 16;               // 256 CUs x 8 resident workgroups x 2

enum { BM_COPY = 0, BM_GATHER = 1, BM_SCATTER = 2 };

// The cache base pointers are read from memory, so the compiler cannot know their address space and would address them as
// flat; they are device memory by contract: global_load / global_store_dwordx4.
typedef __attribute__((address_space(1))) u32x4 gvec;
__device__ __forceinline__ gvec* as_global(char* p) { return (gvec*)p; }

template <int MODE>
__global__ __launch_bounds__(BM_THREADS) void block_move_kernel(char* const* __restrict__ planes, int n_planes,
                                                                const int64_t* __restrict__ ids, int64_t n_units, int vecs,
                                                                int chunks, char* __restrict__ staging) {
    const int64_t block_bytes = (int64_t)vecs * 16;
    for (int64_t u = blockIdx.x; u < n_units; u += gridDim.x) {
        const int chunk = (int)(u % chunks);
        const int64_t rest = u / chunks;
        const int plane = (int)(rest % n_planes);
        const int64_t item = rest / n_planes;
        char* base = planes[plane];
        const gvec* src;
        gvec* dst;
        if (MODE == BM_COPY) {
            src = as_global(base + ids[2 * item] * block_bytes);
            dst = as_global(base + ids[2 * item + 1] * block_bytes);
        } else {
            char* in_cache = base + ids[item] * block_bytes;
            char* in_stage = staging + (item * n_planes + plane) * block_bytes;
            src = as_global(MODE == BM_GATHER ? in_cache : in_stage);
            dst = as_global(MODE == BM_GATHER ? in_stage : in_cache);
        }
        const int v0 = chunk * BM_CHUNK + threadIdx.x;
        u32x4 r[BM_UNROLL];
#pragma unroll
        for (int i = 0; i < BM_UNROLL; ++i) {
            const int v = v0 + i * BM_THREADS;
            if (v < vecs) r[i] = src[v];
        }
#pragma unroll
        for (int i = 0; i < BM_UNROLL; ++i) {
            const int v = v0 + i * BM_THREADS;
            if (v < vecs) dst[v] = r[i];
        }
    }
}

template <int MODE>
int block_move(void* const* planes, int num_layers, const int64_t* ids, int n, int64_t block_bytes, void* staging, hipStream_t st) {
    if (num_layers < 1 || n < 0 || block_bytes < 16 || block_bytes % 16 || block_bytes / 16 > 0x7fffffff) return -1;
    if (n == 0) return 0;
    const int vecs = (int)(block_bytes / 16);
    const int chunks = (vecs + BM_CHUNK - 1) / BM_CHUNK;
    const int n_planes = 2 * num_layers;
    const int64_t n_units = (int64_t)n * n_planes * chunks;
    const int grid = (int)(n_units < BM_MAX_GRID ? n_units : BM_MAX_GRID);
    hipLaunchKernelGGL(block_move_kernel<MODE>, dim3(grid), dim3(BM_THREADS), 0, st, reinterpret_cast<char* const*>(planes),
                       n_planes, ids, n_units, vecs, chunks, reinterpret_cast<char*>(staging));
    return 0;
}

}  // namespace

int copy_blocks(void* const* layer_ptrs, int num_layers, const int64_t* pairs, int num_pairs, int64_t block_bytes, hipStream_t st) {
    return block_move<BM_COPY>(layer_ptrs, num_layers, pairs, num_pairs, block_bytes, nullptr, st);
}

int gather_blocks(void* const* layer_ptrs, int num_layers, const int64_t* block_ids, int n, int64_t block_bytes, void* staging,
                  hipStream_t st) {
    return block_move<BM_GATHER>(layer_ptrs, num_layers, block_ids, n, block_bytes, staging, st);
}

int scatter_blocks(void* const* layer_ptrs, int num_layers, const int64_t* block_ids, int n, int64_t block_bytes,
                   const void* staging, hipStream_t st) {
    return block_move<BM_SCATTER>(layer_ptrs, num_layers, block_ids, n, block_bytes, const_cast<void*>(staging), st);
}

}  // namespace qspec
