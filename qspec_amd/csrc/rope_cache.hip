// RoPE and the paged KV-cache write.
//
// Replaces (reference, relative to /root/reference):
//   rotary_embedding_kernel              csrc/pos_encoding_kernels.cu:10-35,71-92  (call: quarot_llama.py:207-211)
//   reshape_and_cache_flash_kernel       csrc/cache_kernels.cu:207-247             (call: flash_attn.py:711-720)
//
// KV cache layout is vLLM's flash layout: [num_blocks, block_size, n_kv, d] fp16,
// one tensor for K and one for V, shared by the draft and the verify pass.
#include <stdlib.h>

#include "common.cuh"
#include "kernels.h"

namespace qspec {

// NeoX rotation with every operator rounded to fp16, as c10::Half arithmetic does.
__device__ __forceinline__ void rope_pair(f16& x, f16& y, f16 c, f16 s) {
    float xf = h2f(x), yf = h2f(y), cf = h2f(c), sf = h2f(s);
    f16 nx = f2h(h2f(f2h(xf * cf)) - h2f(f2h(yf * sf)));
    f16 ny = f2h(h2f(f2h(yf * cf)) + h2f(f2h(xf * sf)));
    x = nx;
    y = ny;
}

__global__ __launch_bounds__(256) void rotary_embedding_kernel(const int64_t* __restrict__ positions,
                                                               f16* __restrict__ q, f16* __restrict__ k,
                                                               const f16* __restrict__ cos_sin_cache, int nq, int nkv,
                                                               int d, int rot_dim, int64_t q_stride,
                                                               int64_t k_stride) {
    const int t = blockIdx.x;
    const int embed = rot_dim / 2;
    const f16* cs = cos_sin_cache + positions[t] * rot_dim;
    for (int i = threadIdx.x; i < (nq + nkv) * embed; i += blockDim.x) {
        int h = i / embed, o = i % embed;
        f16* base = h < nq ? q + t * q_stride + (size_t)h * d : k + t * k_stride + (size_t)(h - nq) * d;
        rope_pair(base[o], base[embed + o], cs[o], cs[embed + o]);
    }
}

int rotary_embedding(const int64_t* positions, f16* q, f16* k, const f16* cos_sin_cache, int T, int nq, int nkv, int d,
                     int rot_dim, int64_t q_stride, int64_t k_stride, hipStream_t st) {
    if (T == 0) return 0;
    if (rot_dim > d || rot_dim % 2) return -1;
    hipLaunchKernelGGL(rotary_embedding_kernel, dim3(T), dim3(256), 0, st, positions, q, k, cos_sin_cache, nq, nkv, d,
                       rot_dim, q_stride, k_stride);
    return 0;
}

// KVT = f16: the cache element is the fp16 value.  KVT = uint8_t: the e4m3 byte of f(value) * inv (common.cuh: f2e4m3),
// at the same element position -- reshape_and_cache_flash(..., "fp8", k_scale, v_scale), inv = 1 / scale.
template <typename KVT>
__device__ __forceinline__ KVT kv_elem(f16 v, float inv) {
    if constexpr (sizeof(KVT) == 1) return f2e4m3(h2f(v) * inv);
    else return v;
}
// eight consecutive elements: one 16-byte (fp16) or one 8-byte (e4m3) store
template <typename KVT>
__device__ __forceinline__ void kv_store8(KVT* dst, f16x8 v, float inv) {
    if constexpr (sizeof(KVT) == 1) {
        u32x2 w;
        w[0] = f2e4m3_x4(h2f(v[0]) * inv, h2f(v[1]) * inv, h2f(v[2]) * inv, h2f(v[3]) * inv);
        w[1] = f2e4m3_x4(h2f(v[4]) * inv, h2f(v[5]) * inv, h2f(v[6]) * inv, h2f(v[7]) * inv);
        *reinterpret_cast<u32x2*>(dst) = w;
    } else {
        *reinterpret_cast<f16x8*>(dst) = v;
    }
}

template <typename KVT>
__global__ __launch_bounds__(256) void reshape_and_cache_flash_kernel(const f16* __restrict__ key,
                                                                      const f16* __restrict__ value,
                                                                      KVT* __restrict__ key_cache,
                                                                      KVT* __restrict__ value_cache,
                                                                      const int64_t* __restrict__ slot_mapping, int n,
                                                                      int64_t k_stride, int64_t v_stride, float k_inv,
                                                                      float v_inv) {
    const int t = blockIdx.x;
    const int64_t slot = slot_mapping[t];
    if (slot < 0) return;  // padded token
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        key_cache[slot * n + i] = kv_elem<KVT>(key[t * k_stride + i], k_inv);
        value_cache[slot * n + i] = kv_elem<KVT>(value[t * v_stride + i], v_inv);
    }
}

int reshape_and_cache_flash(const f16* key, const f16* value, void* key_cache, void* value_cache,
                            const int64_t* slot_mapping, int T, int nkv, int d, int64_t k_stride, int64_t v_stride,
                            hipStream_t st, KvQuant kq) {
    if (T == 0) return 0;
    if (kq.fp8)
        hipLaunchKernelGGL(reshape_and_cache_flash_kernel<uint8_t>, dim3(T), dim3(256), 0, st, key, value,
                           (uint8_t*)key_cache, (uint8_t*)value_cache, slot_mapping, nkv * d, k_stride, v_stride, kq.k_inv,
                           kq.v_inv);
    else
        hipLaunchKernelGGL(reshape_and_cache_flash_kernel<f16>, dim3(T), dim3(256), 0, st, key, value, (f16*)key_cache,
                           (f16*)value_cache, slot_mapping, nkv * d, k_stride, v_stride, 1.0f, 1.0f);
    return 0;
}

// Fused: in-place RoPE on the q and k slices of the fused qkv row, then scatter k,v into the paged cache.
// qkv [T, (nq + 2 nkv) * d]; one workgroup per token, 8 fp16 (16 B) per lane trip.
template <typename KVT>
__global__ __launch_bounds__(256) void rope_kv_write_kernel(const int64_t* __restrict__ positions,
                                                            f16* __restrict__ qkv,
                                                            const f16* __restrict__ cos_sin_cache,
                                                            KVT* __restrict__ key_cache, KVT* __restrict__ value_cache,
                                                            const int64_t* __restrict__ slot_mapping, int nq, int nkv,
                                                            int d, int rot_dim, float k_inv, float v_inv) {
    const int t = blockIdx.x;
    const int embed = rot_dim / 2;
    const int row = (nq + 2 * nkv) * d;
    f16* base = qkv + (size_t)t * row;
    const f16* cs = cos_sin_cache + positions[t] * rot_dim;
    const int64_t slot = slot_mapping[t];
    const int vec_per_head = embed / 8;  // 16-byte chunks of the x half
    for (int i = threadIdx.x; i < (nq + nkv) * vec_per_head; i += blockDim.x) {
        int h = i / vec_per_head, o = (i % vec_per_head) * 8;
        f16* hp = base + (size_t)h * d;
        f16x8 x = *reinterpret_cast<f16x8*>(hp + o), y = *reinterpret_cast<f16x8*>(hp + embed + o);
        f16x8 c = *reinterpret_cast<const f16x8*>(cs + o), s = *reinterpret_cast<const f16x8*>(cs + embed + o);
#pragma unroll
        for (int e = 0; e < 8; e++) {
            f16 xe = x[e], ye = y[e];
            rope_pair(xe, ye, c[e], s[e]);
            x[e] = xe;
            y[e] = ye;
        }
        *reinterpret_cast<f16x8*>(hp + o) = x;
        *reinterpret_cast<f16x8*>(hp + embed + o) = y;
        if (h >= nq && slot >= 0) {
            KVT* kc = key_cache + (slot * nkv + (h - nq)) * d;
            kv_store8<KVT>(kc + o, x, k_inv);
            kv_store8<KVT>(kc + embed + o, y, k_inv);
        }
    }
    if (slot >= 0) {
        const f16* vsrc = base + (size_t)(nq + nkv) * d;
        KVT* vc = value_cache + slot * nkv * d;
        for (int i = threadIdx.x; i < nkv * d / 8; i += blockDim.x)
            kv_store8<KVT>(vc + 8 * i, *reinterpret_cast<const f16x8*>(vsrc + 8 * i), v_inv);
        if (rot_dim < d) {  // un-rotated tail of k
            for (int i = threadIdx.x; i < nkv * (d - rot_dim); i += blockDim.x) {
                int h = i / (d - rot_dim), o = rot_dim + i % (d - rot_dim);
                key_cache[(slot * nkv + h) * d + o] = kv_elem<KVT>(base[(size_t)(nq + h) * d + o], k_inv);
            }
        }
    }
}

int rope_kv_write(const int64_t* positions, f16* qkv, const f16* cos_sin_cache, void* key_cache, void* value_cache,
                  const int64_t* slot_mapping, int T, int nq, int nkv, int d, int rot_dim, hipStream_t st, KvQuant kq) {
    if (T == 0) return 0;
    if (rot_dim > d || rot_dim % 16 || d % 8) return -1;
    if (kq.fp8)
        hipLaunchKernelGGL(rope_kv_write_kernel<uint8_t>, dim3(T), dim3(256), 0, st, positions, qkv, cos_sin_cache,
                           (uint8_t*)key_cache, (uint8_t*)value_cache, slot_mapping, nq, nkv, d, rot_dim, kq.k_inv, kq.v_inv);
    else
        hipLaunchKernelGGL(rope_kv_write_kernel<f16>, dim3(T), dim3(256), 0, st, positions, qkv, cos_sin_cache,
                           (f16*)key_cache, (f16*)value_cache, slot_mapping, nq, nkv, d, rot_dim, 1.0f, 1.0f);
    return 0;
}

}  // namespace qspec
