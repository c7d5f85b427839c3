// The kernels of the ce_rng_* entries (gfx950), over rng.h's device functions.
// Included by one translation unit (policy_engine.hip); another unit that
// needs one of these launches goes through a host function of that unit
// (policy_engine.h: rng_enqueue_replay).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "rng.h"

namespace ce {

// out[s][r][a] (record s at out + s * stride floats) for draws t0 + s, rows
// row0 + r under `purpose`; thread i of the launch owns one (s, r, block)
__device__ __forceinline__ void rng_normal_block(float *out, long long i, int rows, int A,
                                                 long long stride, uint32_t seed_lo,
                                                 uint32_t seed_hi, uint32_t t0, uint32_t row0,
                                                 uint32_t purpose) {
    const int nb = (A + 3) >> 2;
    const int b = static_cast<int>(i % nb);
    const long long sr = i / nb;
    const int r = static_cast<int>(sr % rows);
    const long long s = sr / rows;
    const float4 z = rng_normal4(seed_lo, seed_hi, row0 + static_cast<uint32_t>(r),
                                 t0 + static_cast<uint32_t>(s), static_cast<uint32_t>(b), purpose);
    float *dst = out + s * stride + static_cast<long long>(r) * A + 4 * b;
    const float v[4] = {z.x, z.y, z.z, z.w};
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (4 * b + j < A) dst[j] = v[j];
}

// ce_rng_normal: the policy noise; one thread per (s, r, block)
__global__ __launch_bounds__(256) void rng_normal_kernel(float *out, long long total, int rows,
                                                         int A, long long stride, uint32_t seed_lo,
                                                         uint32_t seed_hi, uint32_t t0,
                                                         uint32_t row0) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= total) return;
    rng_normal_block(out, i, rows, A, stride, seed_lo, seed_hi, t0, row0, kRngPolicy);
}

// ce_rng_normal_purpose: the same block under the caller's purpose
__global__ __launch_bounds__(256) void rng_normal_purpose_kernel(
    float *out, long long total, int rows, int A, long long stride, uint32_t seed_lo,
    uint32_t seed_hi, uint32_t t0, uint32_t row0, uint32_t purpose) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= total) return;
    rng_normal_block(out, i, rows, A, stride, seed_lo, seed_hi, t0, row0, purpose);
}

// ce_rng_u32: value i is word i % 4 of the block (0, t, i / 4, purpose)
__global__ __launch_bounds__(256) void rng_u32_kernel(uint32_t *out, long long n, uint32_t seed_lo,
                                                      uint32_t seed_hi, uint32_t purpose,
                                                      uint32_t t) {
    const long long b = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (4 * b >= n) return;
    const RngWords w = philox4x32_10(0u, t, static_cast<uint32_t>(b), purpose, seed_lo, seed_hi);
    const uint32_t v[4] = {w.x0, w.x1, w.x2, w.x3};
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (4 * b + j < n) out[4 * b + j] = v[j];
}

// ce_rng_replay / ce_ddpg_train: out[s][i], s < steps, i < n, = (word * size)
// >> 32 of word i % 4 of the block (0, t0 + s, i / 4, kRngReplay): an index in
// [0, size).  One thread per (s, block); nb = ceil(n / 4) blocks per draw.
__global__ __launch_bounds__(256) void rng_replay_kernel(int32_t *out, long long total, int nb,
                                                         int n, uint32_t size, uint32_t seed_lo,
                                                         uint32_t seed_hi, uint32_t t0) {
    const long long i = static_cast<long long>(blockIdx.x) * 256 + threadIdx.x;
    if (i >= total) return;
    const int b = static_cast<int>(i % nb);
    const long long s = i / nb;
    const RngWords w = philox4x32_10(0u, t0 + static_cast<uint32_t>(s), static_cast<uint32_t>(b),
                                     kRngReplay, seed_lo, seed_hi);
    const uint32_t v[4] = {w.x0, w.x1, w.x2, w.x3};
    int32_t *dst = out + s * n + 4 * b;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (4 * b + j < n) dst[j] = static_cast<int32_t>(__umulhi(v[j], size));
}

}  // namespace ce
