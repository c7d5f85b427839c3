// The project's counter-based generator (gfx950): Philox4x32-10 (Salmon et
// al., Random123) and the four N(0,1) values of one block.
// custom_envs_amd/rng.py states both in NumPy (philox_numpy, normal_numpy).
//
//   key      (seed & 0xffffffff, seed >> 32)
//   counter  (row, t, block, purpose): the global row, the draw index (one per
//            env step or per epoch), the group of four values inside the row,
//            and a tag (kRngPolicy, kRngPermutation, kRngPredict,
//            kRngActionNoise, kRngReplay)
//   uniform  u(x) = ((x >> 8) + 0.5) * 2^-24, strictly inside (0, 1)
//   normals  r = sqrt(-2 ln u(x0)), z0 = r cospi(2 u(x1)), z1 = r sinpi(2 u(x1));
//            the same from (x2, x3) gives z2, z3.  |z| <= 5.89.
//
// With n = x >> 8, (n + 0.5) * 2^-24 takes 25 bits once n >= 2^23, so float32
// cannot hold u in the upper half of (0, 1).  Both uses below therefore start
// from the distance to the far end, (2^24 - n) - 0.5, which is exact there:
//   ln u       = log1pf(-v),  v = ((2^24 - n) - 0.5) * 2^-24 = 1 - u
//   cospi(2 u) = cospi(2 u - 2),  2 u - 2 = -((2^24 - n) - 0.5) * 2^-23
// so every argument of logf / log1pf / sincospif is the exact real number the
// statement names, and the float32 result is within a few ulp of the float64
// one at every x (near u = 1 a rounded u would cost up to 2.4e-4 in z).
//
// Device functions only, so every kernel header may include it; the kernels
// of the ce_rng_* entries are in rng_kernels.h (policy_engine.hip's unit).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ce {

constexpr uint32_t kRngPolicy = 0, kRngPermutation = 1, kRngPredict = 2;
constexpr uint32_t kRngActionNoise = 3, kRngReplay = 4;     // DDPG: action noise, replay indices

struct RngWords {
    uint32_t x0, x1, x2, x3;
};

__device__ __forceinline__ RngWords philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2,
                                                  uint32_t c3, uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
        const uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return RngWords{c0, c1, c2, c3};
}

// two normals from one word pair (see the header comment)
__device__ __forceinline__ void rng_box_muller(uint32_t xa, uint32_t xb, float *za, float *zb) {
#pragma clang fp contract(off)
    const uint32_t na = xa >> 8, nb = xb >> 8;
    float ln_u;
    if (na < (1u << 23)) {
        ln_u = logf((static_cast<float>(na) + 0.5f) * 5.9604644775390625e-08f);
    } else {
        const float v = (static_cast<float>((1u << 24) - na) - 0.5f) * 5.9604644775390625e-08f;
        ln_u = log1pf(-v);
    }
    const float r = sqrtf(-2.0f * ln_u);
    const float angle = nb < (1u << 23)
                            ? (static_cast<float>(nb) + 0.5f) * 1.1920928955078125e-07f
                            : -((static_cast<float>((1u << 24) - nb) - 0.5f) * 1.1920928955078125e-07f);
    float s, c;
    sincospif(angle, &s, &c);
    *za = r * c;
    *zb = r * s;
}

// the four N(0,1) values of block `block` of global row `row` at draw `t`
__device__ __forceinline__ float4 rng_normal4(uint32_t seed_lo, uint32_t seed_hi, uint32_t row,
                                              uint32_t t, uint32_t block, uint32_t purpose) {
    const RngWords w = philox4x32_10(row, t, block, purpose, seed_lo, seed_hi);
    float4 z;
    rng_box_muller(w.x0, w.x1, &z.x, &z.y);
    rng_box_muller(w.x2, w.x3, &z.z, &z.w);
    return z;
}

}  // namespace ce
