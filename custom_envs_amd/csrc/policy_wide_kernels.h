// policy_mlp_kernel (policy_kernels.h) for observations up to 1024 wide and
// heads up to 512 wide (gfx950): the policy of the reference's default
// Optimize shape, 981 -> hidden -> 490.
//
// Same semantics, launch shape and layouts as the narrow kernel: grid
// (ceil(rows / 32), 2) x 256 threads, a 32-row tile per workgroup, wave w on
// output units 32w .. 32w + 31, v_mfma_f32_32x32x2_f32 with the rows along M,
// activations k-major [width][33] in LDS, weights staged in LDS from the
// padded parameter image.  What a layer wider than the 128 x 128 stage needs:
//
//   first layer  the observation is walked in K-chunks of 128 columns.  Each
//                chunk stages its slice of the obs tile (k-major) and rows
//                k0 .. k0 + 127 of W0 (contiguous in the image), and the MFMAs
//                continue the same accumulators.
//   head         the output columns are walked in N-chunks of 128 (4 waves x
//                32).  Each chunk stages columns c0 .. c0 + 127 of the head's
//                image as [in][chunk], multiplies, then samples, clips and
//                stores its columns.
//
// A hidden layer has one chunk each way, so the loop below is the narrow
// kernel's for it.  Every output unit's dot product is one accumulator chain
// over ascending k with the narrow kernel's operands, so at a shape the narrow
// kernel takes too the outputs are the same bits.
//
// neglogp keeps the narrow partition: 8 threads per row, thread `part` over
// columns part, part + 8, ... in ascending order, the same shuffle tree, the
// same sequential logstd sum (read through LDS here: up to 512 dependent global
// loads by one thread per row would outlast the network).  The explicit instance reads the noise row from
// global memory up front; the generated instance forms the noise of one head
// chunk at a time (32 x 128 floats, not 32 x 512) and carries each thread's
// partial sum across the chunks -- a chunk starts at a multiple of 128, so a
// thread meets the same columns in the same order.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "policy_kernels.h"
#include "rng.h"

namespace ce {

constexpr int kPolWideMaxD = 1024;   // observation width
constexpr int kPolWideMaxA = 512;    // action width
constexpr int kPolChunk = 128;       // K-chunk of the first layer, N-chunk of the head
constexpr int kPolStageBatch = 8;    // float4 loads a thread issues before it stores one

// LDS: the weight stage (a.w_floats), two activation buffers (a.act_floats
// each; the first also takes the obs chunks) and, kGen, the noise of one head
// chunk [32][min(round4(A), 128)].
template <bool kGen>
__global__ __launch_bounds__(kPolBlock) void policy_wide_kernel(const PolicyArgs a) {
    extern __shared__ float pol_lds[];
    float *wbuf = pol_lds;
    float *cur = wbuf + a.w_floats;
    float *nxt = cur + a.act_floats;
    float *gen = nxt + a.act_floats;
    const int a4 = (a.A + 3) & ~3;
    const int gw = a4 < kPolChunk ? a4 : kPolChunk;      // words per row of gen
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 31, h = lane >> 5;
    const int net = blockIdx.y;
    const long long row0 = static_cast<long long>(blockIdx.x) * kPolTile;
    const int live = a.rows - row0 < kPolTile ? static_cast<int>(a.rows - row0) : kPolTile;
    const int nr = tid >> 3, part = tid & 7;             // neglogp: row and column class
    float sq = 0.0f;                                     // this thread's share of sum noise^2

    if (!kGen && net == 0 && a.noise && nr < live) {
        const float *nz = a.noise + (row0 + nr) * a.A;
        for (int c0 = part; c0 < a.A; c0 += 64) {        // eight loads together, the sum in order
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = c0 + 8 * j < a.A ? nz[c0 + 8 * j] : 0.0f;
#pragma unroll
            for (int j = 0; j < 8; ++j)
                if (c0 + 8 * j < a.A) sq += v[j] * v[j];
        }
    }

    for (int l = 0; l <= a.n_hidden; ++l) {
        const int ip = a.in_pad[l], op = a.out_pad[net][l];
        const bool head = l == a.n_hidden;
        for (int c0 = 0; c0 < op; c0 += kPolChunk) {
            const int cw = op - c0 < kPolChunk ? op - c0 : kPolChunk;
            const int n0 = wave * 32;
            pol_f32x16 acc = {};
            for (int k0 = 0; k0 < ip; k0 += kPolChunk) {
                const int kc = ip - k0 < kPolChunk ? ip - k0 : kPolChunk;
                {   // rows k0 .. k0 + kc - 1, columns c0 .. c0 + cw - 1 of the weight image
                    const float *src = a.img + a.off_w[net][l] + static_cast<long long>(k0) * op + c0;
                    // eight loads in flight per thread, then the eight stores: one
                    // load per loop trip would make the stage a chain of latencies
                    const int c4 = cw >> 2, n4 = kc * c4;
                    for (int base = tid; base < n4; base += kPolStageBatch * kPolBlock) {
                        float4 v[kPolStageBatch];
#pragma unroll
                        for (int j = 0; j < kPolStageBatch; ++j) {
                            const int i = base + j * kPolBlock;
                            const int ic = i < n4 ? i : n4 - 1;      // a live address either way
                            const int k = ic / c4, c = ic - k * c4;
                            v[j] = *reinterpret_cast<const float4 *>(src + k * op + 4 * c);
                        }
#pragma unroll
                        for (int j = 0; j < kPolStageBatch; ++j) {
                            const int i = base + j * kPolBlock;
                            if (i < n4) reinterpret_cast<float4 *>(wbuf)[i] = v[j];
                        }
                    }
                }
                if (l == 0) {   // this chunk of the observation tile, zero past D and the last row
                    // thread -> column tid % 128 of rows tid / 128 + 2 j: the 16 loads
                    // of a thread are issued together, a wave reads 64 consecutive floats
                    const float *src = a.obs + row0 * a.D + k0;
                    const int k = tid & (kPolChunk - 1), rb = tid >> 7;
                    float v[kPolTile / 2];
#pragma unroll
                    for (int j = 0; j < kPolTile / 2; ++j) {
                        const int r = rb + 2 * j;
                        v[j] = (r < live && k0 + k < a.D) ? src[static_cast<long long>(r) * a.D + k] : 0.0f;
                    }
                    if (k < kc) {
#pragma unroll
                        for (int j = 0; j < kPolTile / 2; ++j) cur[k * kPolLd + rb + 2 * j] = v[j];
                    }
                }
                if (kGen && head && net == 0) {   // this chunk of the noise tile (one K-chunk here)
                    const int nb = (a4 - c0 < kPolChunk ? a4 - c0 : kPolChunk) >> 2;
                    for (int i = tid; i < live * nb; i += kPolBlock) {
                        const int r = i / nb, b = i - r * nb;
                        *reinterpret_cast<float4 *>(gen + r * gw + 4 * b) =
                            rng_normal4(a.seed_lo, a.seed_hi, a.row0 + static_cast<uint32_t>(row0 + r),
                                        a.t, static_cast<uint32_t>((c0 >> 2) + b), kRngPolicy);
                    }
                }
                __syncthreads();
                if (n0 < cw) {   // wave-uniform
                    const float *xa = cur + h * kPolLd + li;
                    const float *wb = wbuf + h * cw + n0 + li;
                    for (int k = 0; k < kc; k += 2)
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[k * kPolLd], wb[k * cw], acc, 0, 0, 0);
                }
                if (k0 + kc < ip) __syncthreads();       // the stage and the obs chunk are free
            }
            if (kGen && head && net == 0 && nr < live) {
                const int nc = a.A - c0 < kPolChunk ? a.A - c0 : kPolChunk;
                const float *nz = gen + nr * gw;
                for (int c = part; c < nc; c += 8) sq += nz[c] * nz[c];
            }
            if (n0 < cw) {
                const int lc = n0 + li, col = c0 + lc;
                const float bias = a.img[a.off_b[net][l] + col];
                if (!head) {
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        nxt[col * kPolLd + pol_acc_row(r, h)] = tanhf(acc[r] + bias);
                } else if (net == 0) {
                    if (col < a.A) {
                        const float sd = expf(a.img[a.off_logstd + col]);
                        const float lo = a.img[a.off_low + col], hi = a.img[a.off_high + col];
                        float nz[16] = {};               // the explicit noise, loaded together
                        if (!kGen && a.noise) {
#pragma unroll
                            for (int r = 0; r < 16; ++r) {
                                const int row = pol_acc_row(r, h);
                                nz[r] = row < live ? a.noise[(row0 + row) * a.A + col] : 0.0f;
                            }
                        }
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int row = pol_acc_row(r, h);
                            if (row < live) {
                                const long long o = (row0 + row) * a.A + col;
                                float act = acc[r] + bias;
                                if (kGen) act += sd * gen[row * gw + lc];
                                else if (a.noise) act += sd * nz[r];
                                a.action[o] = act;
                                a.env_action[o] = act < lo ? lo : (act > hi ? hi : act);
                            }
                        }
                    }
                } else if (col == 0) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = pol_acc_row(r, h);
                        if (row < live) a.value[row0 + row] = acc[r] + bias;
                    }
                }
            }
            __syncthreads();
        }
        float *t = cur;
        cur = nxt;
        nxt = t;
    }

    if (net == 0) {   // uniform over the workgroup
        sq += __shfl_xor(sq, 1);
        sq += __shfl_xor(sq, 2);
        sq += __shfl_xor(sq, 4);
        // logstd through LDS (both activation buffers are free after the last
        // barrier; A <= 512 <= act_floats): 490 dependent global loads by one
        // thread per row would be most of the launch.  The sum stays sequential.
        float *lsd = cur;
        for (int c = tid; c < a.A; c += kPolBlock) lsd[c] = a.img[a.off_logstd + c];
        __syncthreads();
        if (part == 0 && nr < live) {
            float ls = 0.0f;
            for (int c = 0; c < a.A; ++c) ls += lsd[c];
            a.neglogp[row0 + nr] = 0.5f * sq + ls + 0.5f * a.A * 1.8378770664093453f;
        }
    }
}

}  // namespace ce
