// The A2C learner's kernels (gfx950): the n-step returns scan, the loss
// gradient of the two tanh MLPs of policy_kernels.h with the rollout records
// as its row source, the statistics, RMSProp.  ppo2_reduce_kernel sums the
// partials for both learners (ppo2_launch_reduce).
//
// a2c_grad_kernel -- grid (G, 2) x 256 threads, G = min(tiles, limit): the
// tile machinery of ppo_grad_tile.h (forward, backward, dW on
// v_mfma_f32_32x32x2_f32, the float64 first layer and mean, partials on chip)
// with A2C's two heads:
//   pi   adv = ret - old_value in float32 per row, row weight w = adv / N;
//        the row's statistic adv * neglogp (float64, kept as a float32 pair)
//   vf   dZ[row][0] = 2 vf_coef (v - ret) / N; statistic (v - ret)^2
// and records in place as the row source: row i of the batch is (t, r) =
// (i / R, i % R), and its actions / old value sit in record t of the strided
// policy records (base + t * stride), so a K-step rollout needs no copy.  obs
// ([K][R][D]) and the returns ([K][R]) are contiguous; a flat batch is the
// case R = m.  idx gathers as in PPO2 (clamped: never out of bounds).
//
// No floating-point atomics: the same inputs with the same G give the same
// bits, and the flat and the in-place form of the same rows agree bit for bit
// (only addresses differ).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "policy_engine.h"
#include "ppo_grad_tile.h"
#include "ppo_grad_wide_tile.h"

namespace ce {

// -------------------------------------------------------------------- returns
// One thread per row, a reverse scan over K.  rewards / dones are read in
// place in the rollout records (base + t * stride bytes).  Unfused multiplies
// and adds in returns_numpy's order, so a float32 returns_numpy gives the same
// bits.
__global__ __launch_bounds__(256) void a2c_returns_kernel(
    int k, int rows, const char *rewards, long long reward_stride, const unsigned char *dones,
    long long done_stride, const float *last_values, float gamma, float *ret) {
#pragma clang fp contract(off)
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    float carry = last_values[r];
    for (int t = k - 1; t >= 0; --t) {
        const float rew = reinterpret_cast<const float *>(rewards + t * reward_stride)[r];
        const float nt = 1.0f - (dones[t * done_stride + r] != 0 ? 1.0f : 0.0f);
        carry = rew + gamma * carry * nt;
        ret[static_cast<long long>(t) * rows + r] = carry;
    }
}

// ------------------------------------------------------------------- gradient
struct A2cGradArgs {
    PolicyPlan p;                    // shape, image offsets and img of the policy
    int n, m;                        // rows of the call; rows idx gathers from (K R in place)
    int n_total;                     // N of the mean (n unless ranks exchange gradients)
    int tiles, grid;                 // 32-row tiles; workgroups per network
    int img_floats;                  // floats of one partial
    int w_floats, act_floats;        // LDS floats: weight stage, one activation buffer
    float vf_coef;
    int rec_rows;                    // R: rows per record (m for a flat batch)
    long long action_stride, value_stride;   // floats from one record to the next
    const int32_t *idx;              // [n] or null
    const float *obs;                // [m][D]
    const float *actions;            // record t: [R][A] at actions + t * action_stride
    const float *ret;                // [m]
    const float *old_values;         // record t: [R] at old_values + t * value_stride
    float *slab;                     // [grid][img_floats]
    double *stat_slab;               // [grid][2][kPpoRowStats]

    // the row source: records in place
    __device__ __forceinline__ const float *action_row(int s, int A) const {
        const int t = s / rec_rows, r = s - t * rec_rows;
        return actions + t * action_stride + static_cast<long long>(r) * A;
    }
    __device__ __forceinline__ float old_value(int s) const {
        const int t = s / rec_rows, r = s - t * rec_rows;
        return old_values[t * value_stride + r];
    }
    // the value head: SB 2.x's mse, no 0.5
    __device__ __forceinline__ float vf_row(int s, float v, float inv_n, float *stat) const {
        const float e = v - ret[s];
        stat[0] = e * e;
        return 2.0f * vf_coef * e * inv_n;
    }
    // the policy head: adv is a constant of the rollout, so d loss / d neglogp
    // = adv / N.  adv * neglogp as a float32 pair (the terms of pg cancel).
    __device__ __forceinline__ float pi_row(int s, double nlp, float inv_n, float *stat) const {
        const float av = ret[s] - old_value(s);
        const double term = av * nlp;
        const float hi = static_cast<float>(term);
        stat[0] = hi;
        stat[kPpoTile] = static_cast<float>(term - hi);
        return av * inv_n;
    }
};

__global__ __launch_bounds__(kPpoBlock) void a2c_grad_kernel(const A2cGradArgs g) {
    ppo_grad_tiles(g);
}

// the same heads on the chunked body of ppo_grad_wide_tile.h (ce_a2c_create_wide)
__global__ __launch_bounds__(kPpoBlock) void a2c_grad_wide_kernel(const A2cGradArgs g) {
    ppo_grad_wide_tiles(g);
}

// The four statistics and |grad|^2 from the partials, one workgroup:
// stats = loss, pg_loss, vf_loss, entropy, 0, 0, |grad|^2, 0.
__global__ __launch_bounds__(256) void a2c_finish_kernel(const Ppo2FinishArgs f) {
    __shared__ double red[256];
    __shared__ double sums[2 * kPpoRowStats];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int i = tid; i < f.n_sq; i += 256) s += f.sq[i];
    const double gn2 = ppo_block_sum(s, red);
    if (tid < 2 * kPpoRowStats) {
        double t = 0.0;
        for (int gi = 0; gi < f.grid; ++gi) t += f.stat_slab[static_cast<long long>(gi) * f.stat_stride + tid];
        sums[tid] = t;
    }
    __syncthreads();
    if (tid == 0) {
        double ent = 0.0;
        for (int c = 0; c < f.A; ++c) ent += f.img[f.off_logstd + c] + 0.5 * kPpoLog2PiE;
        const double pg = (sums[0] + sums[1]) / f.n;      // the float32 pair of pi_row
        const double vf = sums[kPpoRowStats] / f.n;
        f.stats[0] = static_cast<float>(pg - f.ent_coef * ent + f.vf_coef * vf);
        f.stats[1] = static_cast<float>(pg);
        f.stats[2] = static_cast<float>(vf);
        f.stats[3] = static_cast<float>(ent);
        f.stats[4] = 0.0f;
        f.stats[5] = 0.0f;
        f.stats[6] = static_cast<float>(gn2);
        f.stats[7] = 0.0f;
    }
}

// -------------------------------------------------------------------- RMSProp
// TF's RMSPropOptimizer over the flat vector (epsilon inside the root); the
// clip scale from the |grad|^2 the finish kernel wrote (no host read in
// between).
__global__ __launch_bounds__(256) void a2c_rmsprop_kernel(
    int n, const float *grad, const float *stats, float max_grad_norm, float lr, float alpha,
    float oma, float eps, float momentum, float *params, float *ms, float *mom) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float scale = 1.0f;
    if (max_grad_norm > 0.0f) {
        scale = max_grad_norm / (sqrtf(stats[6]) + 1e-6f);
        scale = scale < 1.0f ? scale : 1.0f;
    }
    const float gi = grad[i] * scale;
    const float si = alpha * ms[i] + oma * gi * gi;
    const float mi = momentum * mom[i] + lr * gi / sqrtf(si + eps);
    ms[i] = si;
    mom[i] = mi;
    params[i] -= mi;
}

}  // namespace ce
