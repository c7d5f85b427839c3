// The PPO2 learner's kernels (gfx950): GAE, the loss gradient of the two tanh
// MLPs of policy_kernels.h, the deterministic reduce, Adam.
//
// ppo2_grad_kernel -- grid (G, 2) x 256 threads, G = min(tiles, limit): the
// tile machinery of ppo_grad_tile.h (forward, backward, dW on
// v_mfma_f32_32x32x2_f32, partials on chip; its header comment has the walk,
// the accuracy notes and the LDS budget) with PPO2's two heads:
//   pi   one thread per row forms ratio, the clip branch and the row weight w
//   vf   dZ[row][0] from the two value-clip branches
// and flat [m]-row arrays as the row source.
//
// No floating-point atomics: the same inputs with the same G give the same
// bits.  Different G regroup the float32 per-workgroup sums.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "policy_engine.h"
#include "ppo_grad_tile.h"
#include "ppo_grad_wide_tile.h"

namespace ce {

// ------------------------------------------------------------------------ GAE
// One thread per row, a reverse scan over K.  rewards / dones / values are
// read in place in the rollout records (base + t * stride bytes).  Unfused
// multiplies and adds in gae_numpy's order, so a float32 gae_numpy gives the
// same bits.
__global__ __launch_bounds__(256) void ppo2_gae_kernel(
    int k, int rows, const char *rewards, long long reward_stride, const unsigned char *dones,
    long long done_stride, const char *values, long long value_stride, const float *last_values,
    float gamma, float gamma_lam, float *adv, float *ret) {
#pragma clang fp contract(off)
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    float carry = 0.0f, v_next = last_values[r];
    for (int t = k - 1; t >= 0; --t) {
        const float rew = reinterpret_cast<const float *>(rewards + t * reward_stride)[r];
        const float v = reinterpret_cast<const float *>(values + t * value_stride)[r];
        const float nt = 1.0f - (dones[t * done_stride + r] != 0 ? 1.0f : 0.0f);
        const float delta = rew + gamma * v_next * nt - v;
        carry = delta + gamma_lam * nt * carry;
        adv[static_cast<long long>(t) * rows + r] = carry;
        ret[static_cast<long long>(t) * rows + r] = carry + v;
        v_next = v;
    }
}

// -------------------------------------------------- advantage normalisation
// The minibatch mean and 1 / (std + 1e-8) of the gathered advantages, summed
// in float64 in a fixed order by one workgroup; {0, 1} when off.
__global__ __launch_bounds__(kPpoStatBlock) void ppo2_advstat_kernel(
    int n, int m, const int32_t *idx, const float *adv, int normalize, float *out) {
    __shared__ double red[kPpoStatBlock];
    if (!normalize) {
        if (threadIdx.x == 0) {
            out[0] = 0.0f;
            out[1] = 1.0f;
        }
        return;
    }
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += kPpoStatBlock) s += adv[ppo_src_row(idx, i, m)];
    const double mean = ppo_block_sum(s, red) / n;
    s = 0.0;
    for (int i = threadIdx.x; i < n; i += kPpoStatBlock) {
        const double d = adv[ppo_src_row(idx, i, m)] - mean;
        s += d * d;
    }
    const double var = ppo_block_sum(s, red) / n;
    if (threadIdx.x == 0) {
        out[0] = static_cast<float>(mean);
        out[1] = static_cast<float>(1.0 / (sqrt(var) + 1e-8));
    }
}

// Under a gradient exchange the normalisation is over every rank's rows.
// ppo2_advmoments_kernel: ppo2_advstat_kernel's two passes over this rank's
// gathered advantages, left as the triple (n_r, mean_r, M2_r = sum (a -
// mean_r)^2) in float64.  ppo2_advmerge_kernel: the `world` triples merged in
// rank order by Chan's formula (merge_moments_numpy states it), one thread,
// into {mean, 1 / (sqrt(M2 / N) + 1e-8)}.  At world 1 no merge step runs and
// the two floats are ppo2_advstat_kernel's.
__global__ __launch_bounds__(kPpoStatBlock) void ppo2_advmoments_kernel(
    int n, int m, const int32_t *idx, const float *adv, double *out3) {
    __shared__ double red[kPpoStatBlock];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += kPpoStatBlock) s += adv[ppo_src_row(idx, i, m)];
    const double mean = ppo_block_sum(s, red) / n;
    s = 0.0;
    for (int i = threadIdx.x; i < n; i += kPpoStatBlock) {
        const double d = adv[ppo_src_row(idx, i, m)] - mean;
        s += d * d;
    }
    const double m2 = ppo_block_sum(s, red);
    if (threadIdx.x == 0) {
        out3[0] = n;
        out3[1] = mean;
        out3[2] = m2;
    }
}

__global__ __launch_bounds__(64) void ppo2_advmerge_kernel(int world, const double *moments,
                                                           float *out) {
#pragma clang fp contract(off)
    if (threadIdx.x != 0) return;
    double cnt = moments[0], mean = moments[1], m2 = moments[2];
    for (int r = 1; r < world; ++r) {
        const double nr = moments[3 * r], delta = moments[3 * r + 1] - mean;
        const double tot = cnt + nr;
        mean = mean + delta * nr / tot;
        m2 = m2 + moments[3 * r + 2] + delta * delta * cnt * nr / tot;
        cnt = tot;
    }
    out[0] = static_cast<float>(mean);
    out[1] = static_cast<float>(1.0 / (sqrt(m2 / cnt) + 1e-8));
}

// ------------------------------------------------------------------ gradient
struct Ppo2GradArgs {
    PolicyPlan p;                    // shape, image offsets and img of the policy
    int n, m;                        // rows of the call; rows of the arrays idx gathers from
    int n_total;                     // N of the mean (n unless ranks exchange gradients)
    int tiles, grid;                 // 32-row tiles; workgroups per network
    int img_floats;                  // floats of one partial
    int w_floats, act_floats;        // LDS floats: weight stage, one activation buffer
    float cliprange, cliprange_vf, vf_coef;
    const int32_t *idx;              // [n] or null
    const float *obs, *actions;      // [m][D], [m][A]
    const float *adv, *ret, *old_neglogp, *old_values;   // [m]
    const float *advstat;            // {mean, 1 / (std + 1e-8)}
    float *slab;                     // [grid][img_floats]
    double *stat_slab;               // [grid][2][kPpoRowStats]

    // the row source: flat arrays
    __device__ __forceinline__ const float *action_row(int s, int A) const {
        return actions + static_cast<long long>(s) * A;
    }
    // the value head: the two value-clip branches
    __device__ __forceinline__ float vf_row(int s, float v, float inv_n, float *stat) const {
        const float rt = ret[s];
        const float e1 = v - rt;
        float dv = e1, vf = e1 * e1;
        if (cliprange_vf >= 0.0f) {
            const float ov = old_values[s], d = v - ov, cv = cliprange_vf;
            const float e2 = ov + (d < -cv ? -cv : (d > cv ? cv : d)) - rt;
            if (e2 * e2 > e1 * e1) {
                vf = e2 * e2;
                dv = fabsf(d) < cv ? e2 : 0.0f;
            }
        }
        stat[0] = 0.5f * vf;
        return vf_coef * dv * inv_n;
    }
    // the policy head: ratio, the clip branch, the row weight
    __device__ __forceinline__ float pi_row(int s, double nlp, float inv_n, float *stat) const {
        float w = 0.0f;
        const float dnlp = static_cast<float>(old_neglogp[s] - nlp);
        const float ratio = expf(dnlp);
        const float av = (adv[s] - advstat[0]) * advstat[1];
        const float lo = 1.0f - cliprange, hi = 1.0f + cliprange;
        const float pg1 = -av * ratio;
        const float pg2 = -av * (ratio < lo ? lo : (ratio > hi ? hi : ratio));
        const bool inside = ratio > lo && ratio < hi;
        if (pg1 >= pg2 || inside) w = av * ratio * inv_n;
        stat[0] = pg1 >= pg2 ? pg1 : pg2;
        stat[kPpoTile] = 0.5f * dnlp * dnlp;
        stat[2 * kPpoTile] = fabsf(ratio - 1.0f) > cliprange ? 1.0f : 0.0f;
        return w;
    }
};

__global__ __launch_bounds__(kPpoBlock) void ppo2_grad_kernel(const Ppo2GradArgs g) {
    ppo_grad_tiles(g);
}

// the same heads on the chunked body of ppo_grad_wide_tile.h (ce_ppo2_create_wide)
__global__ __launch_bounds__(kPpoBlock) void ppo2_grad_wide_kernel(const Ppo2GradArgs g) {
    ppo_grad_wide_tiles(g);
}

// -------------------------------------------------------------------- reduce
// (Ppo2ReduceArgs and what the kernel computes: ppo_grad_tile.h)
__global__ __launch_bounds__(256) void ppo2_reduce_kernel(const Ppo2ReduceArgs q) {
    __shared__ double red[256];
    const int p = blockIdx.x * 256 + threadIdx.x;
    double sq = 0.0;
    if (p < q.p.n_params) {
        int s = 0;
        while (s + 1 < q.p.n_segs && q.p.seg_src[s + 1] <= p) ++s;
        const int i = p - q.p.seg_src[s], cols = q.p.seg_cols[s];
        const int r = i / cols, c = i - r * cols;
        const float *at = q.slab + q.p.seg_dst[s] + r * q.p.seg_cols_pad[s] + c;
        double sum = 0.0;
        for (int gi = 0; gi < q.grid; ++gi) sum += at[static_cast<long long>(gi) * q.p.img_floats];
        if (s == q.p.n_segs - 1) sum -= q.ent_coef;
        const float gf = static_cast<float>(sum);
        q.grad[p] = gf;
        sq = static_cast<double>(gf) * gf;
    }
    sq = ppo_block_sum(sq, red);
    if (threadIdx.x == 0) q.sq[blockIdx.x] = sq;
}

// ------------------------------------------------------- partial, combine
// (Ppo2PartialArgs, Ppo2CombineArgs and the record: ppo_grad_tile.h)
// The reduce kernel's grid.  Block 0 also folds the statistic sums over the G
// workgroups (the finish kernels' loop) and writes the row count.
__global__ __launch_bounds__(256) void ppo2_partial_kernel(const Ppo2PartialArgs q) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < q.p.n_params) {
        int s = 0;
        while (s + 1 < q.p.n_segs && q.p.seg_src[s + 1] <= p) ++s;
        const int i = p - q.p.seg_src[s], cols = q.p.seg_cols[s];
        const int r = i / cols, c = i - r * cols;
        const float *at = q.slab + q.p.seg_dst[s] + r * q.p.seg_cols_pad[s] + c;
        double sum = 0.0;
        for (int gi = 0; gi < q.grid; ++gi) sum += at[static_cast<long long>(gi) * q.p.img_floats];
        q.record[p] = sum;
    }
    if (blockIdx.x == 0) {
        const int tid = threadIdx.x;
        if (tid < 2 * kPpoRowStats) {
            double t = 0.0;
            for (int gi = 0; gi < q.grid; ++gi) t += q.stat_slab[gi * 2 * kPpoRowStats + tid];
            q.record[q.p.n_params + tid] = t;
        } else if (tid < ppo_record_doubles(q.p.n_params) - q.p.n_params) {
            // the row count, then zeros to the record's padded end
            q.record[q.p.n_params + tid] = tid == 2 * kPpoRowStats ? static_cast<double>(q.n) : 0.0;
        }
    }
}

__global__ __launch_bounds__(256) void ppo2_combine_kernel(const Ppo2CombineArgs q) {
    __shared__ double red[256];
    const int p = blockIdx.x * 256 + threadIdx.x;
    double sq = 0.0;
    if (p < q.n_params) {
        double sum = 0.0;
        for (int r = 0; r < q.world; ++r)
            sum += q.records[static_cast<long long>(r) * q.record_doubles + p];
        if (p >= q.off_logstd_flat) sum -= q.ent_coef;
        const float gf = static_cast<float>(sum);
        q.grad[p] = gf;
        sq = static_cast<double>(gf) * gf;
    }
    sq = ppo_block_sum(sq, red);
    if (threadIdx.x == 0) q.sq[blockIdx.x] = sq;
}

// The six statistics and |grad|^2 from the partials, one workgroup.
__global__ __launch_bounds__(256) void ppo2_finish_kernel(const Ppo2FinishArgs f) {
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
        const double pg = sums[0] / f.n, kl = sums[1] / f.n, cf = sums[2] / f.n;
        const double vf = sums[kPpoRowStats] / f.n;
        f.stats[0] = static_cast<float>(pg - f.ent_coef * ent + f.vf_coef * vf);
        f.stats[1] = static_cast<float>(pg);
        f.stats[2] = static_cast<float>(vf);
        f.stats[3] = static_cast<float>(ent);
        f.stats[4] = static_cast<float>(kl);
        f.stats[5] = static_cast<float>(cf);
        f.stats[6] = static_cast<float>(gn2);
        f.stats[7] = 0.0f;
    }
}

// ---------------------------------------------------------------------- Adam
// TF-style Adam over the flat vector; the clip scale from the |grad|^2 the
// finish kernel wrote (no host read in between).
__global__ __launch_bounds__(256) void ppo2_adam_kernel(
    int n, const float *grad, const float *stats, float max_grad_norm, float lr_t, float beta1,
    float beta2, float omb1, float omb2, float eps, float *params, float *m, float *v) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float scale = 1.0f;
    if (max_grad_norm > 0.0f) {
        scale = max_grad_norm / (sqrtf(stats[6]) + 1e-6f);
        scale = scale < 1.0f ? scale : 1.0f;
    }
    const float gi = grad[i] * scale;
    const float mi = beta1 * m[i] + omb1 * gi;
    const float vi = beta2 * v[i] + omb2 * gi * gi;
    m[i] = mi;
    v[i] = vi;
    params[i] -= lr_t * mi / (sqrtf(vi) + eps);
}

}  // namespace ce
