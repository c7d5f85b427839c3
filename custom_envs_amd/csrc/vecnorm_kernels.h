// stable-baselines' VecNormalize on the device: one launch does one step of
// the statement in custom_envs_amd/vectorize/vecnormalize.py
// (vecnormalize_numpy): the running float64 moments of the observation columns
// and of the discounted returns are merged with this step's batch, then the
// observations and rewards are scaled, clipped and stored as float32.
//
// Grid: workgroups 0 .. ceil(D / 4) - 1 each own 4 observation columns for
// all rows; the last workgroup owns `ret`, the return moments and the rewards.
// In an observation workgroup thread t works on column t % 4 of the rows
// t / 4, t / 4 + 256, ...: four neighbouring lanes read the 16 contiguous bytes
// the workgroup owns of a row, so a wave's load touches 16 rows' cache lines,
// not 64 (one thread per row with four 4-byte loads each measured 22 us at
// 4096 x 41: the wave's cache-line requests, not the arithmetic).
// Every sum is float64 in a fixed order: per thread in row order, a shuffle
// tree over the lanes of the same column inside each wave, then the 16 waves'
// partials in wave order.  No floating-point atomic: the same inputs give the
// same bits.  A column's moments are written by its own workgroup only; the
// count is kept per column so no workgroup reads what another writes.
//
// The launch is a dozen workgroups, so its time is a chain of latencies, not
// bandwidth: the loops issue the global loads of four rows per thread before
// the first use (kVnBatch), and what a later pass needs again sits in LDS.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ce {

constexpr int kVnBlock = 1024;
constexpr int kVnWaves = kVnBlock / 64;
constexpr int kVnCols = 4;                 // observation columns per workgroup
constexpr int kVnRowLanes = kVnBlock / kVnCols;
constexpr int kVnBatch = 4;                // rows a thread loads before it uses one
// a workgroup's rows x 4 floats (the return workgroup's rows doubles) are
// staged in LDS up to this many rows (128 KB of the CU's 160 KB); past it
// the later passes read global memory again (the rows sit in L2)
constexpr int kVnStageRows = 8192;

struct VecnormArgs {
    int rows, D;
    int norm_obs, norm_reward, training, reset, staged;
    double clip_obs, clip_reward, gamma, epsilon;
    const float *obs;          // [rows][D]
    const float *reward;       // [rows]   (null with reset)
    const uint8_t *done;       // [rows]   (null with reset)
    float *obs_out;            // [rows][D]
    float *reward_out;         // [rows]   (null with reset)
    double *obs_mean, *obs_var, *obs_count;   // [D] each
    double *ret_stat;          // mean, var, count
    double *ret;               // [rows]
};

// The sum of v over the threads of the block with the same t % GROUPS (1: the
// whole block; 4: one sum per observation column), to each of them, in a
// fixed order.  Every thread of the block calls it.  `red` holds GROUPS x 16
// doubles.
template <int GROUPS>
__device__ inline double vn_group_sum(double v, double *red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane % GROUPS;
#pragma unroll
    for (int off = 32; off >= GROUPS; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane < GROUPS) red[g * kVnWaves + wave] = v;
    __syncthreads();
    double s = red[g * kVnWaves];
#pragma unroll 4
    for (int w = 1; w < kVnWaves; ++w) s += red[g * kVnWaves + w];
    __syncthreads();           // `red` is free again
    return s;
}

// update(mean, var, count, batch mean, batch var, n) of the statement
__device__ inline void vn_merge(double &mean, double &var, double &count, double bm, double bv,
                                double n) {
    const double d = bm - mean, tot = count + n;
    const double m2 = var * count + bv * n + d * d * count * n / tot;
    mean = mean + d * n / tot;
    var = m2 / tot;
    count = tot;
}

// ret * gamma + reward as a multiply and an add, each rounded (no fused
// multiply-add), so `ret` carries the bits of the NumPy statement
__device__ inline double vn_ret_next(double ret, double gamma, double reward) {
#pragma clang fp contract(off)
    const double scaled = ret * gamma;
    return scaled + reward;
}

__device__ inline float vn_clip(double v, double c) {
    return static_cast<float>(fmin(fmax(v, -c), c));
}

__device__ inline void vn_obs_columns(const VecnormArgs &a, float *stage, double *red,
                                      double *bcast) {
    const int t = threadIdx.x, rows = a.rows;
    const size_t D = static_cast<size_t>(a.D);
    const int c0 = blockIdx.x * kVnCols;
    const int nc = min(kVnCols, a.D - c0);
    const int col = t & (kVnCols - 1), rl = t / kVnCols;
    const bool live = col < nc;            // the last workgroup may own fewer columns
    const float *__restrict__ src = a.obs + c0 + col;
    float *__restrict__ dst = a.obs_out + c0 + col;
    if (!a.norm_obs) {         // the switch is off: the output is the input
        if (live)
            for (int r = rl; r < rows; r += kVnRowLanes) dst[r * D] = src[r * D];
        return;
    }
    const bool staged = a.staged != 0, training = a.training != 0;
    // pass 1: the column sums; the elements go to LDS on the way (a thread
    // reads back only what it staged itself, so no barrier is needed for them)
    double s = 0.0;
    if (live && (staged || training)) {
        for (int r0 = rl; r0 < rows; r0 += kVnBatch * kVnRowLanes) {
            float x[kVnBatch];
#pragma unroll
            for (int i = 0; i < kVnBatch; ++i) {
                const int r = r0 + i * kVnRowLanes;
                if (r < rows) x[i] = src[r * D];
            }
#pragma unroll
            for (int i = 0; i < kVnBatch; ++i) {
                const int r = r0 + i * kVnRowLanes;
                if (r < rows) {
                    if (staged) stage[r * kVnCols + col] = x[i];
                    s += double(x[i]);
                }
            }
        }
    }
    if (training) {
        const double n = double(rows);
        const double bm = vn_group_sum<kVnCols>(s, red) / n;
        // pass 2: the squared deviations from the batch mean
        double q = 0.0;
        if (live) {
#pragma unroll 4
            for (int r = rl; r < rows; r += kVnRowLanes) {
                const double d = double(staged ? stage[r * kVnCols + col] : src[r * D]) - bm;
                q += d * d;
            }
        }
        q = vn_group_sum<kVnCols>(q, red);
        if (t < nc) {          // thread t < 4 is column t's
            double mean = a.obs_mean[c0 + t], var = a.obs_var[c0 + t], count = a.obs_count[c0 + t];
            vn_merge(mean, var, count, bm, q / n, n);
            a.obs_mean[c0 + t] = mean;
            a.obs_var[c0 + t] = var;
            a.obs_count[c0 + t] = count;
            bcast[t] = mean;
            bcast[kVnCols + t] = 1.0 / sqrt(var + a.epsilon);
        }
    } else if (t < nc) {
        bcast[t] = a.obs_mean[c0 + t];
        bcast[kVnCols + t] = 1.0 / sqrt(a.obs_var[c0 + t] + a.epsilon);
    }
    __syncthreads();
    if (!live) return;
    // pass 3: normalise, clip, store
    const double mean = bcast[col], inv = bcast[kVnCols + col], c = a.clip_obs;
#pragma unroll 4
    for (int r = rl; r < rows; r += kVnRowLanes) {
        const float x = staged ? stage[r * kVnCols + col] : src[r * D];
        dst[r * D] = vn_clip((double(x) - mean) * inv, c);
    }
}

__device__ inline void vn_returns(const VecnormArgs &a, float *stage_f, double *red,
                                  double *bcast) {
    const int t = threadIdx.x, rows = a.rows;
    double *__restrict__ ret = a.ret;
    if (a.reset) {             // reset(): ret = 0, the return moments untouched
        for (int r = t; r < rows; r += kVnBlock) ret[r] = 0.0;
        return;
    }
    const float *__restrict__ reward = a.reward;
    const uint8_t *__restrict__ done = a.done;
    float *__restrict__ reward_out = a.reward_out;
    double *stage = reinterpret_cast<double *>(stage_f);
    const bool staged = a.staged != 0;
    const bool update = a.training && a.norm_reward;
    // pass 1: ret = ret * gamma + reward and its sum.  The new ret goes to
    // global memory only at the end, where the dones are known; until then a
    // thread keeps it in LDS (or, past the staging bound, in `ret` itself,
    // whose entries it reads back itself).
    double s = 0.0;
    for (int r0 = t; r0 < rows; r0 += kVnBatch * kVnBlock) {
        double old[kVnBatch];
        float rw[kVnBatch];
#pragma unroll
        for (int i = 0; i < kVnBatch; ++i) {
            const int r = r0 + i * kVnBlock;
            if (r < rows) {
                old[i] = ret[r];
                rw[i] = reward[r];
            }
        }
#pragma unroll
        for (int i = 0; i < kVnBatch; ++i) {
            const int r = r0 + i * kVnBlock;
            if (r < rows) {
                const double v = vn_ret_next(old[i], a.gamma, double(rw[i]));
                if (staged) stage[r] = v; else ret[r] = v;
                s += v;
            }
        }
    }
    if (update) {
        const double n = double(rows), bm = vn_group_sum<1>(s, red) / n;
        double q = 0.0;
#pragma unroll 4
        for (int r = t; r < rows; r += kVnBlock) {
            const double d = (staged ? stage[r] : ret[r]) - bm;
            q += d * d;
        }
        q = vn_group_sum<1>(q, red);
        if (t == 0) {
            double mean = a.ret_stat[0], var = a.ret_stat[1], count = a.ret_stat[2];
            vn_merge(mean, var, count, bm, q / n, n);
            a.ret_stat[0] = mean;
            a.ret_stat[1] = var;
            a.ret_stat[2] = count;
            bcast[0] = 1.0 / sqrt(var + a.epsilon);
        }
    } else if (t == 0) {
        bcast[0] = 1.0 / sqrt(a.ret_stat[1] + a.epsilon);
    }
    __syncthreads();
    const double inv = bcast[0], c = a.clip_reward;
    for (int r0 = t; r0 < rows; r0 += kVnBatch * kVnBlock) {
        float rw[kVnBatch];
        uint8_t dn[kVnBatch];
#pragma unroll
        for (int i = 0; i < kVnBatch; ++i) {
            const int r = r0 + i * kVnBlock;
            if (r < rows) {
                rw[i] = reward[r];
                dn[i] = done[r];
            }
        }
#pragma unroll
        for (int i = 0; i < kVnBatch; ++i) {
            const int r = r0 + i * kVnBlock;
            if (r < rows) {
                reward_out[r] = a.norm_reward ? vn_clip(double(rw[i]) * inv, c) : rw[i];   // no mean shift
                if (dn[i]) ret[r] = 0.0;
                else if (staged) ret[r] = stage[r];
            }
        }
    }
}

__global__ __launch_bounds__(kVnBlock) void vecnorm_step_kernel(VecnormArgs a) {
    // [rows][4] floats (observation workgroups) or [rows] doubles (the returns') when a.staged
    extern __shared__ __align__(16) float vn_stage[];
    __shared__ double red[kVnCols * kVnWaves];
    __shared__ double bcast[2 * kVnCols];
    const int col_blocks = (a.D + kVnCols - 1) / kVnCols;
    if (static_cast<int>(blockIdx.x) < col_blocks)
        vn_obs_columns(a, vn_stage, red, bcast);
    else
        vn_returns(a, vn_stage, red, bcast);
}

}  // namespace ce
