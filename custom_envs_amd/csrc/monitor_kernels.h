// The episode monitor's kernels (gfx950, wave64, 256-thread blocks): what
// utils_logging.VecMonitor.step does K times on the host, over the rollout
// records where collect left them.
//
//   monitor_scan_kernel       one thread per env, forward over t: the carry
//                             (ep_reward float64, ep_len, episode, total_steps)
//                             in VecMonitor.step's order of operations; a done
//                             stages (r, l, current_reward, episode) at [t][env]
//   monitor_count_kernel      finished episodes per 256 flags of the flattened
//                             [K E] done flags
//   monitor_blockscan_kernel  one workgroup: the exclusive scan of the block
//                             counts and the total
//   monitor_write_kernel      recomputes its block-local prefix (ballot +
//                             popcount per wave, wave totals through LDS) and
//                             writes one record per finished episode, in (t,
//                             env) order, the info columns gathered at [t][env];
//                             nothing at or past `capacity`
//   monitor_reset_kernel      VecMonitor.reset of the masked envs
//   monitor_ev_kernel         explained variance, two passes in float64 in a
//                             fixed order by one workgroup
//
// Records are read in place as base + t * stride bytes (as ppo2_gae_kernel
// reads its records); an env's reward and done are those of row env *
// row_stride.  No floating-point atomics: the same inputs give the same bits.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ce {

constexpr int kMonBlock = 256;
constexpr int kMonWaves = kMonBlock / 64;
constexpr int kMonMaxInfo = 16;          // CE_MONITOR_MAX_INFO
constexpr int kMonRecordHead = 32;       // bytes before a record's info columns

// element (t, env) of a column: ((float *)(base + t * stride))[env * row_floats + col]
struct MonitorColumn {
    const char *base;
    long long stride;
    int row_floats, col;
};

struct MonitorRecords {
    int k, envs, row_stride, n_info;
    const char *reward;
    long long reward_stride;
    const unsigned char *done;
    long long done_stride;
    MonitorColumn info[kMonMaxInfo];
};

struct MonitorCarry {
    double *ep_reward;
    int *ep_len;
    long long *episode, *total_steps;
};

// [K E] each, written only where done is set
struct MonitorStage {
    double *r;
    int *l;
    float *cur;
    long long *episode;
};

__device__ __forceinline__ bool mon_done(const MonitorRecords &q, int i) {
    const int t = i / q.envs, e = i - t * q.envs;
    return q.done[t * q.done_stride + static_cast<long long>(e) * q.row_stride] != 0;
}

__global__ __launch_bounds__(kMonBlock) void monitor_scan_kernel(const MonitorRecords q,
                                                                 const MonitorCarry c,
                                                                 const MonitorStage s) {
    const int e = blockIdx.x * kMonBlock + threadIdx.x;
    if (e >= q.envs) return;
    double r = c.ep_reward[e];
    int l = c.ep_len[e];
    long long ep = c.episode[e];
    const long long row = static_cast<long long>(e) * q.row_stride;
    for (int t = 0; t < q.k; ++t) {
        const float rew = reinterpret_cast<const float *>(q.reward + t * q.reward_stride)[row];
        r += static_cast<double>(rew);
        l += 1;
        if (q.done[t * q.done_stride + row] != 0) {
            const long long i = static_cast<long long>(t) * q.envs + e;
            s.r[i] = r;
            s.l[i] = l;
            s.cur[i] = rew;
            s.episode[i] = ep;
            r = 0.0;
            l = 0;
            ep += 1;
        }
    }
    c.ep_reward[e] = r;
    c.ep_len[e] = l;
    c.episode[e] = ep;
    c.total_steps[e] += q.k;
}

// The flagged threads before this one in its block, and the block's count.
__device__ __forceinline__ int mon_block_prefix(bool flag, int *wave_tot, int *block_total) {
    const unsigned long long b = __ballot(flag);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int before = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) wave_tot[w] = __popcll(b);
    __syncthreads();
    int off = 0, total = 0;
    for (int j = 0; j < kMonWaves; ++j) {
        if (j < w) off += wave_tot[j];
        total += wave_tot[j];
    }
    *block_total = total;
    return off + before;
}

__global__ __launch_bounds__(kMonBlock) void monitor_count_kernel(const MonitorRecords q,
                                                                  int *block_count) {
    __shared__ int wave_tot[kMonWaves];
    const int n = q.k * q.envs;
    const int i = blockIdx.x * kMonBlock + threadIdx.x;
    int total;
    mon_block_prefix(i < n && mon_done(q, i), wave_tot, &total);
    if (threadIdx.x == 0) block_count[blockIdx.x] = total;
}

// block_off[b] = sum of block_count[0 .. b), total[0] = sum of all; `extra`
// (or null) gets the total too.
__global__ __launch_bounds__(kMonBlock) void monitor_blockscan_kernel(int nb, const int *block_count,
                                                                      int *block_off,
                                                                      long long *total,
                                                                      long long *extra) {
    __shared__ long long part[kMonBlock];
    const int tid = threadIdx.x;
    const int chunk = (nb + kMonBlock - 1) / kMonBlock;
    const int lo = tid * chunk < nb ? tid * chunk : nb;
    const int hi = lo + chunk < nb ? lo + chunk : nb;
    long long s = 0;
    for (int b = lo; b < hi; ++b) s += block_count[b];
    part[tid] = s;
    __syncthreads();
    long long base = 0;
    for (int j = 0; j < tid; ++j) base += part[j];
    for (int b = lo; b < hi; ++b) {
        block_off[b] = static_cast<int>(base);
        base += block_count[b];
    }
    if (tid == kMonBlock - 1) {       // base is now the sum of every part
        total[0] = base;
        if (extra) extra[0] = base;
    }
}

// One record: {int32 env, int32 t, float64 r, int32 l, float32 current_reward,
// int64 episode, float32 info[n_info]}, record_bytes = 32 + 4 * n_info rounded
// up to 8 (the pad float is written as zero).
__global__ __launch_bounds__(kMonBlock) void monitor_write_kernel(const MonitorRecords q,
                                                                  const MonitorStage s,
                                                                  const int *block_off, char *out,
                                                                  long long capacity,
                                                                  int record_bytes) {
    __shared__ int wave_tot[kMonWaves];
    const int n = q.k * q.envs;
    const int i = blockIdx.x * kMonBlock + threadIdx.x;
    const bool flag = i < n && mon_done(q, i);
    int total;
    const long long pos = block_off[blockIdx.x] + mon_block_prefix(flag, wave_tot, &total);
    if (!flag || pos >= capacity) return;
    const int t = i / q.envs, e = i - t * q.envs;
    char *rec = out + pos * record_bytes;
    reinterpret_cast<int *>(rec)[0] = e;
    reinterpret_cast<int *>(rec)[1] = t;
    *reinterpret_cast<double *>(rec + 8) = s.r[i];
    *reinterpret_cast<int *>(rec + 16) = s.l[i];
    *reinterpret_cast<float *>(rec + 20) = s.cur[i];
    *reinterpret_cast<long long *>(rec + 24) = s.episode[i];
    float *info = reinterpret_cast<float *>(rec + kMonRecordHead);
    for (int c = 0; c < q.n_info; ++c) {
        const MonitorColumn &col = q.info[c];
        info[c] = reinterpret_cast<const float *>(col.base + t * col.stride)[
            static_cast<long long>(e) * col.row_floats + col.col];
    }
    if (q.n_info & 1) info[q.n_info] = 0.0f;
}

// VecMonitor.reset of the envs whose mask byte is set (null: all): the running
// sums cleared, the episode number advanced.
__global__ __launch_bounds__(kMonBlock) void monitor_reset_kernel(int envs,
                                                                  const unsigned char *mask,
                                                                  const MonitorCarry c) {
    const int e = blockIdx.x * kMonBlock + threadIdx.x;
    if (e >= envs || (mask && !mask[e])) return;
    c.ep_reward[e] = 0.0;
    c.ep_len[e] = 0;
    c.episode[e] += 1;
}

// The block's sum in a fixed order, on every thread.
__device__ __forceinline__ double mon_block_sum(double v, double *red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int w = kMonBlock / 2; w > 0; w >>= 1) {
        if (static_cast<int>(threadIdx.x) < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    return red[0];
}

// 1 - Var[ret - val] / Var[ret] over the k * rows values (read strided in the
// policy records) and the learner's flat returns; NaN when Var[ret] == 0
// (stable-baselines' explained_variance).  Var is the population variance.
__global__ __launch_bounds__(kMonBlock) void monitor_ev_kernel(int k, int rows, const char *values,
                                                               long long value_stride,
                                                               const float *ret, double *out) {
#pragma clang fp contract(off)
    __shared__ double red[kMonBlock];
    const int n = k * rows;
    double sr = 0.0, sd = 0.0;
    for (int i = threadIdx.x; i < n; i += kMonBlock) {
        const int t = i / rows, r = i - t * rows;
        const double y = ret[i];
        const double v = reinterpret_cast<const float *>(values + t * value_stride)[r];
        sr += y;
        sd += y - v;
    }
    const double mr = mon_block_sum(sr, red) / n;
    const double md = mon_block_sum(sd, red) / n;
    sr = 0.0;
    sd = 0.0;
    for (int i = threadIdx.x; i < n; i += kMonBlock) {
        const int t = i / rows, r = i - t * rows;
        const double y = ret[i];
        const double v = reinterpret_cast<const float *>(values + t * value_stride)[r];
        const double a = y - mr, b = (y - v) - md;
        sr += a * a;
        sd += b * b;
    }
    const double vr = mon_block_sum(sr, red) / n;
    const double vd = mon_block_sum(sd, red) / n;
    if (threadIdx.x == 0) out[0] = vr == 0.0 ? __builtin_nan("") : 1.0 - vd / vr;
}

}  // namespace ce
