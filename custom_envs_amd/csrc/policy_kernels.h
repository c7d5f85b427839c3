// The actor-critic MLP policy of a PPO2 / A2C agent as ONE launch (gfx950).
//
// stable-baselines' MlpPolicy (net_arch=[dict(pi=[...], vf=[...])], tanh): two
// separate tanh networks of the same hidden widths over the observation row,
// a linear mean head (A values) on the first and a linear value head (1) on
// the second, a state-independent logstd[A], and a diagonal Gaussian sample
//   action     = mean + exp(logstd) * noise          (noise supplied, or null; or
//                                                    formed here: kGen below)
//   env_action = min(max(action, low), high)
//   neglogp    = 0.5 sum noise^2 + sum logstd + 0.5 A log(2 pi)
// (neglogp from the noise itself, not from (action - mean) / std).
//
// Launch shape: grid (ceil(rows / 32), 2) x 256 threads.  blockIdx.y picks the
// network, so one launch covers both and 4096 rows give 256 workgroups (one
// per CU), each running half the dependent layer chain.  A workgroup owns a
// 32-row tile; wave w owns output units 32w .. 32w + 31 of the layer.
//
// Arithmetic: float32 on v_mfma_f32_32x32x2_f32 with the rows along M:
//   Z (32 rows x 32 units) += X (32 rows x 2) . W (2 x 32 units)
// Activations live in LDS k-major ([width][33]: the A operand of lane l is
// X^T[k][l & 31], consecutive words; the store of a result column strides 33
// words, conflict free).  The layer's weights are staged in LDS one layer at
// a time from the policy's parameter image (policy_engine.hip: every matrix
// zero-padded to [round4(in)][round32(out)], 16-byte aligned, so the stage is
// float4 copies by all 256 threads and the B operand W[k][n0 + (l & 31)] is
// one conflict-free row read).  Bias, tanh, sample, clip and log-prob run on
// the vector units.  Rows past `rows` are loaded as zeros and never stored.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "rng.h"

namespace ce {

constexpr int kPolBlock = 256;       // 4 waves: up to 128 output units per layer
constexpr int kPolTile = 32;         // rows per workgroup (the MFMA's M)
constexpr int kPolLd = 33;           // LDS words per activation column
constexpr int kPolMaxHidden = 3;     // hidden layers
constexpr int kPolMaxWidth = 128;    // hidden width (multiple of 32)
constexpr int kPolMaxD = 128;        // observation width
constexpr int kPolMaxA = 64;         // action width
constexpr int kPolLayers = kPolMaxHidden + 1;   // hidden layers + the head

typedef float pol_f32x16 __attribute__((ext_vector_type(16)));

struct PolicyArgs {
    int rows, D, A, n_hidden;
    int in_pad[kPolLayers];          // per layer (the head last): rows of its W image
    int out_pad[2][kPolLayers];      // columns of its W image, per network
    int off_w[2][kPolLayers];        // float offsets into img (multiples of 4)
    int off_b[2][kPolLayers];
    int off_logstd, off_low, off_high;
    int w_floats;                    // LDS floats of the weight stage
    int act_floats;                  // LDS floats of one activation buffer
    const float *img;
    const float *obs;                // [rows][D]
    const float *noise;              // [rows][A] or null (the explicit instance)
    uint32_t seed_lo, seed_hi, t, row0;   // the generated instance: rng.h's key, draw, first row
    float *action, *env_action;      // [rows][A]
    float *neglogp, *value;          // [rows]
};

__device__ __forceinline__ int pol_acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// kGen false: the noise is a.noise (or null).  kGen true: the pi workgroup
// (blockIdx.y == 0) forms its tile's noise once from rng.h -- every thread
// whole Philox blocks of a row -- into an LDS block of 32 x round4(A) floats
// behind the activation buffers, and both consumers read it there.
template <bool kGen>
__global__ __launch_bounds__(kPolBlock) void policy_mlp_kernel(const PolicyArgs a) {
    extern __shared__ float pol_lds[];
    float *wbuf = pol_lds;
    float *cur = wbuf + a.w_floats;
    float *nxt = cur + a.act_floats;
    float *gen = nxt + a.act_floats;         // kGen: [32][round4(A)]
    const int a4 = (a.A + 3) & ~3;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 31, h = lane >> 5;
    const int net = blockIdx.y;
    const long long row0 = static_cast<long long>(blockIdx.x) * kPolTile;
    const int live = a.rows - row0 < kPolTile ? static_cast<int>(a.rows - row0) : kPolTile;

    // the observation tile, k-major, zero past D and past the last row
    {
        const int dp = a.in_pad[0];
        const float *src = a.obs + row0 * a.D;
        for (int i = tid; i < kPolTile * dp; i += kPolBlock) {
            const int r = i / dp, k = i - r * dp;
            cur[k * kPolLd + r] = (r < live && k < a.D) ? src[r * a.D + k] : 0.0f;
        }
    }

    // neglogp needs no network: 8 threads per row over the noise row
    if (net == 0) {
        if (kGen) {
            const int nb = a4 >> 2;
            for (int i = tid; i < live * nb; i += kPolBlock) {
                const int r = i / nb, b = i - r * nb;
                reinterpret_cast<float4 *>(gen)[i] =
                    rng_normal4(a.seed_lo, a.seed_hi, a.row0 + static_cast<uint32_t>(row0 + r), a.t,
                                static_cast<uint32_t>(b), kRngPolicy);
            }
            __syncthreads();                 // net is uniform over the workgroup
        }
        const int r = tid >> 3, part = tid & 7;
        float s = 0.0f;
        if (kGen) {
            if (r < live) {
                const float *nz = gen + r * a4;
                for (int c = part; c < a.A; c += 8) s += nz[c] * nz[c];
            }
        } else if (a.noise && r < live) {
            const float *nz = a.noise + (row0 + r) * a.A;
            for (int c = part; c < a.A; c += 8) s += nz[c] * nz[c];
        }
        s += __shfl_xor(s, 1);
        s += __shfl_xor(s, 2);
        s += __shfl_xor(s, 4);
        if (part == 0 && r < live) {
            float ls = 0.0f;
            for (int c = 0; c < a.A; ++c) ls += a.img[a.off_logstd + c];
            a.neglogp[row0 + r] = 0.5f * s + ls + 0.5f * a.A * 1.8378770664093453f;
        }
    }

    for (int l = 0; l <= a.n_hidden; ++l) {
        const int ip = a.in_pad[l], op = a.out_pad[net][l];
        {   // stage this layer's weight image
            const float4 *src = reinterpret_cast<const float4 *>(a.img + a.off_w[net][l]);
            float4 *dst = reinterpret_cast<float4 *>(wbuf);
            const int n4 = ip * op / 4;
            for (int i = tid; i < n4; i += kPolBlock) dst[i] = src[i];
        }
        __syncthreads();
        const int n0 = wave * 32;
        if (n0 < op) {   // wave-uniform
            pol_f32x16 acc = {};
            const float *xa = cur + h * kPolLd + li;
            const float *wb = wbuf + h * op + n0 + li;
            for (int k = 0; k < ip; k += 2)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[k * kPolLd], wb[k * op], acc, 0, 0, 0);
            const int col = n0 + li;
            const float bias = a.img[a.off_b[net][l] + col];
            if (l < a.n_hidden) {
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    nxt[col * kPolLd + pol_acc_row(r, h)] = tanhf(acc[r] + bias);
            } else if (net == 0) {
                if (col < a.A) {
                    const float sd = expf(a.img[a.off_logstd + col]);
                    const float lo = a.img[a.off_low + col], hi = a.img[a.off_high + col];
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = pol_acc_row(r, h);
                        if (row < live) {
                            const long long o = (row0 + row) * a.A + col;
                            float act = acc[r] + bias;
                            if (kGen) act += sd * gen[row * a4 + col];
                            else if (a.noise) act += sd * a.noise[o];
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
        float *t = cur;
        cur = nxt;
        nxt = t;
    }
}

// The parameter image from the caller's flat vector: segment s is a
// [rows][cols] row-major block of `flat` at src, written zero-padded as
// [rows_pad][cols_pad] at dst.
constexpr int kPolSegs = 4 * kPolLayers + 1;   // (W, b) per layer per network + logstd

struct PolicyPack {
    int n;
    int dst[kPolSegs], src[kPolSegs], rows[kPolSegs], cols[kPolSegs];
    int rows_pad[kPolSegs], cols_pad[kPolSegs];
};

__global__ __launch_bounds__(256) void policy_pack_kernel(const PolicyPack p, const float *flat,
                                                          float *img) {
    const int s = blockIdx.x;
    if (s >= p.n) return;
    const int cp = p.cols_pad[s], total = p.rows_pad[s] * cp;
    for (int i = threadIdx.x; i < total; i += 256) {
        const int r = i / cp, c = i - r * cp;
        img[p.dst[s] + i] = (r < p.rows[s] && c < p.cols[s]) ? flat[p.src[s] + r * p.cols[s] + c] : 0.0f;
    }
}

}  // namespace ce
