// The DDPG learner's tile kernels at wide shapes (gfx950): obs_dim <= 1024,
// act_dim <= 512, 1-2 hidden layers of 32 or 64 units -- the reference's
// Optimize-v0 spec is 981 -> 490.  ddpg_kernels.h states the contracts and the
// tile conventions; these kernels keep both (32-row tiles, 256 threads,
// v_mfma_f32_32x32x2_f32 with the rows along M, activations in LDS k-major
// with the 33-word column, the same Args, the same slab [G][img_floats] and
// stat_slab, rows gathered by idx, exact zeros past n, no floating-point
// atomics) and differ in how a layer meets the workgroup.  The narrow kernels
// hold whole layers and whole activation rows in LDS; here four layers are
// walked in chunks of kDdpgWideChunk = 128:
//
//   both first layers, W0 [D][h0]         in K-chunks: 128 observation columns
//       [128][33] and 128 rows of W0 [128][h0 + 1] per step, one accumulator
//       chain per wave running across the chunks in ascending k.
//   the actor's head, w_out [h][A]        in N-chunks: 128 columns [h][129]
//       per step, wave w the columns 32 w .. 32 w + 31 of the chunk.
//   the critic's concat layer, [h0 + A]   in K-chunks: the h0 hidden rows, then
//       128 action rows per step; the accumulator chain runs across them.
//   dQ / d action, out-dimension A        in N-chunks: 128 rows of the concat
//       layer's weights per step, dZ_1 W_1^T for those rows.
//
// The action never stands in LDS whole.  Where the actor feeds the critic (the
// target kernel, the gradient kernel's actor branch) the head walk and the
// concat walk are one loop: head chunk c gives 128 action columns [128][33],
// which are the concat chain's next 128 k-rows.  The critic branch loads the
// stored action chunk by chunk from global memory, for the forward and again
// for dW.  What does stand whole is S [round32(A)][33]: 1 - a^2 from
// ddpg_tanh as the head is walked, then, in place, the head's dZ = dQ / da o
// (1 - a^2) as dQ / da comes out of the accumulators chunk by chunk (the
// thread that holds dQ / da of (row, column) owns that element of S), so dQ /
// da is never stored either.
//
// Every dW block's C operand lives in the workgroup's OWN slab partial in
// global memory: per tile a wave reads its block (16 values a lane), runs the
// narrow kernel's 16 MFMAs and writes it back.  Block -> wave -> lane is a
// function of the shape alone, so a lane only ever reads what it wrote; the
// workgroup's first tile starts from zero without reading, so a partial never
// shows what an earlier call left in the slab.  The first layers' dW0 (up to
// 64 blocks), the concat layer's dW (up to 36) and the head's dW (up to 32) do
// not fit the accumulators; the hidden 64 x 64 blocks would, and take the
// same path so that there is one.  db stays in registers, the head's two
// columns a thread (tid and tid + 256).  dW0 walks the observation chunks
// again (re-read from global memory and clipped again).
//
// Operands and their order are the narrow kernels': a dot product adds its
// products in ascending k across the chunks in one chain from zero, a dW
// block's tiles are added in tile order, the db sums run over the rows in
// order, and the epilogues are the same expressions.  At a shape both take
// the wide kernels write the narrow kernels' bits (at the same G).
//
// LDS (floats), the same plan for the four kernels:
//   weight stage   128 x 65 = 8320   (a [64][129] head chunk is 8256)
//   chunk          128 x 33 = 4224   (observation or action columns)
//   hidden         4 x 64 x 33 = 8448 (actor h0, h1; critic h0, h1)
//   critic head dZ 32 x 33 = 1056
//   row scalars    128               (Q, y, one spare row, rowsrc)
//   S              round32(A) x 33   (the act kernel's N(0,1) block)
// 22 176 + 33 round32(A): 156 288 B at A = 490 and at the limit, of 163 840.
#pragma once

#include "ddpg_kernels.h"

namespace ce {

constexpr int kDdpgWideMaxD = 1024;
constexpr int kDdpgWideMaxA = 512;
constexpr int kDdpgWideChunk = 128;
constexpr int kDdpgWideGrid = 64;        // default workgroups per branch (a partial is ~0.8 MB)
constexpr int kDdpgWideHid = 64;         // the widest hidden layer
constexpr int kDdpgWideStage = kDdpgWideChunk * (kDdpgWideHid + 1);
static_assert(kDdpgWideStage >= kDdpgWideHid * (kDdpgWideChunk + 1), "a head chunk fits the stage");

__host__ __device__ constexpr int ddpg_wide_lds_floats(int act_dim) {
    return kDdpgWideStage + kDdpgWideChunk * kDdpgLd + 4 * kDdpgWideHid * kDdpgLd +
           kDdpgTile * kDdpgLd + kDdpgRowFloats + (act_dim + 31) / 32 * 32 * kDdpgLd;
}
constexpr int kDdpgWideMaxLdsBytes = ddpg_wide_lds_floats(kDdpgWideMaxA) * 4;
static_assert(ddpg_wide_lds_floats(490) * 4 == 156288, "the header comment's LDS plan at 981 -> 490");
static_assert(kDdpgWideMaxLdsBytes == 156288, "the header comment's LDS plan at the limits");
static_assert(kDdpgWideMaxLdsBytes <= 160 * 1024, "the CU's LDS");

struct DdpgWideLds {
    float *wbuf, *xc, *hb[4], *dzc, *rowf, *s;
    int *rowsrc;
};
__device__ __forceinline__ DdpgWideLds ddpg_wide_lds(float *base) {
    DdpgWideLds s;
    s.wbuf = base;
    s.xc = s.wbuf + kDdpgWideStage;
    for (int i = 0; i < 4; ++i) s.hb[i] = s.xc + kDdpgWideChunk * kDdpgLd + i * kDdpgWideHid * kDdpgLd;
    s.dzc = s.hb[3] + kDdpgWideHid * kDdpgLd;
    s.rowf = s.dzc + kDdpgTile * kDdpgLd;
    s.rowsrc = reinterpret_cast<int *>(s.rowf + 3 * kDdpgTile);
    s.s = s.rowf + kDdpgRowFloats;
    return s;
}

// ---------------------------------------------------------------- tile pieces
// (called by all 256 threads; no piece has a barrier unless it says so)

// rows x cols of a padded image layer (row stride src_ld, cols and every
// offset a multiple of 4) into the stage as [rows][cols + 1]
__device__ __forceinline__ void ddpg_wide_stage(float *wbuf, const float *src, int rows, int cols,
                                                int src_ld) {
    const int c4 = cols >> 2, n4 = rows * c4, ld = cols + 1;
    for (int i = threadIdx.x; i < n4; i += kDdpgBlock) {
        const int r = i / c4, c = 4 * (i - r * c4);
        const float4 v = *reinterpret_cast<const float4 *>(src + static_cast<long long>(r) * src_ld + c);
        float *d = wbuf + r * ld + c;
        d[0] = v.x;
        d[1] = v.y;
        d[2] = v.z;
        d[3] = v.w;
    }
}

// columns k0 .. k0 + kn - 1 of the tile's observations, clipped, k-major,
// zero past D and past the last row
__device__ __forceinline__ void ddpg_wide_load_obs(float *xc, const float *obs, const int *rowsrc,
                                                   int D, int k0, int kn, float lo, float hi) {
    for (int i = threadIdx.x; i < kDdpgTile * kn; i += kDdpgBlock) {
        const int r = i / kn, k = i - r * kn;
        const int s = rowsrc[r];
        float v = 0.0f;
        if (s >= 0 && k0 + k < D) {
            v = obs[static_cast<long long>(s) * D + k0 + k];
            v = fminf(fmaxf(v, lo), hi);
        }
        xc[k * kDdpgLd + r] = v;
    }
}

// columns c0 .. c0 + kn - 1 of the tile's stored actions, zero past A and
// past the last row
__device__ __forceinline__ void ddpg_wide_load_act(float *xc, const float *actions,
                                                   const int *rowsrc, int A, int c0, int kn) {
    for (int i = threadIdx.x; i < kDdpgTile * kn; i += kDdpgBlock) {
        const int r = i / kn, k = i - r * kn;
        const int s = rowsrc[r];
        xc[k * kDdpgLd + r] =
            (s >= 0 && c0 + k < A) ? actions[static_cast<long long>(s) * A + c0 + k] : 0.0f;
    }
}

// ddpg_xw continued: kn more k-rows of x and of the stage on the chain `acc`
__device__ __forceinline__ ddpg_f32x16 ddpg_wide_xw(ddpg_f32x16 acc, const float *x,
                                                    const float *wbuf, int kn, int ld, int n0) {
    const int lane = threadIdx.x & 63, li = lane & 31, h = lane >> 5;
    const float *xa = x + h * kDdpgLd + li;
    const float *wb = wbuf + h * ld + n0 + li;
    for (int k = 0; k < kn; k += 2)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[k * kDdpgLd], wb[k * ld], acc, 0, 0, 0);
    return acc;
}

// ddpg_zwt continued: kn more out-units of dz and of the stage's columns
__device__ __forceinline__ ddpg_f32x16 ddpg_wide_zwt(ddpg_f32x16 acc, const float *dz,
                                                     const float *wbuf, int kn, int ld, int n0) {
    const int lane = threadIdx.x & 63, li = lane & 31, h = lane >> 5;
    const float *za = dz + h * kDdpgLd + li;
    const float *wb = wbuf + (n0 + li) * ld + h;
    for (int k = 0; k < kn; k += 2)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(za[k * kDdpgLd], wb[k], acc, 0, 0, 0);
    return acc;
}

// relu(acc + bias) as column `col` of the k-major buffer `out`
__device__ __forceinline__ void ddpg_wide_relu_out(ddpg_f32x16 acc, float bias, float *out, int col,
                                                   int h) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] += bias;
#pragma unroll
    for (int r = 0; r < 16; ++r) out[col * kDdpgLd + ddpg_acc_row(r, h)] = fmaxf(acc[r], 0.0f);
}

// dX o (x > 0) over the kept activations' column `col`
__device__ __forceinline__ void ddpg_wide_mask_out(const ddpg_f32x16 &acc, float *x, int col, int h) {
    float *c = x + col * kDdpgLd;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = ddpg_acc_row(r, h);
        c[row] = c[row] > 0.0f ? acc[r] : 0.0f;
    }
}

// A first layer over the observation chunks: out = relu(clip(obs) W0 + b0),
// units 0 .. h0 - 1 of `out`.  Barriers inside; ends with one.
__device__ __forceinline__ void ddpg_wide_first(const DdpgPlan &a, int net, const float *img,
                                                const float *obs, const DdpgWideLds &s, float *out) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, h = lane >> 5;
    const int ip = a.in_pad[net][0], op = a.out_pad[net][0], ld = op + 1, n0 = wave * 32;
    ddpg_f32x16 acc = {};
    for (int k0 = 0; k0 < ip; k0 += kDdpgWideChunk) {
        const int kn = ip - k0 < kDdpgWideChunk ? ip - k0 : kDdpgWideChunk;
        __syncthreads();          // the last readers of the chunk and the stage are done
        ddpg_wide_load_obs(s.xc, obs, s.rowsrc, a.D, k0, kn, a.obs_lo, a.obs_hi);
        ddpg_wide_stage(s.wbuf, img + a.off_w[net][0] + k0 * op, kn, op, op);
        __syncthreads();
        if (n0 < op) acc = ddpg_wide_xw(acc, s.xc, s.wbuf, kn, ld, n0);      // wave-uniform
    }
    if (n0 < op) ddpg_wide_relu_out(acc, img[a.off_b[net][0] + n0 + li], out, n0 + li, h);
    __syncthreads();
}

// A layer that fits the stage whole (in, out <= 64): the accumulators of X W
// for this wave's units, no bias (zero on the waves past op).  Barriers
// before the stage and behind it; none after the product.
__device__ __forceinline__ ddpg_f32x16 ddpg_wide_small(const DdpgPlan &a, int net, int l,
                                                       const float *img, const DdpgWideLds &s,
                                                       const float *x) {
    const int ip = a.in_pad[net][l], op = a.out_pad[net][l], n0 = (threadIdx.x >> 6) * 32;
    __syncthreads();
    ddpg_wide_stage(s.wbuf, img + a.off_w[net][l], ip, op, op);
    __syncthreads();
    ddpg_f32x16 acc = {};
    if (n0 < op) acc = ddpg_wide_xw(acc, x, s.wbuf, ip, op + 1, n0);
    return acc;
}

// The end of the critic behind the concat chain `acc1` (no bias yet): with two
// hidden layers relu into ch1 and the 1-wide head, with one the chain is the
// head.  Q of tile row r into qrow[r].  Ends with a barrier.
__device__ __forceinline__ void ddpg_wide_critic_tail(const DdpgPlan &a, const float *img,
                                                      const DdpgWideLds &s, ddpg_f32x16 acc1,
                                                      float *ch1, float *qrow) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, h = lane >> 5;
    const int n0 = wave * 32, col = n0 + li;
    if (a.n_hidden == 2) {
        if (n0 < a.out_pad[1][1]) ddpg_wide_relu_out(acc1, img[a.off_b[1][1] + col], ch1, col, h);
        acc1 = ddpg_wide_small(a, 1, 2, img, s, ch1);
    }
    if (col == 0) {
        const float bias = img[a.off_b[1][a.n_hidden]];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc1[r] += bias;
#pragma unroll
        for (int r = 0; r < 16; ++r) qrow[ddpg_acc_row(r, h)] = acc1[r];
    }
    __syncthreads();
}

// The start of the concat chain: the critic's h0 hidden rows.  Barriers
// before the stage and behind it.
__device__ __forceinline__ ddpg_f32x16 ddpg_wide_concat_head(const DdpgPlan &a, const float *img,
                                                             const DdpgWideLds &s, const float *ch0) {
    const int h0 = a.out_dim[1][0], op1 = a.out_pad[1][1], n0 = (threadIdx.x >> 6) * 32;
    __syncthreads();
    ddpg_wide_stage(s.wbuf, img + a.off_w[1][1], h0, op1, op1);
    __syncthreads();
    ddpg_f32x16 acc1 = {};
    if (n0 < op1) acc1 = ddpg_wide_xw(acc1, ch0, s.wbuf, h0, op1 + 1, n0);
    return acc1;
}

// The actor of image `img` at the tile's observations, its action fed chunk
// by chunk into that image's critic; Q of tile row r into qrow[r].  Leaves the
// actor's layer inputs in hb[0] (h0) and hb[1] (h1, two hidden layers), the
// critic's in hb[2] and hb[3], and, with `sech2`, 1 - a^2 in it [round32(A)]
// [33].  rowsrc is set and a barrier lies behind it.  Ends with a barrier.
__device__ __forceinline__ void ddpg_wide_actor_then_critic(const DdpgPlan &a, const float *img,
                                                            const float *obs, const DdpgWideLds &s,
                                                            float *qrow, float *sech2) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, h = lane >> 5;
    const int n0 = wave * 32, L = a.n_hidden;
    ddpg_wide_first(a, 0, img, obs, s, s.hb[0]);
    ddpg_wide_first(a, 1, img, obs, s, s.hb[2]);
    const float *xlast = s.hb[0];
    if (L == 2) {
        const ddpg_f32x16 acc = ddpg_wide_small(a, 0, 1, img, s, s.hb[0]);
        if (n0 < a.out_pad[0][1])
            ddpg_wide_relu_out(acc, img[a.off_b[0][1] + n0 + li], s.hb[1], n0 + li, h);
        xlast = s.hb[1];        // the barrier of the next stage orders these writes
    }
    const int h0c = a.out_dim[1][0], ip1 = a.in_pad[1][1], op1 = a.out_pad[1][1];
    const int ipL = a.in_pad[0][L], opA = a.out_pad[0][L];
    ddpg_f32x16 acc1 = ddpg_wide_concat_head(a, img, s, s.hb[2]);
    for (int c0 = 0; c0 < opA; c0 += kDdpgWideChunk) {
        const int cn = opA - c0 < kDdpgWideChunk ? opA - c0 : kDdpgWideChunk;
        const int rest = ip1 - h0c - c0, kn = rest < kDdpgWideChunk ? rest : kDdpgWideChunk;
        __syncthreads();
        ddpg_wide_stage(s.wbuf, img + a.off_w[0][L] + c0, ipL, cn, opA);
        __syncthreads();
        if (n0 < cn) {
            ddpg_f32x16 acc = {};
            acc = ddpg_wide_xw(acc, xlast, s.wbuf, ipL, cn + 1, n0);
            const int col = c0 + n0 + li;
            const float bias = img[a.off_b[0][L] + col];
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] += bias;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = ddpg_acc_row(r, h);
                float d;
                const float t = ddpg_tanh(acc[r], &d);
                s.xc[(n0 + li) * kDdpgLd + row] = col < a.A ? t : 0.0f;
                if (sech2) sech2[col * kDdpgLd + row] = d;
            }
        }
        __syncthreads();
        ddpg_wide_stage(s.wbuf, img + a.off_w[1][1] + (h0c + c0) * op1, kn, op1, op1);
        __syncthreads();
        if (n0 < op1) acc1 = ddpg_wide_xw(acc1, s.xc, s.wbuf, kn, op1 + 1, n0);
    }
    ddpg_wide_critic_tail(a, img, s, acc1, s.hb[3], qrow);
}

// ------------------------------------------------------------------------ act
// The generated noise of the wide instance: DdpgActRng with the columns'
// mean and sigma in device memory (2 x 512 floats do not go through the
// kernel arguments).
struct DdpgWideActRng {
    uint32_t seed_lo, seed_hi, t, row0;
    int kind;
    float theta, dt;
    float *ou;
    const uint8_t *reset;
    const float *mean, *sigma;     // [A] each, device
};

template <bool RNG>
__device__ __forceinline__ void ddpg_act_wide_tile(const DdpgActArgs &g, const DdpgWideActRng *n) {
    extern __shared__ __attribute__((aligned(16))) float ddpg_lds_act_wide[];
    const DdpgPlan &a = g.p;
    const DdpgWideLds s = ddpg_wide_lds(ddpg_lds_act_wide);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 31, h = lane >> 5;
    const int n0 = wave * 32, L = a.n_hidden;
    const long long row0 = static_cast<long long>(blockIdx.x) * kDdpgTile;
    const int live = g.rows - row0 < kDdpgTile ? static_cast<int>(g.rows - row0) : kDdpgTile;
    ddpg_tile_rows(s.rowsrc, nullptr, row0, live, g.rows);
    if constexpr (RNG) {      // ddpg_act_tile's draw: one (row, block of four) a thread
        const int nb = (a.A + 3) >> 2;
        for (int i = threadIdx.x; i < live * nb; i += kDdpgBlock) {
            const int r = i / nb, b = i - r * nb;
            const float4 z = rng_normal4(n->seed_lo, n->seed_hi,
                                         n->row0 + static_cast<uint32_t>(row0 + r), n->t,
                                         static_cast<uint32_t>(b), kRngActionNoise);
            float *dst = s.s + 4 * b * kDdpgLd + r;
            dst[0] = z.x;
            dst[kDdpgLd] = z.y;
            dst[2 * kDdpgLd] = z.z;
            dst[3 * kDdpgLd] = z.w;
        }
    }
    __syncthreads();
    ddpg_wide_first(a, 0, g.img, g.obs, s, s.hb[0]);
    const float *xlast = s.hb[0];
    if (L == 2) {
        const ddpg_f32x16 acc = ddpg_wide_small(a, 0, 1, g.img, s, s.hb[0]);
        if (n0 < a.out_pad[0][1])
            ddpg_wide_relu_out(acc, g.img[a.off_b[0][1] + n0 + li], s.hb[1], n0 + li, h);
        xlast = s.hb[1];
    }
    const int ipL = a.in_pad[0][L], opA = a.out_pad[0][L];
    for (int c0 = 0; c0 < opA; c0 += kDdpgWideChunk) {
        const int cn = opA - c0 < kDdpgWideChunk ? opA - c0 : kDdpgWideChunk;
        __syncthreads();
        ddpg_wide_stage(s.wbuf, g.img + a.off_w[0][L] + c0, ipL, cn, opA);
        __syncthreads();
        if (n0 >= cn) continue;      // wave-uniform
        const int col = c0 + n0 + li;
        const bool on = col < a.A;
        ddpg_f32x16 acc = {};
        acc = ddpg_wide_xw(acc, xlast, s.wbuf, ipL, cn + 1, n0);
        const float bias = g.img[a.off_b[0][L] + col];
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] += bias;
        const float sc = g.scale[col];
        float mean = 0.0f, sigma = 0.0f;
        if constexpr (RNG) {
            mean = n->mean[col];
            sigma = n->sigma[col];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = ddpg_acc_row(r, h);
            if (on && row < live) {
                const long long o = (row0 + row) * a.A + col;
                float d;
                float act = ddpg_tanh(acc[r], &d);
                if constexpr (RNG) {
#pragma clang fp contract(off)
                    const float z = s.s[col * kDdpgLd + row];
                    float noise;
                    if (n->kind == kDdpgNoiseOu) {
                        float x = n->ou[o];
                        if (n->reset && n->reset[row0 + row]) x = 0.0f;
                        noise = (x + (n->theta * (mean - x)) * n->dt) + sigma * z;
                        n->ou[o] = noise;
                    } else {
                        noise = mean + sigma * z;
                    }
                    act = fminf(fmaxf(act + noise, -1.0f), 1.0f);
                } else {
                    if (g.noise) act = fminf(fmaxf(act + g.noise[o], -1.0f), 1.0f);
                }
                g.action[o] = act;
                g.env_action[o] = act * sc;
            }
        }
    }
}

__global__ __launch_bounds__(kDdpgBlock) void ddpg_act_wide_kernel(const DdpgActArgs g) {
    ddpg_act_wide_tile<false>(g, nullptr);
}

__global__ __launch_bounds__(kDdpgBlock) void ddpg_act_rng_wide_kernel(const DdpgActArgs g,
                                                                       const DdpgWideActRng n) {
    ddpg_act_wide_tile<true>(g, &n);
}

// --------------------------------------------------------------------- target
__global__ __launch_bounds__(kDdpgBlock) void ddpg_target_wide_kernel(const DdpgTargetArgs g) {
    extern __shared__ __attribute__((aligned(16))) float ddpg_lds_target_wide[];
    const DdpgPlan &a = g.p;
    const DdpgWideLds s = ddpg_wide_lds(ddpg_lds_target_wide);
    const int tid = threadIdx.x;
    const long long row0 = static_cast<long long>(blockIdx.x) * kDdpgTile;
    const int live = g.n - row0 < kDdpgTile ? static_cast<int>(g.n - row0) : kDdpgTile;
    ddpg_tile_rows(s.rowsrc, g.idx, row0, live, g.m);
    __syncthreads();
    ddpg_wide_actor_then_critic(a, g.timg, g.obs1, s, s.rowf, nullptr);
    if (tid < live) {
        const int src = s.rowsrc[tid];
        const float nonterminal = 1.0f - (g.dones[src] != 0 ? 1.0f : 0.0f);
        g.y[row0 + tid] = g.rewards[src] + g.gamma * nonterminal * s.rowf[tid];
    }
}

// ------------------------------------------------------------------- gradient
// Block (mi, ni) of a layer's dW += X^T dZ with its C operand in the slab
// partial: `w` is the layer's image in the partial ([ip][op]), `xa` this
// lane's row of X (k-major; `valid`: the row exists), `dz` the layer's dZ.
__device__ __forceinline__ void ddpg_wide_dw(float *w, int ip, int op, int mi, int ni,
                                             const float *xa, bool valid, const float *dz,
                                             bool first) {
    const int lane = threadIdx.x & 63, li = lane & 31, h = lane >> 5;
    float *blk = w + static_cast<long long>(mi) * 32 * op + ni * 32 + li;
    const int rows = ip - mi * 32;
    ddpg_f32x16 c = {};
    if (!first) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = ddpg_acc_row(r, h);
            if (row < rows) c[r] = blk[row * op];
        }
    }
    const float *x = xa + h;
    const float *zb = dz + (ni * 32 + li) * kDdpgLd + h;
#pragma unroll
    for (int k = 0; k < kDdpgTile; k += 2)
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(valid ? x[k] : 0.0f, zb[k], c, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = ddpg_acc_row(r, h);
        if (row < rows) blk[row * op] = c[r];
    }
}

// The dW blocks of the layer rows row0 .. row0 + kn - 1 whose X stands in `x`
// (k-major, its row 0 the layer's row row0; row0 a multiple of 32): block b =
// wave + 4 j of the [ceil(kn / 32)][op / 32] grid.
__device__ __forceinline__ void ddpg_wide_dw_rows(float *w, int ip, int op, int row0, int kn,
                                                  const float *x, const float *dz, bool first) {
    const int wave = threadIdx.x >> 6, li = threadIdx.x & 31;
    const int nni = op >> 5, nb = ((kn + 31) >> 5) * nni;
    for (int b = wave; b < nb; b += 4) {      // wave-uniform
        const int mi = b / nni, ni = b - mi * nni;
        const int mrow = mi * 32 + li;
        const bool valid = mrow < kn;
        ddpg_wide_dw(w, ip, op, (row0 >> 5) + mi, ni, x + (valid ? mrow : 0) * kDdpgLd, valid, dz,
                     first);
    }
}

// sum over the tile's rows of dz's column `col`, rows in order
__device__ __forceinline__ float ddpg_wide_colsum(const float *dz, int col) {
    const float *c = dz + col * kDdpgLd;
    float s = 0.0f;
    for (int r = 0; r < kDdpgTile; ++r) s += c[r];
    return s;
}

// db_0 and dW_0 += X_0^T dZ_0 of a first layer over the observation chunks.
// A barrier lies behind the last writer of dz.  No barrier at the end.
__device__ __forceinline__ void ddpg_wide_first_back(const DdpgPlan &a, int net, float *part,
                                                     const float *obs, const DdpgWideLds &s,
                                                     const float *dz, bool first, float *db0) {
    const int ip = a.in_pad[net][0], op = a.out_pad[net][0];
    if (threadIdx.x < static_cast<unsigned>(op)) *db0 += ddpg_wide_colsum(dz, threadIdx.x);
    for (int k0 = 0; k0 < ip; k0 += kDdpgWideChunk) {
        const int kn = ip - k0 < kDdpgWideChunk ? ip - k0 : kDdpgWideChunk;
        __syncthreads();
        ddpg_wide_load_obs(s.xc, obs, s.rowsrc, a.D, k0, kn, a.obs_lo, a.obs_hi);
        __syncthreads();
        ddpg_wide_dw_rows(part + a.off_w[net][0], ip, op, k0, kn, s.xc, dz, first);
    }
}

__global__ __launch_bounds__(kDdpgBlock) void ddpg_grad_wide_kernel(const DdpgGradArgs g) {
    extern __shared__ __attribute__((aligned(16))) float ddpg_lds_grad_wide[];
    const DdpgPlan &a = g.p;
    const DdpgWideLds s = ddpg_wide_lds(ddpg_lds_grad_wide);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 31, h = lane >> 5, n0 = wave * 32;
    const int branch = blockIdx.y;
    const int L = a.n_hidden;
    const int h0c = a.out_dim[1][0], ip1 = a.in_pad[1][1], op1 = a.out_pad[1][1], ld1 = op1 + 1;
    const int ipL = a.in_pad[0][L], opA = a.out_pad[0][L];
    const int na = ip1 - h0c;                  // round4(A): the concat layer's action rows
    const float inv_n = 1.0f / static_cast<float>(g.n_total);
    float *ah0 = s.hb[0], *ah1 = s.hb[1], *ch0 = s.hb[2], *ch1 = s.hb[3];
    float *qrow = s.rowf, *yrow = s.rowf + kDdpgTile;
    float *part = g.slab + static_cast<long long>(blockIdx.x) * a.img_floats;

    float db[kDdpgLayers] = {};
    float dbh = 0.0f;             // the actor's head column tid + 256
    double stat_acc = 0.0;        // thread t < kDdpgRowStats keeps statistic t

    for (int tile = blockIdx.x; tile < g.tiles; tile += g.grid) {
        const bool first = tile == static_cast<int>(blockIdx.x);
        const long long row0 = static_cast<long long>(tile) * kDdpgTile;
        const int live = g.n - row0 < kDdpgTile ? static_cast<int>(g.n - row0) : kDdpgTile;
        __syncthreads();       // the previous tile's last LDS readers are done
        ddpg_tile_rows(s.rowsrc, g.idx, row0, live, g.m);
        __syncthreads();

        if (branch == 0) {
            // ------------------------------------------------ the critic's loss
            if (tid < kDdpgTile) yrow[tid] = tid < live ? g.y[row0 + tid] : 0.0f;
            ddpg_wide_first(a, 1, g.img, g.obs0, s, ch0);
            ddpg_f32x16 acc1 = ddpg_wide_concat_head(a, g.img, s, ch0);
            for (int c0 = 0; c0 < na; c0 += kDdpgWideChunk) {      // the stored action
                const int kn = na - c0 < kDdpgWideChunk ? na - c0 : kDdpgWideChunk;
                __syncthreads();
                ddpg_wide_load_act(s.xc, g.actions, s.rowsrc, a.A, c0, kn);
                ddpg_wide_stage(s.wbuf, g.img + a.off_w[1][1] + (h0c + c0) * op1, kn, op1, op1);
                __syncthreads();
                if (n0 < op1) acc1 = ddpg_wide_xw(acc1, s.xc, s.wbuf, kn, ld1, n0);
            }
            ddpg_wide_critic_tail(a, g.img, s, acc1, ch1, qrow);
            // the head's dZ: column 0 carries 2 (Q - y) / N, the padding zeros
            for (int i = tid; i < kDdpgTile * kDdpgTile; i += kDdpgBlock) {
                const int c = i / kDdpgTile, r = i & (kDdpgTile - 1);
                s.dzc[c * kDdpgLd + r] =
                    (c == 0 && r < live) ? 2.0f * (qrow[r] - yrow[r]) * inv_n : 0.0f;
            }
            if (tid < 3) {        // err^2, Q, y: rows in order, float64
                double sum = 0.0;
                for (int r = 0; r < live; ++r) {
                    const double q = qrow[r], y = yrow[r];
                    sum += tid == 0 ? (q - y) * (q - y) : (tid == 1 ? q : y);
                }
                stat_acc += sum;
            }
            __syncthreads();
            const float *dz1 = s.dzc;
            if (L == 2) {         // the 1-wide head over ch1
                ddpg_wide_dw_rows(part + a.off_w[1][2], a.in_pad[1][2], 32, 0, a.in_pad[1][2], ch1,
                                  s.dzc, first);
                if (tid < 32) db[2] += ddpg_wide_colsum(s.dzc, tid);
                __syncthreads();          // every dW_2 read of ch1 is done
                ddpg_wide_stage(s.wbuf, g.img + a.off_w[1][2], a.in_pad[1][2], 32, 32);
                __syncthreads();
                if (n0 < a.out_dim[1][1]) {
                    ddpg_f32x16 acc = {};
                    acc = ddpg_wide_zwt(acc, s.dzc, s.wbuf, 32, 33, n0);
                    ddpg_wide_mask_out(acc, ch1, n0 + li, h);
                }
                __syncthreads();
                dz1 = ch1;
            }
            // the concat layer: the hidden rows, then the action rows again
            ddpg_wide_dw_rows(part + a.off_w[1][1], ip1, op1, 0, h0c, ch0, dz1, first);
            if (tid < op1) db[1] += ddpg_wide_colsum(dz1, tid);
            for (int c0 = 0; c0 < na; c0 += kDdpgWideChunk) {
                const int kn = na - c0 < kDdpgWideChunk ? na - c0 : kDdpgWideChunk;
                __syncthreads();
                ddpg_wide_load_act(s.xc, g.actions, s.rowsrc, a.A, c0, kn);
                __syncthreads();
                ddpg_wide_dw_rows(part + a.off_w[1][1], ip1, op1, h0c + c0, kn, s.xc, dz1, first);
            }
            __syncthreads();              // every dW_1 read of ch0 is done
            ddpg_wide_stage(s.wbuf, g.img + a.off_w[1][1], h0c, op1, op1);
            __syncthreads();
            if (n0 < h0c) {               // the hidden units only: the action rows get no dZ
                ddpg_f32x16 acc = {};
                acc = ddpg_wide_zwt(acc, dz1, s.wbuf, op1, ld1, n0);
                ddpg_wide_mask_out(acc, ch0, n0 + li, h);
            }
            __syncthreads();
            ddpg_wide_first_back(a, 1, part, g.obs0, s, ch0, first, &db[0]);
        } else {
            // ----------------------------- the actor's loss through the critic
            ddpg_wide_actor_then_critic(a, g.img, g.obs0, s, qrow, s.s);
            // the critic's head dZ = -1 / N on the live rows
            for (int i = tid; i < kDdpgTile * kDdpgTile; i += kDdpgBlock) {
                const int c = i / kDdpgTile, r = i & (kDdpgTile - 1);
                s.dzc[c * kDdpgLd + r] = (c == 0 && r < live) ? -inv_n : 0.0f;
            }
            if (tid == 0) {
                double sum = 0.0;
                for (int r = 0; r < live; ++r) sum += qrow[r];
                stat_acc += sum;
            }
            __syncthreads();
            // the critic's backward to d / d action: no dW, masks from the
            // kept activations
            const float *dz1 = s.dzc;
            if (L == 2) {
                ddpg_wide_stage(s.wbuf, g.img + a.off_w[1][2], a.in_pad[1][2], 32, 32);
                __syncthreads();
                if (n0 < a.out_dim[1][1]) {
                    ddpg_f32x16 acc = {};
                    acc = ddpg_wide_zwt(acc, s.dzc, s.wbuf, 32, 33, n0);
                    ddpg_wide_mask_out(acc, ch1, n0 + li, h);
                }
                dz1 = ch1;        // the barrier of the next stage orders these writes
            }
            // the actor's head dZ = d / d action o (1 - a^2) in place, zero past
            // A.  Rows of the stage past the concat layer's in_pad are not
            // staged: the columns they give are past A.
            for (int c0 = 0; c0 < opA; c0 += kDdpgWideChunk) {
                const int cn = opA - c0 < kDdpgWideChunk ? opA - c0 : kDdpgWideChunk;
                const int kn = na - c0 < kDdpgWideChunk ? na - c0 : kDdpgWideChunk;
                __syncthreads();
                ddpg_wide_stage(s.wbuf, g.img + a.off_w[1][1] + (h0c + c0) * op1, kn, op1, op1);
                __syncthreads();
                if (n0 < cn) {
                    ddpg_f32x16 da = {};
                    da = ddpg_wide_zwt(da, dz1, s.wbuf, op1, ld1, n0);
                    const int col = c0 + n0 + li;
                    const bool on = col < a.A;
                    float *sc = s.s + col * kDdpgLd;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = ddpg_acc_row(r, h);
                        sc[row] = on ? da[r] * sc[row] : 0.0f;
                    }
                }
            }
            __syncthreads();
            // the actor's backward: the head over the last hidden layer
            float *xl = L == 2 ? ah1 : ah0;
            ddpg_wide_dw_rows(part + a.off_w[0][L], ipL, opA, 0, ipL, xl, s.s, first);
            if (tid < opA) {
                const float sum = ddpg_wide_colsum(s.s, tid);
                if (L == 2)
                    db[2] += sum;
                else
                    db[1] += sum;
            }
            if (tid + kDdpgBlock < opA) dbh += ddpg_wide_colsum(s.s, tid + kDdpgBlock);
            ddpg_f32x16 dx = {};
            for (int c0 = 0; c0 < opA; c0 += kDdpgWideChunk) {
                const int cn = opA - c0 < kDdpgWideChunk ? opA - c0 : kDdpgWideChunk;
                __syncthreads();          // at c0 = 0: every dW read of xl is done too
                ddpg_wide_stage(s.wbuf, g.img + a.off_w[0][L] + c0, ipL, cn, opA);
                __syncthreads();
                if (n0 < ipL) dx = ddpg_wide_zwt(dx, s.s + c0 * kDdpgLd, s.wbuf, cn, cn + 1, n0);
            }
            if (n0 < ipL) ddpg_wide_mask_out(dx, xl, n0 + li, h);
            __syncthreads();
            if (L == 2) {
                ddpg_wide_dw_rows(part + a.off_w[0][1], a.in_pad[0][1], a.out_pad[0][1], 0,
                                  a.in_pad[0][1], ah0, ah1, first);
                if (tid < a.out_pad[0][1]) db[1] += ddpg_wide_colsum(ah1, tid);
                __syncthreads();          // every dW_1 read of ah0 is done
                ddpg_wide_stage(s.wbuf, g.img + a.off_w[0][1], a.in_pad[0][1], a.out_pad[0][1],
                                a.out_pad[0][1]);
                __syncthreads();
                if (n0 < a.out_dim[0][0]) {
                    ddpg_f32x16 acc = {};
                    acc = ddpg_wide_zwt(acc, ah1, s.wbuf, a.out_pad[0][1], a.out_pad[0][1] + 1, n0);
                    ddpg_wide_mask_out(acc, ah0, n0 + li, h);
                }
                __syncthreads();
            }
            ddpg_wide_first_back(a, 0, part, g.obs0, s, ah0, first, &db[0]);
        }
    }

    const int net = branch == 0 ? 1 : 0;
#pragma unroll
    for (int l = 0; l < kDdpgLayers; ++l)
        if (l <= L && tid < a.out_pad[net][l]) part[a.off_b[net][l] + tid] = db[l];
    if (net == 0 && tid + kDdpgBlock < opA) part[a.off_b[0][L] + tid + kDdpgBlock] = dbh;
    if (tid < kDdpgRowStats)
        g.stat_slab[(static_cast<long long>(blockIdx.x) * 2 + branch) * kDdpgRowStats + tid] = stat_acc;
}

}  // namespace ce
