// The DDPG learner's kernels (gfx950): the deterministic relu actor with its
// tanh head, the Q critic that takes the action in after its first layer, the
// target y from the target networks, both loss gradients (the actor's taken
// through the critic), and Adam x2 + the soft update + the images' repack.
// custom_envs_amd/ddpg.py states the semantics in NumPy.
//
// Tile conventions are policy_kernels.h's: 32-row tiles, 256 threads (4
// waves, wave w owns output units 32w .. 32w + 31), float32 on
// v_mfma_f32_32x32x2_f32 with the rows along M, activations in LDS k-major
// with a 33-word column, every layer's weights staged from a padded image
// [round4(in)][round32(out)] as [in][out + 1] (the odd row stride serves both
// X W and dZ W^T from one stage, as ppo_grad_tile.h does).  The observation is
// clipped to the observation range as the tile is loaded.  Two images of one
// layout hold the online and the target networks (actor, then critic).
//
// The concat of the critic is a row offset: the activation buffer of its
// second layer is [h0 + A] k-rows, the first layer's relu units in rows 0 ..
// h0 - 1 and the action in rows h0 .. h0 + A - 1, and the staged W_1 has the
// same rows, so neither the forward nor dW_1 = X_1^T dZ_1 copies anything and
// dQ / d action is the in-chunks h0, h0 + 32 of dZ_1 W_1^T.
//
// ddpg_act_kernel      grid ceil(rows / 32): obs tile -> actor chain -> tanh
//                      (+ noise, clip to [-1, 1]) -> action, action * scale.
// ddpg_act_rng_kernel  the same tile with the noise formed in the epilogue from
//                      rng.h's stream (Normal or Ornstein-Uhlenbeck).
// ddpg_target_kernel   grid ceil(n / 32), rows gathered by idx: obs1 tile once,
//                      the target actor's action left in LDS as the concat rows
//                      of the target critic's second layer, the target critic,
//                      y = r + gamma (1 - done) Q'.
// ddpg_grad_kernel     persistent grid (G, 2), G = min(tiles, grid_max);
//                      workgroup x walks tiles x, x + G, ...
//     y == 0  the critic: forward at (obs0, action), dZ = 2 (Q - y) / N,
//             backward with every layer's dW in MFMA accumulators and db in
//             registers across the workgroup's tiles.
//     y == 1  the actor: its forward, the critic's forward at the actor's own
//             action, the critic's backward to dQ / d action only (no dW; relu
//             masks from the kept activations) started from dZ = -1 / N, the
//             head's dZ = that o (1 - a^2), the actor's backward with dW, db.
//     Rows past n contribute exact zeros (their head dZ is 0).  N is the
//     call's n_total: its own n, or every rank's rows under a gradient
//     exchange.  The partials leave the workgroup once, as partial x of a
//     slab of images.
// ddpg_reduce_kernel   grad[p] = the G partials of parameter p's image element,
//                      added in workgroup order in float64, rounded once.
// ddpg_stats_kernel    one workgroup: the statistic sums over the partials (the
//                      G workgroups' of the slab, or the W ranks' inside their
//                      records) in order and the two squared gradient norms,
//                      float64.
// ddpg_partial_kernel  the reduce kernel's sums left in float64, with the
// ddpg_combine_kernel  statistic sums and the row count, as one rank's record;
//                      the W records added in rank order and rounded once (the
//                      gradient exchange, below the reduce kernel).
// ddpg_update_kernel   per parameter: Adam (TF form, eps outside the root, the
//                      block's own lr_t), the soft update with its float32
//                      multiplies and adds unfused and in the statement's
//                      order, and both images' elements.  Padding is zeroed
//                      once at create and never written.
//
// The tanh head's derivative is kept beside its value as 1 - a^2 = 4 e / (1 +
// e)^2, e = exp(-2 |z|): 1 - a^2 from a rounded a is off by up to 1.2e-7
// absolute where tanh saturates, which is the whole of a saturated row's
// gradient (7e-4 of the largest entry in the float32 NumPy statement at one
// clipped row).
//
// LDS at the limits (D = 128, hidden 64 + 64, A = 64): weight stage 128 x 65,
// six activation buffers 128 x 33 (obs; actor h0, h1; critic concat, h1; head
// dZ), row scalars, the head's derivative 64 x 33: 35 904 floats = 143 616 B
// of the CU's 160 KiB (kDdpgMaxLdsBytes).  A 128-wide layer would need a
// [192][129] stage and does not fit without a split stage; it is not supported.
//
// No floating-point atomics: the same inputs with the same G give the same
// bits.  Different G regroup the float32 per-workgroup sums.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "rng.h"

namespace ce {

constexpr int kDdpgBlock = 256;      // 4 waves
constexpr int kDdpgTile = 32;        // rows per tile (the MFMA's M)
constexpr int kDdpgLd = 33;          // LDS words per activation column
constexpr int kDdpgMaxHidden = 2;
constexpr int kDdpgLayers = kDdpgMaxHidden + 1;     // hidden layers + the head
constexpr int kDdpgMaxD = 128;
constexpr int kDdpgMaxA = 64;
constexpr int kDdpgBufs = 6;         // activation buffers of the gradient kernel
constexpr int kDdpgActBufs = 3;      // of the act kernel
constexpr int kDdpgRowStats = 4;     // per-branch sums (critic: err^2, Q, y; actor: Q)
constexpr int kDdpgSegs = 4 * kDdpgLayers;          // (W, b) per layer per network
constexpr int kDdpgRowFloats = 4 * kDdpgTile;       // Q, y, one spare row, rowsrc
// LDS of the gradient kernel at the shape limits
constexpr int kDdpgMaxLdsBytes =
    (128 * 65 + kDdpgBufs * 128 * kDdpgLd + kDdpgRowFloats + kDdpgMaxA * kDdpgLd) * 4;

typedef float ddpg_f32x16 __attribute__((ext_vector_type(16)));
__device__ __forceinline__ int ddpg_acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// The shape, both images' layout and the flat vector's segments.  net 0 is
// the actor, net 1 the critic; layer n_hidden is the head.
struct DdpgPlan {
    int D, A, n_hidden, n_params, n_actor, img_floats;
    int out_dim[2][kDdpgLayers];
    int in_pad[2][kDdpgLayers], out_pad[2][kDdpgLayers];
    int off_w[2][kDdpgLayers], off_b[2][kDdpgLayers];      // image offsets (multiples of 4)
    int n_segs;                                            // flat order: W, b per layer, actor first
    int seg_src[kDdpgSegs], seg_dst[kDdpgSegs], seg_cols[kDdpgSegs], seg_cols_pad[kDdpgSegs];
    int w_floats, act_floats;                              // LDS floats: weight stage, one buffer
    float obs_lo, obs_hi;
};

// the image element flat parameter p packs to
__device__ __forceinline__ int ddpg_image_pos(const DdpgPlan &a, int p) {
    int s = 0;
    while (s + 1 < a.n_segs && a.seg_src[s + 1] <= p) ++s;
    const int i = p - a.seg_src[s], cols = a.seg_cols[s];
    const int r = i / cols, c = i - r * cols;
    return a.seg_dst[s] + r * a.seg_cols_pad[s] + c;
}

__device__ __forceinline__ int ddpg_src_row(const int32_t *idx, long long i, int m) {
    if (!idx) return static_cast<int>(i);
    const int s = idx[i];
    return s < 0 ? 0 : (s >= m ? m - 1 : s);     // never read out of bounds
}

// The actor's head: a = tanh z and *d = 1 - a^2, both from e = exp(-2 |z|)
// (see the header comment).  Every kernel forms the action with this one
// function, so the action `act` stores and the action the target and the
// gradient work at are the same bits for the same parameters and row.
__device__ __forceinline__ float ddpg_tanh(float z, float *d) {
    const float e = expf(-2.0f * fabsf(z));
    *d = 4.0f * e / ((1.0f + e) * (1.0f + e));
    return copysignf((1.0f - e) / (1.0f + e), z);
}

// ---------------------------------------------------------------- tile pieces
// (every piece is called by all 256 threads; a piece that ends with a barrier
// says so)

__device__ __forceinline__ void ddpg_stage_w(float *wbuf, const float *img, int ip, int op) {
    const float4 *src = reinterpret_cast<const float4 *>(img);
    const int n4 = ip * op / 4, ld = op + 1;
    for (int i = threadIdx.x; i < n4; i += kDdpgBlock) {
        const float4 v = src[i];
        const int r = (4 * i) / op, c = 4 * i - r * op;
        float *d = wbuf + r * ld + c;
        d[0] = v.x;
        d[1] = v.y;
        d[2] = v.z;
        d[3] = v.w;
    }
}

// rowsrc[r] = the source row of tile row r, -1 past the last row.  No barrier.
__device__ __forceinline__ void ddpg_tile_rows(int *rowsrc, const int32_t *idx, long long row0,
                                               int live, int m) {
    const int tid = threadIdx.x;
    if (tid < kDdpgTile) rowsrc[tid] = tid < live ? ddpg_src_row(idx, row0 + tid, m) : -1;
}

// The observation tile, clipped, k-major, zero past D and past the last row.
// Reads rowsrc: a barrier lies between ddpg_tile_rows and this.  No barrier.
__device__ __forceinline__ void ddpg_load_obs(float *x, const float *obs, const int *rowsrc, int D,
                                              int dp, float lo, float hi) {
    for (int i = threadIdx.x; i < kDdpgTile * dp; i += kDdpgBlock) {
        const int r = i / dp, k = i - r * dp;
        const int s = rowsrc[r];
        float v = 0.0f;
        if (s >= 0 && k < D) {
            v = obs[static_cast<long long>(s) * D + k];
            v = fminf(fmaxf(v, lo), hi);
        }
        x[k * kDdpgLd + r] = v;
    }
}

// X W for this wave's output units n0 .. n0 + 31: x k-major [ip][33], the
// stage [ip][ld].
__device__ __forceinline__ ddpg_f32x16 ddpg_xw(const float *x, const float *wbuf, int ip, int ld,
                                               int n0) {
    const int lane = threadIdx.x & 63, li = lane & 31, h = lane >> 5;
    const float *xa = x + h * kDdpgLd + li;
    const float *wb = wbuf + h * ld + n0 + li;
    ddpg_f32x16 acc = {};
    for (int k = 0; k < ip; k += 2)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[k * kDdpgLd], wb[k * ld], acc, 0, 0, 0);
    return acc;
}

// dZ W^T for the in-units n0 .. n0 + 31 of the staged layer: dz k-major
// [op][33].  Rows of the stage past the layer's in_pad are never staged: the
// columns they give are the caller's to drop.
__device__ __forceinline__ ddpg_f32x16 ddpg_zwt(const float *dz, const float *wbuf, int op, int ld,
                                                int n0) {
    const int lane = threadIdx.x & 63, li = lane & 31, h = lane >> 5;
    const float *za = dz + h * kDdpgLd + li;
    const float *wb = wbuf + (n0 + li) * ld + h;
    ddpg_f32x16 acc = {};
    for (int k = 0; k < op; k += 2)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(za[k * kDdpgLd], wb[k], acc, 0, 0, 0);
    return acc;
}

// One network's forward over the tile.  xs[l] is layer l's input (k-major,
// zero past its in width up to in_pad); hidden layer l writes relu units 0 ..
// out - 1 of xs[l + 1]; the head's pre-activation, bias included, goes to
// head(acc, col) on the waves that own head columns.  The caller has a barrier
// behind the last reader of wbuf and the last writer of xs[0]'s rows other
// than this tile's load; the head's weights stay staged.  Ends with a barrier.
template <class Head>
__device__ __forceinline__ void ddpg_forward(const DdpgPlan &a, int net, const float *img,
                                             float *wbuf, float *const *xs, Head &&head) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 31, h = lane >> 5;
    const int L = a.n_hidden;
    for (int l = 0; l <= L; ++l) {
        const int ip = a.in_pad[net][l], op = a.out_pad[net][l], ld = op + 1;
        ddpg_stage_w(wbuf, img + a.off_w[net][l], ip, op);
        __syncthreads();
        const int n0 = wave * 32;
        if (n0 < op) {      // wave-uniform
            ddpg_f32x16 acc = ddpg_xw(xs[l], wbuf, ip, ld, n0);
            const int col = n0 + li;
            const float bias = img[a.off_b[net][l] + col];
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] += bias;
            if (l < L) {
                float *nxt = xs[l + 1];
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    nxt[col * kDdpgLd + ddpg_acc_row(r, h)] = fmaxf(acc[r], 0.0f);
            } else {
                head(acc, col);
            }
        }
        __syncthreads();
    }
}

// The rows h0 + A .. in_pad - 1 of the critic's concat buffer are zero, so
// the padded rows of the product add nothing.  No barrier.
__device__ __forceinline__ void ddpg_zero_concat_pad(const DdpgPlan &a, float *c1) {
    const int first = a.out_dim[1][0] + a.A, n = (a.in_pad[1][1] - first) * kDdpgTile;
    for (int i = threadIdx.x; i < n; i += kDdpgBlock)
        c1[(first + i / kDdpgTile) * kDdpgLd + (i & (kDdpgTile - 1))] = 0.0f;
}

// One network's backward over the tile with the parameter gradients kept on
// chip: per layer, top down, dW_l += X_l^T dZ_l (block b = wave + 4 j of the
// [ceil(in / 32)][out / 32] grid), db_l += sum_rows dZ_l, dX = dZ_l W_l^T over
// the previous layer's units and dZ_{l-1} = dX o (X_l > 0) written over X_l.
// `staged`: the head's weights are still in wbuf.  Every barrier the pieces
// need is inside; ends with one.
template <int NET>
__device__ __forceinline__ void ddpg_backward(const DdpgPlan &a, const float *img, float *wbuf,
                                              float *const *xs, const float *dzh, bool staged,
                                              ddpg_f32x16 (&dw)[kDdpgLayers][2],
                                              float (&db)[kDdpgLayers]) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 31, h = lane >> 5;
    const int L = a.n_hidden;
#pragma unroll
    for (int l = kDdpgLayers - 1; l >= 0; --l) {
        if (l > L) continue;
        const int ip = a.in_pad[NET][l], op = a.out_pad[NET][l], ld = op + 1;
        float *x = xs[l];
        const float *dz = l == L ? dzh : xs[l + 1];
        if (l > 0 && !(l == L && staged)) ddpg_stage_w(wbuf, img + a.off_w[NET][l], ip, op);
        const int nni = op >> 5, nb = ((ip + 31) >> 5) * nni;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int b = wave + 4 * j;
            if (b < nb) {   // wave-uniform
                const int mi = b / nni, ni = b - mi * nni;
                const int mrow = mi * 32 + li;
                const bool valid = mrow < ip;
                const float *xa = x + (valid ? mrow : 0) * kDdpgLd + h;
                const float *zb = dz + (ni * 32 + li) * kDdpgLd + h;
#pragma unroll
                for (int k = 0; k < kDdpgTile; k += 2)
                    dw[l][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(valid ? xa[k] : 0.0f, zb[k],
                                                                    dw[l][j], 0, 0, 0);
            }
        }
        if (tid < op) {
            const float *col = dz + tid * kDdpgLd;
            float s = 0.0f;
            for (int r = 0; r < kDdpgTile; ++r) s += col[r];
            db[l] += s;
        }
        __syncthreads();          // W_l staged; every dW_l read of X_l is done
        if (l > 0) {
            const int n0 = wave * 32, prev = a.out_dim[NET][l - 1];
            if (n0 < prev) {      // the hidden units only: the critic's action rows get no dZ
                const ddpg_f32x16 acc = ddpg_zwt(dz, wbuf, op, ld, n0);
                float *col = x + (n0 + li) * kDdpgLd;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = ddpg_acc_row(r, h);
                    col[row] = col[row] > 0.0f ? acc[r] : 0.0f;
                }
            }
            __syncthreads();
        }
    }
}

// This workgroup's parameter-gradient partial of one network into the slab.
template <int NET>
__device__ __forceinline__ void ddpg_store_partial(const DdpgPlan &a, float *part,
                                                   const ddpg_f32x16 (&dw)[kDdpgLayers][2],
                                                   const float (&db)[kDdpgLayers]) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 31, h = lane >> 5;
#pragma unroll
    for (int l = 0; l < kDdpgLayers; ++l) {
        if (l > a.n_hidden) continue;
        const int ip = a.in_pad[NET][l], op = a.out_pad[NET][l];
        const int nni = op >> 5, nb = ((ip + 31) >> 5) * nni;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int b = wave + 4 * j;
            if (b < nb) {
                const int mi = b / nni, ni = b - mi * nni;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = mi * 32 + ddpg_acc_row(r, h);
                    if (row < ip) part[a.off_w[NET][l] + row * op + ni * 32 + li] = dw[l][j][r];
                }
            }
        }
        if (tid < op) part[a.off_b[NET][l] + tid] = db[l];
    }
}

// the LDS of the three tile kernels: [wbuf | bufs x act_floats | row scalars |
// the head's derivative (gradient kernel only)]
struct DdpgLds {
    float *wbuf, *buf[kDdpgBufs], *rowf, *sech2;
    int *rowsrc;
};
__device__ __forceinline__ DdpgLds ddpg_lds(float *base, const DdpgPlan &a, int bufs) {
    DdpgLds s;
    s.wbuf = base;
    for (int i = 0; i < kDdpgBufs; ++i) s.buf[i] = base + a.w_floats + (i < bufs ? i : 0) * a.act_floats;
    s.rowf = base + a.w_floats + bufs * a.act_floats;     // [32] Q, [32] y, one spare row
    s.rowsrc = reinterpret_cast<int *>(s.rowf + 3 * kDdpgTile);
    s.sech2 = s.rowf + kDdpgRowFloats;                    // [round32(A)][33]
    return s;
}

// ------------------------------------------------------------------------ act
struct DdpgActArgs {
    DdpgPlan p;
    int rows;
    const float *img;        // the online image
    const float *scale;      // [A]
    const float *obs;        // [rows][D]
    const float *noise;      // [rows][A] or null
    float *action, *env_action;
};

// The noise the generated instance forms (ce_ddpg_act_rng): tile row r, column
// c take z = rng_normal4(seed, row0 + r, t, c / 4, kRngActionNoise)[c % 4], then
//   Normal  n  = mean + sigma * z
//   OU      x' = (x + (theta * (mean - x)) * dt) + s * z,  n = x'
// (stable-baselines' NormalActionNoise / OrnsteinUhlenbeckActionNoise; sigma
// holds s = float32(sigma sqrt(dt)) for OU), every operation float32 and
// unfused.  x is the caller's [rows][A] state, read as 0 where reset[r] != 0;
// the thread that owns (r, c) in the epilogue reads and writes its element.
//
// The tile's z are drawn by all 256 threads, one (row, block of four) each,
// into an LDS block [round4(A)][33] behind the row scalars (where the gradient
// kernel keeps the head's derivative) while the observation tile loads; the
// forward's barriers lie between that and the epilogue, which reads z[c][r].
// Drawn inside the epilogue instead, the one wave that owns an A <= 32 head
// runs 16 Philox + Box-Muller chains per lane with three waves idle: 29.5 us
// a launch against 14.9 us for the tensor instance at 4096 rows, 41 -> 20.
constexpr int kDdpgNoiseNormal = 0, kDdpgNoiseOu = 1;
struct DdpgActRng {
    uint32_t seed_lo, seed_hi, t, row0;
    int kind;
    float theta, dt;
    float *ou;                 // [rows][A], OU only
    const uint8_t *reset;      // [rows] or null, OU only
    float mean[kDdpgMaxA], sigma[kDdpgMaxA];
};

// `n` is read by the RNG instance only.
template <bool RNG>
__device__ __forceinline__ void ddpg_act_tile(const DdpgActArgs &g, const DdpgActRng *n) {
    extern __shared__ __attribute__((aligned(16))) float ddpg_lds_act[];
    const DdpgPlan &a = g.p;
    const DdpgLds s = ddpg_lds(ddpg_lds_act, a, kDdpgActBufs);
    const int h = (threadIdx.x & 63) >> 5;
    const long long row0 = static_cast<long long>(blockIdx.x) * kDdpgTile;
    const int live = g.rows - row0 < kDdpgTile ? static_cast<int>(g.rows - row0) : kDdpgTile;
    ddpg_tile_rows(s.rowsrc, nullptr, row0, live, g.rows);
    __syncthreads();
    ddpg_load_obs(s.buf[0], g.obs, s.rowsrc, a.D, a.in_pad[0][0], a.obs_lo, a.obs_hi);
    if constexpr (RNG) {
        const int nb = (a.A + 3) >> 2;
        for (int i = threadIdx.x; i < live * nb; i += kDdpgBlock) {
            const int r = i / nb, b = i - r * nb;
            const float4 z = rng_normal4(n->seed_lo, n->seed_hi,
                                         n->row0 + static_cast<uint32_t>(row0 + r), n->t,
                                         static_cast<uint32_t>(b), kRngActionNoise);
            float *dst = s.sech2 + 4 * b * kDdpgLd + r;
            dst[0] = z.x;
            dst[kDdpgLd] = z.y;
            dst[2 * kDdpgLd] = z.z;
            dst[3 * kDdpgLd] = z.w;
        }
    }
    float *const xs[kDdpgLayers] = {s.buf[0], s.buf[1], s.buf[2]};
    ddpg_forward(a, 0, g.img, s.wbuf, xs, [&](const ddpg_f32x16 &acc, int col) {
        if (col >= a.A) return;
        const float sc = g.scale[col];
        float mean = 0.0f, sigma = 0.0f;
        if constexpr (RNG) {
            mean = n->mean[col];
            sigma = n->sigma[col];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = ddpg_acc_row(r, h);
            if (row < live) {
                const long long o = (row0 + row) * a.A + col;
                float d;
                float act = ddpg_tanh(acc[r], &d);
                if constexpr (RNG) {
#pragma clang fp contract(off)
                    const float z = s.sech2[col * kDdpgLd + row];
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
    });
}

__global__ __launch_bounds__(kDdpgBlock) void ddpg_act_kernel(const DdpgActArgs g) {
    ddpg_act_tile<false>(g, nullptr);
}

// the instance that forms its own noise
__global__ __launch_bounds__(kDdpgBlock) void ddpg_act_rng_kernel(const DdpgActArgs g,
                                                                  const DdpgActRng n) {
    ddpg_act_tile<true>(g, &n);
}

// The actor's action of network image `img` at the tile in obs_buf into the
// concat rows of c1, then that image's critic at (obs tile, that action); Q
// of tile row r into qrow[r].  `axs` / `cxs`: the two networks' layer inputs
// (axs[0] == cxs[0] == the obs tile, cxs[1] == c1).  `sech2` (or null): where
// 1 - a^2 goes, [A][33].  Ends with a barrier.
__device__ __forceinline__ void ddpg_actor_then_critic(const DdpgPlan &a, const float *img,
                                                       float *wbuf, float *const *axs,
                                                       float *const *cxs, float *qrow,
                                                       float *sech2) {
    const int h = (threadIdx.x & 63) >> 5;
    float *c1 = cxs[1];
    const int h0 = a.out_dim[1][0];
    ddpg_zero_concat_pad(a, c1);
    ddpg_forward(a, 0, img, wbuf, axs, [&](const ddpg_f32x16 &acc, int col) {
        if (col >= a.A) return;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = ddpg_acc_row(r, h);
            float d;
            c1[(h0 + col) * kDdpgLd + row] = ddpg_tanh(acc[r], &d);
            if (sech2) sech2[col * kDdpgLd + row] = d;
        }
    });
    ddpg_forward(a, 1, img, wbuf, cxs, [&](const ddpg_f32x16 &acc, int col) {
        if (col != 0) return;
#pragma unroll
        for (int r = 0; r < 16; ++r) qrow[ddpg_acc_row(r, h)] = acc[r];
    });
}

// --------------------------------------------------------------------- target
struct DdpgTargetArgs {
    DdpgPlan p;
    int n, m;
    float gamma;
    const float *timg;       // the target image
    const int32_t *idx;
    const float *obs1, *rewards;
    const uint8_t *dones;
    float *y;                // [n]
};

__global__ __launch_bounds__(kDdpgBlock) void ddpg_target_kernel(const DdpgTargetArgs g) {
    extern __shared__ __attribute__((aligned(16))) float ddpg_lds_target[];
    const DdpgPlan &a = g.p;
    const DdpgLds s = ddpg_lds(ddpg_lds_target, a, kDdpgBufs);
    const int tid = threadIdx.x;
    const long long row0 = static_cast<long long>(blockIdx.x) * kDdpgTile;
    const int live = g.n - row0 < kDdpgTile ? static_cast<int>(g.n - row0) : kDdpgTile;
    ddpg_tile_rows(s.rowsrc, g.idx, row0, live, g.m);
    __syncthreads();
    ddpg_load_obs(s.buf[0], g.obs1, s.rowsrc, a.D, a.in_pad[0][0], a.obs_lo, a.obs_hi);
    float *const axs[kDdpgLayers] = {s.buf[0], s.buf[1], s.buf[2]};
    float *const cxs[kDdpgLayers] = {s.buf[0], s.buf[3], s.buf[4]};
    ddpg_actor_then_critic(a, g.timg, s.wbuf, axs, cxs, s.rowf, nullptr);
    if (tid < live) {
        const int src = s.rowsrc[tid];
        const float nonterminal = 1.0f - (g.dones[src] != 0 ? 1.0f : 0.0f);
        g.y[row0 + tid] = g.rewards[src] + g.gamma * nonterminal * s.rowf[tid];
    }
}

// ------------------------------------------------------------------- gradient
struct DdpgGradArgs {
    DdpgPlan p;
    int n, m, tiles, grid;
    int n_total;             // the N of 1 / N: n, or every rank's rows together
    const float *img;        // the online image
    const int32_t *idx;
    const float *obs0, *actions;
    const float *y;          // [n], by position (ddpg_target_kernel's)
    float *slab;             // [grid][img_floats]
    double *stat_slab;       // [grid][2][kDdpgRowStats]
};

__global__ __launch_bounds__(kDdpgBlock) void ddpg_grad_kernel(const DdpgGradArgs g) {
    extern __shared__ __attribute__((aligned(16))) float ddpg_lds_grad[];
    const DdpgPlan &a = g.p;
    const DdpgLds s = ddpg_lds(ddpg_lds_grad, a, kDdpgBufs);
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 31, h = lane >> 5;
    const int branch = blockIdx.y;
    const int L = a.n_hidden, h0 = a.out_dim[1][0];
    const float inv_n = 1.0f / static_cast<float>(g.n_total);
    float *const axs[kDdpgLayers] = {s.buf[0], s.buf[1], s.buf[2]};
    float *const cxs[kDdpgLayers] = {s.buf[0], s.buf[3], s.buf[4]};
    float *c1 = s.buf[3], *dzh = s.buf[5];
    float *qrow = s.rowf, *yrow = s.rowf + kDdpgTile;

    ddpg_f32x16 dw[kDdpgLayers][2] = {};
    float db[kDdpgLayers] = {};
    double stat_acc = 0.0;        // thread t < kDdpgRowStats keeps statistic t

    for (int tile = blockIdx.x; tile < g.tiles; tile += g.grid) {
        const long long row0 = static_cast<long long>(tile) * kDdpgTile;
        const int live = g.n - row0 < kDdpgTile ? static_cast<int>(g.n - row0) : kDdpgTile;
        __syncthreads();       // the previous tile's last LDS readers are done
        ddpg_tile_rows(s.rowsrc, g.idx, row0, live, g.m);
        __syncthreads();
        ddpg_load_obs(s.buf[0], g.obs0, s.rowsrc, a.D, a.in_pad[0][0], a.obs_lo, a.obs_hi);

        if (branch == 0) {
            // ------------------------------------------------ the critic's loss
            ddpg_zero_concat_pad(a, c1);
            for (int i = tid; i < kDdpgTile * a.A; i += kDdpgBlock) {    // the stored action
                const int r = i / a.A, c = i - r * a.A;
                const int src = s.rowsrc[r];
                c1[(h0 + c) * kDdpgLd + r] =
                    src >= 0 ? g.actions[static_cast<long long>(src) * a.A + c] : 0.0f;
            }
            if (tid < kDdpgTile) yrow[tid] = tid < live ? g.y[row0 + tid] : 0.0f;
            ddpg_forward(a, 1, g.img, s.wbuf, cxs, [&](const ddpg_f32x16 &acc, int col) {
                if (col != 0) return;
#pragma unroll
                for (int r = 0; r < 16; ++r) qrow[ddpg_acc_row(r, h)] = acc[r];
            });
            // the head's dZ: column 0 carries 2 (Q - y) / N, the padding zeros
            for (int i = tid; i < a.out_pad[1][L] * kDdpgTile; i += kDdpgBlock) {
                const int c = i / kDdpgTile, r = i & (kDdpgTile - 1);
                dzh[c * kDdpgLd + r] = (c == 0 && r < live) ? 2.0f * (qrow[r] - yrow[r]) * inv_n : 0.0f;
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
            ddpg_backward<1>(a, g.img, s.wbuf, cxs, dzh, true, dw, db);
        } else {
            // ----------------------------- the actor's loss through the critic
            ddpg_actor_then_critic(a, g.img, s.wbuf, axs, cxs, qrow, s.sech2);
            // the critic's head dZ = -1 / N on the live rows
            for (int i = tid; i < a.out_pad[1][L] * kDdpgTile; i += kDdpgBlock) {
                const int c = i / kDdpgTile, r = i & (kDdpgTile - 1);
                dzh[c * kDdpgLd + r] = (c == 0 && r < live) ? -inv_n : 0.0f;
            }
            if (tid == 0) {
                double sum = 0.0;
                for (int r = 0; r < live; ++r) sum += qrow[r];
                stat_acc += sum;
            }
            __syncthreads();
            // the critic's backward to d / d action: no dW, masks from the
            // kept activations; the head's weights are still staged
            ddpg_f32x16 da = {};
#pragma unroll
            for (int l = kDdpgLayers - 1; l >= 1; --l) {
                if (l > L) continue;
                const int ip = a.in_pad[1][l], op = a.out_pad[1][l], ld = op + 1;
                const float *dz = l == L ? dzh : cxs[l + 1];
                if (l < L) {
                    ddpg_stage_w(s.wbuf, g.img + a.off_w[1][l], ip, op);
                    __syncthreads();
                }
                if (l == 1) {
                    // the concat layer: in-chunks h0, h0 + 32 are d / d action
                    const int n0 = h0 + wave * 32;
                    if (wave * 32 < a.out_pad[0][L]) da = ddpg_zwt(dz, s.wbuf, op, ld, n0);
                } else {
                    const int n0 = wave * 32;
                    float *x = cxs[l];
                    if (n0 < a.out_dim[1][l - 1]) {
                        const ddpg_f32x16 acc = ddpg_zwt(dz, s.wbuf, op, ld, n0);
                        float *col = x + (n0 + li) * kDdpgLd;
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int row = ddpg_acc_row(r, h);
                            col[row] = col[row] > 0.0f ? acc[r] : 0.0f;
                        }
                    }
                }
                __syncthreads();
            }
            // the actor's head dZ = d / d action o (1 - a^2), zero past A
            if (wave * 32 < a.out_pad[0][L]) {
                const int col = wave * 32 + li;
                const bool on = col < a.A;
                const float *sc = s.sech2 + (on ? col : 0) * kDdpgLd;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = ddpg_acc_row(r, h);
                    dzh[col * kDdpgLd + row] = on ? da[r] * sc[row] : 0.0f;
                }
            }
            __syncthreads();
            ddpg_backward<0>(a, g.img, s.wbuf, axs, dzh, false, dw, db);
        }
    }

    float *part = g.slab + static_cast<long long>(blockIdx.x) * a.img_floats;
    if (branch == 0)
        ddpg_store_partial<1>(a, part, dw, db);
    else
        ddpg_store_partial<0>(a, part, dw, db);
    if (tid < kDdpgRowStats)
        g.stat_slab[(static_cast<long long>(blockIdx.x) * 2 + branch) * kDdpgRowStats + tid] = stat_acc;
}

// --------------------------------------------------------------------- reduce
struct DdpgReduceArgs {
    DdpgPlan p;
    int grid;
    const float *slab;
    float *grad;             // [n_params]
};

__global__ __launch_bounds__(256) void ddpg_reduce_kernel(const DdpgReduceArgs q) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= q.p.n_params) return;
    const float *at = q.slab + ddpg_image_pos(q.p, p);
    double sum = 0.0;
    for (int gi = 0; gi < q.grid; ++gi) sum += at[static_cast<long long>(gi) * q.p.img_floats];
    q.grad[p] = static_cast<float>(sum);
}

__device__ __forceinline__ double ddpg_block_sum(double v, double *red) {
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    __syncthreads();
    for (int s = blockDim.x >> 1; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    return red[0];
}

// One workgroup: the statistics of n rows from `parts` statistic partials,
// `stat_stride` doubles apart (the G workgroups' of stat_slab, or the W ranks'
// inside their records), and the two blocks' squared gradient norms.
__global__ __launch_bounds__(256) void ddpg_stats_kernel(int n, int parts, int stat_stride,
                                                         int n_params, int n_actor,
                                                         const double *stat_parts,
                                                         const float *grad, float *stats) {
    __shared__ double red[256];
    __shared__ double sums[2 * kDdpgRowStats];
    const int tid = threadIdx.x;
    double sa = 0.0, sc = 0.0;
    for (int i = tid; i < n_params; i += 256) {
        const double gv = grad[i];
        if (i < n_actor)
            sa += gv * gv;
        else
            sc += gv * gv;
    }
    const double actor_sq = ddpg_block_sum(sa, red);
    const double critic_sq = ddpg_block_sum(sc, red);
    if (tid < 2 * kDdpgRowStats) {
        double t = 0.0;
        for (int gi = 0; gi < parts; ++gi) t += stat_parts[static_cast<long long>(gi) * stat_stride + tid];
        sums[tid] = t;
    }
    __syncthreads();
    if (tid == 0) {
        stats[0] = static_cast<float>(sums[0] / n);
        stats[1] = static_cast<float>(-sums[kDdpgRowStats] / n);
        stats[2] = static_cast<float>(sums[1] / n);
        stats[3] = static_cast<float>(sums[2] / n);
        stats[4] = 0.0f;
        stats[5] = 0.0f;
        stats[6] = static_cast<float>(critic_sq);
        stats[7] = static_cast<float>(actor_sq);
    }
}

// ------------------------------------------------------ the gradient exchange
// W ranks, rank r with n_r rows, take the single agent's step on all N = sum
// n_r rows: each runs [target, gradient with 1 / N, partial] into slot r of a
// [W][record] buffer, the caller all-gathers the buffer in place, and each
// runs [combine, statistics, update].  One rank's record, float64:
//   [ n_params sums | 2 * kDdpgRowStats statistic sums | n_r | zeros ]
// padded to a multiple of 256 B.  Every rank adds the same float64 values in
// rank order, so every rank gets the same bits; at W = 1 they are the bits of
// [gradient, reduce, statistics] (0.0 + x is x, and the one rounding to
// float32 is the reduce kernel's).
__host__ __device__ constexpr int ddpg_record_doubles(int n_params) {
    return (n_params + 2 * kDdpgRowStats + 1 + 31) / 32 * 32;
}

struct DdpgPartialArgs {
    DdpgPlan p;
    int grid, n;             // this rank's workgroups per branch and rows
    const float *slab;
    const double *stat_slab;
    double *record;          // [ddpg_record_doubles(n_params)]
};

// The reduce kernel's grid and sum, left unrounded.  Block 0 also folds the
// statistic sums over the G workgroups (the statistics kernel's loop) and
// writes the row count and the padding.
__global__ __launch_bounds__(256) void ddpg_partial_kernel(const DdpgPartialArgs q) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < q.p.n_params) {
        const float *at = q.slab + ddpg_image_pos(q.p, p);
        double sum = 0.0;
        for (int gi = 0; gi < q.grid; ++gi) sum += at[static_cast<long long>(gi) * q.p.img_floats];
        q.record[p] = sum;
    }
    if (blockIdx.x == 0) {
        const int tid = threadIdx.x;
        if (tid < 2 * kDdpgRowStats) {
            double t = 0.0;
            for (int gi = 0; gi < q.grid; ++gi)
                t += q.stat_slab[static_cast<long long>(gi) * 2 * kDdpgRowStats + tid];
            q.record[q.p.n_params + tid] = t;
        } else if (tid < ddpg_record_doubles(q.p.n_params) - q.p.n_params) {
            // the row count, then zeros to the record's padded end (at most
            // 2 * kDdpgRowStats + 1 + 31 entries: one block covers them)
            q.record[q.p.n_params + tid] = tid == 2 * kDdpgRowStats ? static_cast<double>(q.n) : 0.0;
        }
    }
}

struct DdpgCombineArgs {
    int n_params, world, record_doubles;
    const double *records;   // [world][record_doubles]
    float *grad;             // [n_params]
};

// grad[p] = the W records' values of parameter p added in rank order in
// float64, rounded once.  The statistics kernel takes its norms from grad.
__global__ __launch_bounds__(256) void ddpg_combine_kernel(const DdpgCombineArgs q) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= q.n_params) return;
    double sum = 0.0;
    for (int r = 0; r < q.world; ++r)
        sum += q.records[static_cast<long long>(r) * q.record_doubles + p];
    q.grad[p] = static_cast<float>(sum);
}

// --------------------------------------- Adam x2, soft update, both images
struct DdpgUpdateArgs {
    DdpgPlan p;
    float lr_t_actor, lr_t_critic;       // the bias correction folded in
    float beta1, beta2, omb1, omb2, eps;
    float tau, omt;                      // tau and 1 - tau, each rounded once
    const float *grad;
    float *params, *target, *m, *v;
    float *img, *timg;
};

// (1 - tau) target + tau params: two multiplies and one add, never contracted
// into a fused multiply-add, so a float32 NumPy run of the statement gives the
// same bits
__device__ __forceinline__ float ddpg_soft_update(float omt, float target, float tau, float param) {
#pragma clang fp contract(off)
    const float keep = omt * target, take = tau * param;
    return keep + take;
}

__global__ __launch_bounds__(256) void ddpg_update_kernel(const DdpgUpdateArgs u) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= u.p.n_params) return;
    const float gi = u.grad[i];
    const float mi = u.beta1 * u.m[i] + u.omb1 * gi;
    const float vi = u.beta2 * u.v[i] + u.omb2 * gi * gi;
    u.m[i] = mi;
    u.v[i] = vi;
    const float lr_t = i < u.p.n_actor ? u.lr_t_actor : u.lr_t_critic;
    const float pi = u.params[i] - lr_t * mi / (sqrtf(vi) + u.eps);
    u.params[i] = pi;
    const float ti = ddpg_soft_update(u.omt, u.target[i], u.tau, pi);
    u.target[i] = ti;
    const int at = ddpg_image_pos(u.p, i);
    u.img[at] = pi;
    u.timg[at] = ti;
}

// set_params: flat into the parameters, the targets and both images
// (params null: into the targets and their image alone)
__global__ __launch_bounds__(256) void ddpg_pack_kernel(const DdpgPlan p, const float *flat,
                                                        float *params, float *target, float *img,
                                                        float *timg) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n_params) return;
    const float v = flat[i];
    const int at = ddpg_image_pos(p, i);
    if (params) {
        params[i] = v;
        img[at] = v;
    }
    target[i] = v;
    timg[at] = v;
}

}  // namespace ce
