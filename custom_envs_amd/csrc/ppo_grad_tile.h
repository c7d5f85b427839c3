// The loss-gradient tile machinery the learners share (gfx950): the forward
// and backward of the two tanh MLPs of policy_kernels.h over 32-row tiles, dW
// on v_mfma_f32_32x32x2_f32, partials kept on chip.  ppo2_kernels.h and
// a2c_kernels.h instantiate ppo_grad_tiles with their own argument struct,
// which carries the loss head and the row source as inlined members:
//
//   action_row(s, A)            row s's stored action, [A] floats
//   vf_row(s, v, inv_n, stat)   value head of source row s: its statistic(s)
//                               into stat[j * kPpoTile], returns dZ
//   pi_row(s, nlp, inv_n, stat) policy head of source row s from its neglogp
//                               (float64): statistics, returns the row weight
//                               w = d loss / d neglogp
//
// and the fields p, n, n_total, m, tiles, grid, img_floats, w_floats,
// act_floats, idx, obs, slab, stat_slab as Ppo2GradArgs names them.  n bounds
// the live rows; n_total is the N of the loss's mean, 1 / N the row weight: n
// itself for a learner alone, the ranks' rows together under a gradient
// exchange (learner_host.h).
//
// Grid (G, 2) x 256 threads, G = min(tiles, limit).  blockIdx.y picks the
// network as in policy_mlp_kernel; workgroup x walks the 32-row tiles x,
// x + G, ... and keeps every layer's dW (MFMA accumulators), db, dlogstd and
// the loss-statistic sums on chip across its tiles; they leave the workgroup
// once, as partial x of the slab ppo2_reduce_kernel sums.
//
// Per tile (float32 on v_mfma_f32_32x32x2_f32, operands as in the forward):
//   forward   X_{l+1} = tanh(X_l W_l + b_l), every X_l kept in LDS k-major
//             ([width][33], hidden ones in complement form, see ppo_tanh_comp); W_l staged in LDS as [in][out + 1] (the odd row
//             stride makes both W[k][n0 + lane] and W[n0 + lane][k] reads
//             conflict free: the forward and the dX product share one stage)
//   head      pi: z = (a - mean) / std into the head buffer; 8 threads per row
//             fold sum z^2, one thread per row forms neglogp and, through
//             pi_row, the row weight w; then dZ = -w z / std in place and
//             dlogstd += sum_rows w (1 - z^2).   vf: dZ[row][0] from vf_row.
//             Rows past N get w = 0: exact zeros below.
//   backward  per layer, top down:  dW_l += X_l^T dZ_l  (the 32 rows are the
//             MFMA's K; block b = wave + 4 j of the [in / 32][out / 32] grid),
//             db_l += sum_rows dZ_l, dX = dZ_l W_l^T, and dZ_{l-1} = dX o
//             (1 - X_l^2) written over X_l: the backward pass has finished
//             with X_l once dW_l is done, so no second dZ buffer exists.
//
// Accuracy: the first layer's pre-activation is float64 on the vector units
// and the policy head's mean a float64 sum of single-MFMA (two-term) float32
// products.  A float32 chain rounds at the size of its partial sums and
// products: with |obs| in the hundreds a unit of a saturated row that happens
// to land near zero has its tanh' off by 2e-5, which that row's large obs
// multiplies into dW_0 (1e-5 of the largest gradient entry, the float32 NumPy
// statement's own error); and a 1e-6 error of the mean is 1e-5 of the ratio
// at 64 actions.  Sum z^2 and neglogp are float64 for the same reason.
//
// LDS at the limits (D = 128, hidden 3 x 128, A = 64): weight stage 128 x 129,
// four activation buffers 128 x 33, head buffer 64 x 33, row scalars:
// 35 712 floats = 142 848 B of the CU's 160 KiB.
//
// No floating-point atomics: the same inputs with the same G give the same
// bits.  Different G regroup the float32 per-workgroup sums.
//
// ppo_grad_wide_tile.h walks the same steps in chunks for wide shapes.  The
// four kernels are register-saturated, and a step is a shared function ("the
// tile parts" below) only where calling it leaves all four kernels' device
// assembly the text it was with the step inline; every other step both
// bodies have stays inline in both, and a fix to it belongs in both.  Which
// steps those are, and what was tried: DESIGN.md 3.24, "One text where the
// code objects allow it".
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "policy_engine.h"

namespace ce {

// the forward's tile shape and MFMA register layout (policy_kernels.h)
constexpr int kPpoBlock = 256;      // 4 waves
constexpr int kPpoTile = 32;        // rows per tile (the MFMA's M)
constexpr int kPpoLd = 33;          // LDS words per activation column
constexpr int kPpoMaxA = 64;        // widest head
typedef float ppo_f32x16 __attribute__((ext_vector_type(16)));
__device__ __forceinline__ int ppo_acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

constexpr int kPpoStats = 8;        // loss, pg, vf, entropy, approxkl, clipfrac, |grad|^2, spare
constexpr int kPpoRowStats = 4;     // per-row sums a workgroup keeps (pi: pg, kl, clipped; vf: vf)
constexpr int kPpoStatBlock = 1024;
// LDS floats of a gradient kernel, as both bodies carve it: the weight stage,
// n_hidden + 1 activation buffers, the head buffer [head_cols][33], the row
// weights, row statistics and source rows
__host__ __device__ constexpr int ppo_lds_floats(int w_floats, int act_floats, int n_hidden,
                                                 int head_cols) {
    return w_floats + (n_hidden + 1) * act_floats + head_cols * kPpoLd +
           (kPpoRowStats + 2) * kPpoTile;
}
// at the shape limits (D = 128, 3 x 128 hidden, A = 64)
constexpr int kPpoMaxLdsBytes = ppo_lds_floats(128 * 129, 128 * kPpoLd, 3, kPpoMaxA) * 4;
static_assert(kPpoMaxLdsBytes == 142848, "the header comment's LDS budget");
constexpr float kPpoLog2PiE = 2.8378770664093453f;   // log(2 pi) + 1

__device__ __forceinline__ int ppo_src_row(const int32_t *idx, long long i, int m) {
    if (!idx) return static_cast<int>(i);
    const int s = idx[i];
    return s < 0 ? 0 : (s >= m ? m - 1 : s);     // never read out of bounds
}

__device__ __forceinline__ double ppo_block_sum(double v, double *red) {
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

// Hidden activations are kept in complement form u = sign(z) (1 - |tanh z|):
// y = sign(u) (1 - |u|) to float32 rounding, and the derivative 1 - y^2 =
// |u| (2 - |u|) keeps its relative accuracy where tanh saturates (1 - y^2 from
// a rounded y is off by up to 1.2e-7 absolute there, which a large input row
// multiplies into dW_0).
__device__ __forceinline__ float ppo_tanh_comp(float z) {
    const float e = expf(-2.0f * fabsf(z));
    return copysignf(2.0f * e / (1.0f + e), z);
}
__device__ __forceinline__ float ppo_act(float u) { return copysignf(1.0f - fabsf(u), u); }

// ------------------------------------------------------------ the tile parts
// What ppo_grad_tiles and ppo_grad_wide_tiles both call.  li = tid & 31,
// h = (tid & 63) >> 5; element r of an MFMA accumulator is row
// ppo_acc_row(r, h), column li of its 32 x 32 block.

// The two weight stagers: a whole contiguous [ip][op] layer to [ip][op + 1],
// and rows x cw floats out of a wider matrix (row stride src_ld; cw, src_ld
// and the offset multiples of 4) to [rows][cw + 1].  The second does the
// first's job at src_ld = op, through other index arithmetic and so other code
// in the narrow kernels: they keep the first.
__device__ __forceinline__ void ppo_stage_w(float *wbuf, const float *img, int ip, int op) {
    const float4 *src = reinterpret_cast<const float4 *>(img);
    const int n4 = ip * op / 4, ld = op + 1;
    for (int i = threadIdx.x; i < n4; i += kPpoBlock) {
        const float4 v = src[i];
        const int r = (4 * i) / op, c = 4 * i - r * op;
        float *d = wbuf + r * ld + c;
        d[0] = v.x;
        d[1] = v.y;
        d[2] = v.z;
        d[3] = v.w;
    }
}
__device__ __forceinline__ void ppo_wide_stage_w(float *wbuf, const float *src, int rows, int cw,
                                                 int src_ld) {
    const int c4 = cw >> 2, n4 = rows * c4, ld = cw + 1;
    for (int i = threadIdx.x; i < n4; i += kPpoBlock) {
        const int r = i / c4, c = 4 * (i - r * c4);
        const float4 v = *reinterpret_cast<const float4 *>(src + static_cast<long long>(r) * src_ld + c);
        float *d = wbuf + r * ld + c;
        d[0] = v.x;
        d[1] = v.y;
        d[2] = v.z;
        d[3] = v.w;
    }
}

// The policy head's row weight.  8 threads per row (thread tid: row tid >> 3)
// come with their share `sum` of the row's sum z^2: the shares are folded, the
// row's first thread forms neglogp (float64, see the header comment) and,
// through pi_row, the weight w into wrow: 0 past the last row.
template <class Args>
__device__ __forceinline__ void ppo_row_weight(const Args &g, const int *rowsrc, float *rowstat,
                                               float *wrow, double sum, double sum_logstd,
                                               float inv_n) {
    const PolicyPlan &a = g.p;
    const int tid = threadIdx.x, r = tid >> 3, part = tid & 7;
    sum += __shfl_xor(sum, 1);
    sum += __shfl_xor(sum, 2);
    sum += __shfl_xor(sum, 4);
    const int src = rowsrc[r];
    if (part == 0) {
        float w = 0.0f;
        if (src >= 0) {
            const double nlp = 0.5 * sum + sum_logstd + 0.5 * a.A * 1.8378770664093453;
            w = g.pi_row(src, nlp, inv_n, rowstat + r);
        }
        wrow[r] = w;
    }
}

// The backward.  One 32 x 32 block of dW += X^T dZ over the tile's 32 rows
// (the MFMA's K) on the accumulator c: xa = X + the lane's row of the block *
// 33 + h (valid: that row exists), zb = dZ + the lane's column * 33 + h; comp:
// X is in complement form.
__device__ __forceinline__ ppo_f32x16 ppo_dw_mfma(ppo_f32x16 c, const float *xa, const float *zb,
                                                  bool valid, bool comp) {
#pragma unroll
    for (int k = 0; k < kPpoTile; k += 2) {
        float xv = valid ? xa[k] : 0.0f;
        if (comp) xv = ppo_act(xv);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(xv, zb[k], c, 0, 0, 0);
    }
    return c;
}
// db's share of the tile: one dZ column summed over the rows
__device__ __forceinline__ float ppo_col_sum(const float *col) {
    float sum = 0.0f;
    for (int r = 0; r < kPpoTile; ++r) sum += col[r];
    return sum;
}
// dX = dZ W^T for one wave's 32 input units, continued on acc over cw staged
// columns: za = dZ + h * 33 + li, wb = W + the lane's unit * ld + h
__device__ __forceinline__ ppo_f32x16 ppo_dx_mfma(ppo_f32x16 acc, const float *za, const float *wb,
                                                  int cw) {
    for (int k = 0; k < cw; k += 2)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(za[k * kPpoLd], wb[k], acc, 0, 0, 0);
    return acc;
}

// the workgroup's statistic sums, held by threads 128 .. 131, to stat_slab
template <class Args>
__device__ __forceinline__ void ppo_store_stats(const Args &g, double stat_acc) {
    const int tid = threadIdx.x, net = blockIdx.y;
    if (tid >= 128 && tid < 128 + kPpoRowStats)
        g.stat_slab[(static_cast<long long>(blockIdx.x) * 2 + net) * kPpoRowStats + tid - 128] = stat_acc;
}

// --------------------------------------------------------- the narrow body
// The whole gradient kernel but its __global__ line (see the header comment).
template <class Args>
__device__ __forceinline__ void ppo_grad_tiles(const Args &g) {
    extern __shared__ float ppo_lds[];
    const PolicyPlan &a = g.p;
    float *wbuf = ppo_lds;
    float *xbase = wbuf + g.w_floats;                       // X_0 .. X_{n_hidden}
    float *dzh = xbase + (a.n_hidden + 1) * g.act_floats;   // the head's z, then dZ
    float *wrow = dzh + kPpoMaxA * kPpoLd;                  // [32] row weights
    float *rowstat = wrow + kPpoTile;                       // [kPpoRowStats][32]
    int *rowsrc = reinterpret_cast<int *>(rowstat + kPpoRowStats * kPpoTile);   // [32]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 31, h = lane >> 5;
    const int net = blockIdx.y;
    const int L = a.n_hidden;
    const float inv_n = 1.0f / static_cast<float>(g.n_total);

    ppo_f32x16 dw[kPlanLayers][4] = {};
    float db[kPlanLayers] = {};
    float dls = 0.0f;
    double stat_acc = 0.0;

    double sum_logstd = 0.0;
    for (int c = 0; c < a.A; ++c) sum_logstd += a.img[a.off_logstd + c];

    // std of this lane's head column, in float64: a relative error in it is a
    // common relative error of every z of the column
    double sd_d = 1.0;
    if (net == 0 && wave * 32 + li < a.A) sd_d = exp(static_cast<double>(a.img[a.off_logstd + wave * 32 + li]));

    for (int tile = blockIdx.x; tile < g.tiles; tile += g.grid) {
        const long long row0 = static_cast<long long>(tile) * kPpoTile;
        const int live = g.n - row0 < kPpoTile ? static_cast<int>(g.n - row0) : kPpoTile;
        __syncthreads();       // the previous tile's last LDS readers are done
        if (tid < kPpoTile) rowsrc[tid] = tid < live ? ppo_src_row(g.idx, row0 + tid, g.m) : -1;
        if (tid < kPpoRowStats * kPpoTile) rowstat[tid] = 0.0f;
        __syncthreads();
        {   // the observation tile, k-major, zero past D and past the last row
            const int dp = a.in_pad[0];
            for (int i = tid; i < kPpoTile * dp; i += kPpoBlock) {
                const int r = i / dp, k = i - r * dp;
                const int s = rowsrc[r];
                xbase[k * kPpoLd + r] =
                    (s >= 0 && k < a.D) ? g.obs[static_cast<long long>(s) * a.D + k] : 0.0f;
            }
        }

        // ------------------------------------------------------------ forward
        for (int l = 0; l <= L; ++l) {
            const int ip = a.in_pad[l], op = a.out_pad[net][l], ld = op + 1;
            const float *cur = xbase + l * g.act_floats;
            ppo_stage_w(wbuf, a.img + a.off_w[net][l], ip, op);
            __syncthreads();
            const int n0 = wave * 32;
            if (l == 0) {
                // The first layer in float64 on the vector units (see the header
                // comment): thread t owns row t & 31 and units t >> 5, + 8, ...
                const int row = tid & 31, cg = tid >> 5;
                double acc0[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) acc0[j] = 0.0;
                const float *xr = cur + row;
                for (int k = 0; k < ip; ++k) {
                    const double x = xr[k * kPpoLd];
                    const float *wr = wbuf + k * ld + cg;
#pragma unroll
                    for (int j = 0; j < 16; ++j)
                        if (8 * j < op) acc0[j] = fma(x, static_cast<double>(wr[8 * j]), acc0[j]);
                }
                float *nxt = xbase + g.act_floats;
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    if (8 * j < op) {
                        const int col = cg + 8 * j;
                        nxt[col * kPpoLd + row] = ppo_tanh_comp(
                            static_cast<float>(acc0[j] + a.img[a.off_b[net][0] + col]));
                    }
            } else if (n0 < op) {   // wave-uniform
                const float *xa = cur + h * kPpoLd + li;
                const float *wb = wbuf + h * ld + n0 + li;
                const int col = n0 + li;
                const float bias = a.img[a.off_b[net][l] + col];
                ppo_f32x16 pre;      // the pre-activation, bias included
                if (l == L && net == 0) {
                    // float64 sums of single-MFMA products (see the header comment)
                    double accd[16];
#pragma unroll
                    for (int r = 0; r < 16; ++r) accd[r] = 0.0;
                    for (int k = 0; k < ip; k += 2) {
                        const float xv = ppo_act(xa[k * kPpoLd]);
                        const ppo_f32x16 zero = {};
                        const ppo_f32x16 c =
                            __builtin_amdgcn_mfma_f32_32x32x2f32(xv, wb[k * ld], zero, 0, 0, 0);
#pragma unroll
                        for (int r = 0; r < 16; ++r) accd[r] += c[r];
                    }
                    if (l == L) {      // always: dropping the test moves the kernels' code
                        // the policy head: z = (action - mean) / std, zero past A
                        // and past the last row
                        const bool on = col < a.A;
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int row = ppo_acc_row(r, h);
                            const int s = rowsrc[row];
                            float z = 0.0f;
                            if (on && s >= 0)
                                z = static_cast<float>(
                                    (g.action_row(s, a.A)[col] - (accd[r] + bias)) / sd_d);
                            dzh[col * kPpoLd + row] = z;
                        }
                    } else {
#pragma unroll
                        for (int r = 0; r < 16; ++r) pre[r] = static_cast<float>(accd[r] + bias);
                    }
                } else {
                    ppo_f32x16 acc = {};
                    for (int k = 0; k < ip; k += 2)
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ppo_act(xa[k * kPpoLd]), wb[k * ld],
                                                                   acc, 0, 0, 0);
#pragma unroll
                    for (int r = 0; r < 16; ++r) pre[r] = acc[r] + bias;
                }
                if (l < L) {
                    float *nxt = xbase + (l + 1) * g.act_floats;
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        nxt[col * kPpoLd + ppo_acc_row(r, h)] = ppo_tanh_comp(pre[r]);
                } else if (net == 1) {
                    // the value head: column 0 carries dZ, the padding zeros
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = ppo_acc_row(r, h);
                        const int s = rowsrc[row];
                        float dz = 0.0f;
                        if (col == 0 && s >= 0) dz = g.vf_row(s, pre[r], inv_n, rowstat + row);
                        dzh[col * kPpoLd + row] = dz;
                    }
                }
            }
            __syncthreads();
        }

        // ------------------------------------------------- the policy's head
        if (net == 0) {
            {   // 8 threads per row fold sum z^2; one forms the row's weight
                const int r = tid >> 3, part = tid & 7;
                double s = 0.0;      // sum z^2 reaches 64: float32 would round at 8e-6
                for (int c = part; c < a.A; c += 8) {
                    const double z = dzh[c * kPpoLd + r];
                    s += z * z;
                }
                ppo_row_weight(g, rowsrc, rowstat, wrow, s, sum_logstd, inv_n);
            }
            __syncthreads();
            // dZ = -w z / std over z, column by column; dlogstd on the way
            if (tid < a.out_pad[0][L]) {
                const bool on = tid < a.A;
                const float inv_sd = on ? expf(-a.img[a.off_logstd + tid]) : 0.0f;
                float *col = dzh + tid * kPpoLd;
                float s = 0.0f;
                for (int r = 0; r < kPpoTile; ++r) {
                    const float z = col[r], w = wrow[r];
                    s += w * (1.0f - z * z);
                    col[r] = -w * z * inv_sd;
                }
                if (on) dls += s;
            }
        }
        // the tile's statistic sums, rows in order, one thread per statistic
        if (tid >= 128 && tid < 128 + kPpoRowStats) {
            const float *rs = rowstat + (tid - 128) * kPpoTile;
            double s = 0.0;
            for (int r = 0; r < kPpoTile; ++r) s += rs[r];
            stat_acc += s;
        }
        __syncthreads();

        // ----------------------------------------------------------- backward
#pragma unroll
        for (int l = kPlanLayers - 1; l >= 0; --l) {
            if (l > L) continue;
            const int ip = a.in_pad[l], op = a.out_pad[net][l], ld = op + 1;
            float *x = xbase + l * g.act_floats;
            const float *dz = l == L ? dzh : xbase + (l + 1) * g.act_floats;
            // the head's weights are still staged from the forward
            if (l < L && l > 0) ppo_stage_w(wbuf, a.img + a.off_w[net][l], ip, op);
            // dW_l += X_l^T dZ_l
            const int nni = op >> 5, nb = ((ip + 31) >> 5) * nni;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int b = wave + 4 * j;
                if (b < nb) {   // wave-uniform
                    const int mi = b / nni, ni = b - mi * nni;
                    const int mrow = mi * 32 + li;
                    const bool valid = mrow < ip;      // l > 0: ip is a hidden width, all valid
                    dw[l][j] = ppo_dw_mfma(dw[l][j], x + (valid ? mrow : 0) * kPpoLd + h,
                                           dz + (ni * 32 + li) * kPpoLd + h, valid, l > 0);
                }
            }
            if (tid < op) db[l] += ppo_col_sum(dz + tid * kPpoLd);
            if (l > 0) {
                __syncthreads();      // W_l staged
                const int n0 = wave * 32;
                ppo_f32x16 acc = {};
                if (n0 < ip)          // dX = dZ_l W_l^T, in-chunk n0 (ip is a hidden width here)
                    acc = ppo_dx_mfma(acc, dz + h * kPpoLd + li, wbuf + (n0 + li) * ld + h, op);
                __syncthreads();      // every dW_l read of X_l is done
                if (n0 < ip) {
                    float *col = x + (n0 + li) * kPpoLd;
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = ppo_acc_row(r, h);
                        const float u = fabsf(col[row]);
                        col[row] = acc[r] * (u * (2.0f - u));      // 1 - y^2 = u (2 - u)
                    }
                }
                __syncthreads();
            }
        }
    }

    // ---------------------------------------------- this workgroup's partial
    float *part = g.slab + static_cast<long long>(blockIdx.x) * g.img_floats;
#pragma unroll
    for (int l = 0; l < kPlanLayers; ++l) {
        if (l > L) continue;
        const int ip = a.in_pad[l], op = a.out_pad[net][l];
        const int nni = op >> 5, nb = ((ip + 31) >> 5) * nni;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int b = wave + 4 * j;
            if (b < nb) {
                const int mi = b / nni, ni = b - mi * nni;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = mi * 32 + ppo_acc_row(r, h);
                    if (row < ip) part[a.off_w[net][l] + row * op + ni * 32 + li] = dw[l][j][r];
                }
            }
        }
        if (tid < op) part[a.off_b[net][l] + tid] = db[l];
    }
    if (net == 0 && tid < a.A) part[a.off_logstd + tid] = dls;
    ppo_store_stats(g, stat_acc);
}

// -------------------------------------------------------------------- reduce
// grad[p] = sum over the G partials, in order, in float64, of the image
// element flat parameter p packs to (the entropy term's -ent_coef on logstd);
// sq[block] = this block's sum of grad^2.  ppo2_reduce_kernel (ppo2_kernels.h)
// serves both learners; ppo2_launch_reduce (ppo2_engine.hip) enqueues it.
struct Ppo2ReduceArgs {
    PolicyPlan p;
    int grid;
    float ent_coef;
    const float *slab;
    float *grad;
    double *sq;      // [ceil(n_params / 256)]
};
void ppo2_launch_reduce(const Ppo2ReduceArgs &q, hipStream_t stream);

// ------------------------------------------------- the gradient exchange
// One rank's record, what crosses GPUs (learner_host.h has the launch lists):
//   [n_params f64 | 2 kPpoRowStats f64 | n_r as f64], padded to 256 B
// the per-parameter float64 sums over the G partials in flat parameter order,
// before the reduce kernel's rounding and without its -ent_coef; the statistic
// sums of stat_slab over G; the rows of this rank.
constexpr int kPpoRecordTail = 2 * kPpoRowStats + 1;
__host__ __device__ constexpr int ppo_record_doubles(int n_params) {
    return (n_params + kPpoRecordTail + 31) / 32 * 32;
}

// ppo2_partial_kernel: ppo2_reduce_kernel's sum, unrounded, into `record`.
struct Ppo2PartialArgs {
    PolicyPlan p;
    int grid, n;
    const float *slab;
    const double *stat_slab;
    double *record;  // [ppo_record_doubles(n_params)]
};
void ppo2_launch_partial(const Ppo2PartialArgs &q, hipStream_t stream);

// ppo2_combine_kernel: grad[p] = the `world` records' values added in rank
// order in float64 (-ent_coef on logstd), rounded once; sq as the reduce
// kernel's.  At world 1 these are the reduce kernel's bits.
struct Ppo2CombineArgs {
    int n_params, off_logstd_flat, world, record_doubles;
    float ent_coef;
    const double *records;   // [world][record_doubles]
    float *grad;
    double *sq;
};
void ppo2_launch_combine(const Ppo2CombineArgs &q, hipStream_t stream);

// What a finish kernel reads: `grid` statistic partials, stat_stride doubles
// apart (the workgroups' of stat_slab, or the ranks' inside their records),
// and the |grad|^2 blocks.
struct Ppo2FinishArgs {
    int n, grid, n_sq, A, off_logstd, stat_stride;
    float ent_coef, vf_coef;
    const float *img;
    const double *stat_slab, *sq;
    float *stats;    // [kPpoStats]
};

}  // namespace ce
