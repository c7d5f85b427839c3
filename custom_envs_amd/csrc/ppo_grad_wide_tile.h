// ppo_grad_tiles (ppo_grad_tile.h) for observations up to 1024 wide and policy
// heads up to 512 wide (gfx950): the loss gradient of the reference's default
// Optimize shape, 981 -> hidden -> 490.  ppo2_kernels.h and a2c_kernels.h
// instantiate ppo_grad_wide_tiles with the argument structs of the narrow
// kernels; the contract is the narrow body's: grid (G, 2) x 256 threads,
// blockIdx.y the network, workgroup x on the 32-row tiles x, x + G, ..., the
// same Args members, the same slab [G][img_floats] and stat_slab, no
// floating-point atomics.  The reduce, finish, optimiser, pack, partial and
// combine kernels serve both bodies.
//
// What a layer wider than the 128 x 129 weight stage needs:
//
//   first layer, forward   the observation is walked in K-chunks of 128
//       columns.  Each chunk stages its slice of the gathered obs tile
//       (k-major, [128][33]) and rows k0 .. k0 + 127 of W0 (contiguous in the
//       image); each thread's float64 acc0[] runs on across the chunks in
//       ascending k.
//   policy head, forward   the columns are walked in N-chunks of 128
//       (policy_wide_kernel's chunks).  Two passes, so that only one chunk of
//       z is ever in LDS:
//         pass 1  per chunk: stage W[:, c0 .. c0 + 127], z = (a - mean) / std
//                 into the chunk buffer, every row's 8 threads add their
//                 columns' z^2 (float64) and carry the sum to the next chunk;
//                 z is dropped.  Then neglogp and the row weight w.
//         pass 2  per chunk: the stage and z again (the same instructions on
//                 the same operands: the same bits), dZ = -w z / std in
//                 place, dlogstd, db, dW, and the chunk's share of the
//                 dX = dZ W^T chain: one accumulator chain over ascending
//                 columns across the chunks.
//       A head of one chunk keeps its stage and its z between the passes.
//   dW of the first layer and of the head layer   up to 128 and 64 32 x 32
//       blocks: they do not fit the accumulators across tiles.  The workgroup
//       accumulates them in its OWN slab partial in global memory: per tile
//       and chunk the wave that owns a block loads it as the MFMA's C operand,
//       runs the 16 MFMAs over the tile's 32 rows and stores it back.  Block
//       -> wave -> lane is fixed, so a lane reads back only addresses it wrote
//       itself: program order suffices, no fence, no atomic.  The workgroup's
//       first tile starts from zero without reading, so a partial never shows
//       what an earlier call left in the slab.  The head's db and dlogstd go
//       the same way (a thread owns columns tid, tid + 128, ...).  The value
//       head is a head layer and takes the same path (4 blocks).
//   dW of hidden-to-hidden layers (at most 2 x 16 blocks), every other db and
//       the statistic sums stay on chip across the tiles as in the narrow
//       body and leave the workgroup once.
//   first layer, backward  dW0 = X0^T dZ0 walks the K-chunks again: the obs
//       chunk is gathered a second time (dZ0 stands in X1's buffer).
//
// Accumulation order: every dot product and every per-column sum has the
// narrow body's operands in the narrow body's order -- acc0 over ascending k,
// the mean a float64 sum of single-MFMA products over ascending k, sum z^2 by
// 8 threads per row over columns part, part + 8, ... (a chunk starts at a
// multiple of 8), the dX chain over ascending columns, a dW block's float32
// additions tile after tile whether its C operand waits in a register or in
// the slab.  At a shape the narrow body takes, there is one chunk each way and
// the slab and stat_slab hold the narrow body's bits at the same G, but for
// dlogstd's last place: how the compiler contracts s += w (1 - z^2) over the
// unrolled rows is not a property of the source.
//
// LDS (floats): weight stage min(in, 128) x (min(out, 128) + 1) at most
// 128 x 129; n_hidden + 1 activation buffers [<= 128][33] (the first takes
// the obs chunks); one head chunk of z / dZ [128][33]; row scalars 6 x 32.
//   981 -> 64 -> 64 -> 490: 16 512 + 3 x 4 224 + 4 224 + 192 = 33 600 floats
//                           = 134 400 B
//   the limits (1024 -> 3 x 128 -> 512): 16 512 + 4 x 4 224 + 4 224 + 192
//                           = 37 824 floats = 151 296 B of the CU's 160 KiB
//
// The row weight, a dW block's MFMAs, the hidden and first layers' db sums, the
// hidden layers' dX chain and the statistic store are the tile parts of
// ppo_grad_tile.h.  The other steps the narrow body has too are written here
// again, and a fix to one belongs in both: see that file's header comment.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "policy_engine.h"
#include "ppo_grad_tile.h"

namespace ce {

constexpr int kPpoWideMaxD = kPlanWideMaxD;     // observation width: a wide handle's limit
constexpr int kPpoWideMaxA = kPlanWideMaxA;     // action width
constexpr int kPpoWideChunk = 128;     // K-chunk of the first layer, N-chunk of the head
// LDS of a wide gradient kernel at the shape limits
constexpr int kPpoWideMaxLdsBytes = ppo_lds_floats(128 * 129, 128 * kPpoLd, 3, kPpoWideChunk) * 4;
static_assert(kPpoWideMaxLdsBytes == 151296, "the header comment's LDS budget");

// columns k0 .. k0 + kc - 1 of the gathered observation tile, k-major, zero
// past D and past the last row
__device__ __forceinline__ void ppo_wide_stage_obs(float *x, const float *obs, const int *rowsrc,
                                                   int D, int k0, int kc) {
#pragma unroll 4
    for (int j = 0; j < kPpoTile * kPpoWideChunk / kPpoBlock; ++j) {
        const int i = threadIdx.x + j * kPpoBlock;
        const int k = i & (kPpoWideChunk - 1), r = i >> 7;
        if (k < kc) {
            const int s = rowsrc[r];
            x[k * kPpoLd + r] =
                (s >= 0 && k0 + k < D) ? obs[static_cast<long long>(s) * D + k0 + k] : 0.0f;
        }
    }
}

// ppo_dw_mfma with the block's C operand in the workgroup's slab partial:
// `blk` is element (0, this lane's column) of the block, `ld` its row stride,
// rows below `rows` exist.  The first tile starts from zero without reading.
__device__ __forceinline__ void ppo_wide_dw_slab(float *blk, int ld, int rows, bool first,
                                                 const float *xa, const float *zb, bool valid,
                                                 bool comp, int h) {
    ppo_f32x16 c = {};
    if (!first) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = ppo_acc_row(r, h);
            if (row < rows) c[r] = blk[row * ld];
        }
    }
    c = ppo_dw_mfma(c, xa, zb, valid, comp);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = ppo_acc_row(r, h);
        if (row < rows) blk[row * ld] = c[r];
    }
}

// The whole wide gradient kernel but its __global__ line (see the header comment).
template <class Args>
__device__ __forceinline__ void ppo_grad_wide_tiles(const Args &g) {
    extern __shared__ float ppo_lds[];
    const PolicyPlan &a = g.p;
    const int L = a.n_hidden;
    float *wbuf = ppo_lds;
    float *xbase = wbuf + g.w_floats;                       // X_0's chunk, X_1 .. X_{n_hidden}
    float *dzh = xbase + (L + 1) * g.act_floats;            // one head chunk of z, then dZ
    float *wrow = dzh + kPpoWideChunk * kPpoLd;             // [32] row weights
    float *rowstat = wrow + kPpoTile;                       // [kPpoRowStats][32]
    int *rowsrc = reinterpret_cast<int *>(rowstat + kPpoRowStats * kPpoTile);   // [32]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int li = lane & 31, h = lane >> 5;
    const int net = blockIdx.y;
    const int n0 = wave * 32;
    const float inv_n = 1.0f / static_cast<float>(g.n_total);
    float *part = g.slab + static_cast<long long>(blockIdx.x) * g.img_floats;

    ppo_f32x16 dwh[2][4] = {};          // hidden-to-hidden dW (layers 1 and 2)
    float db[kPlanLayers - 1] = {};     // db of layers below the head
    double stat_acc = 0.0;

    double sum_logstd = 0.0;
    for (int c = 0; c < a.A; ++c) sum_logstd += a.img[a.off_logstd + c];

    const int ipL = a.in_pad[L], opL = a.out_pad[net][L];
    const bool one_chunk = opL <= kPpoWideChunk;

    // z = (action - mean) / std of head columns c0 .. c0 + cw - 1 from the
    // staged chunk into dzh: the float64 sum of single-MFMA products, zero past
    // A and past the last row.  Both passes come through here.
    const auto head_z = [&](int c0, int cw) {
        if (n0 >= cw) return;           // wave-uniform
        const int ld = cw + 1, lc = n0 + li, col = c0 + lc;
        const float *xa = xbase + L * g.act_floats + h * kPpoLd + li;
        const float *wb = wbuf + h * ld + lc;
        const float bias = a.img[a.off_b[0][L] + col];
        const bool on = col < a.A;
        // std in float64: a relative error in it is a common relative error of
        // every z of the column
        const double sd_d = on ? exp(static_cast<double>(a.img[a.off_logstd + col])) : 1.0;
        double accd[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) accd[r] = 0.0;
        for (int k = 0; k < ipL; k += 2) {
            const float xv = ppo_act(xa[k * kPpoLd]);
            const ppo_f32x16 zero = {};
            const ppo_f32x16 c = __builtin_amdgcn_mfma_f32_32x32x2f32(xv, wb[k * ld], zero, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 16; ++r) accd[r] += c[r];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = ppo_acc_row(r, h);
            const int s = rowsrc[row];
            float z = 0.0f;
            if (on && s >= 0)
                z = static_cast<float>((g.action_row(s, a.A)[col] - (accd[r] + bias)) / sd_d);
            dzh[lc * kPpoLd + row] = z;
        }
    };

    for (int tile = blockIdx.x; tile < g.tiles; tile += g.grid) {
        const bool first = tile == static_cast<int>(blockIdx.x);
        const long long row0 = static_cast<long long>(tile) * kPpoTile;
        const int live = g.n - row0 < kPpoTile ? static_cast<int>(g.n - row0) : kPpoTile;
        __syncthreads();       // the previous tile's last LDS readers are done
        if (tid < kPpoTile) rowsrc[tid] = tid < live ? ppo_src_row(g.idx, row0 + tid, g.m) : -1;
        if (tid < kPpoRowStats * kPpoTile) rowstat[tid] = 0.0f;

        // ------------------------------------------------------------ forward
        {   // The first layer in float64 on the vector units over the K-chunks:
            // thread t owns row t & 31 and units t >> 5, + 8, ...
            const int ip = a.in_pad[0], op = a.out_pad[net][0], ld = op + 1;
            const int row = tid & 31, cg = tid >> 5;
            double acc0[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) acc0[j] = 0.0;
            for (int k0 = 0; k0 < ip; k0 += kPpoWideChunk) {
                const int kc = ip - k0 < kPpoWideChunk ? ip - k0 : kPpoWideChunk;
                __syncthreads();      // rowsrc is set; the previous chunk is read
                ppo_wide_stage_obs(xbase, g.obs, rowsrc, a.D, k0, kc);
                ppo_wide_stage_w(wbuf, a.img + a.off_w[net][0] + static_cast<long long>(k0) * op,
                                 kc, op, op);
                __syncthreads();
                const float *xr = xbase + row;
                for (int k = 0; k < kc; ++k) {
                    const double x = xr[k * kPpoLd];
                    const float *wr = wbuf + k * ld + cg;
#pragma unroll
                    for (int j = 0; j < 16; ++j)
                        if (8 * j < op) acc0[j] = fma(x, static_cast<double>(wr[8 * j]), acc0[j]);
                }
            }
            float *nxt = xbase + g.act_floats;
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (8 * j < op) {
                    const int col = cg + 8 * j;
                    nxt[col * kPpoLd + row] =
                        ppo_tanh_comp(static_cast<float>(acc0[j] + a.img[a.off_b[net][0] + col]));
                }
            __syncthreads();
        }
        // the hidden layers, and the value head (one chunk each way: the narrow body)
        for (int l = 1; l <= L; ++l) {
            if (l == L && net == 0) break;
            const int ip = a.in_pad[l], op = a.out_pad[net][l], ld = op + 1;
            const float *cur = xbase + l * g.act_floats;
            ppo_wide_stage_w(wbuf, a.img + a.off_w[net][l], ip, op, op);
            __syncthreads();
            if (n0 < op) {   // wave-uniform
                const float *xa = cur + h * kPpoLd + li;
                const float *wb = wbuf + h * ld + n0 + li;
                const int col = n0 + li;
                const float bias = a.img[a.off_b[net][l] + col];
                ppo_f32x16 acc = {};
                for (int k = 0; k < ip; k += 2)
                    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(ppo_act(xa[k * kPpoLd]), wb[k * ld],
                                                               acc, 0, 0, 0);
                if (l < L) {
                    float *nxt = xbase + (l + 1) * g.act_floats;
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        nxt[col * kPpoLd + ppo_acc_row(r, h)] = ppo_tanh_comp(acc[r] + bias);
                } else {
                    // the value head: column 0 carries dZ, the padding zeros
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = ppo_acc_row(r, h);
                        const int s = rowsrc[row];
                        float dz = 0.0f;
                        if (col == 0 && s >= 0) dz = g.vf_row(s, acc[r] + bias, inv_n, rowstat + row);
                        dzh[col * kPpoLd + row] = dz;
                    }
                }
            }
            __syncthreads();
        }

        // ------------------------------------- the policy's head, pass 1: w
        if (net == 0) {
            const int r = tid >> 3, pt = tid & 7;
            double s = 0.0;      // sum z^2 reaches the head's width: float32 would round
            for (int c0 = 0; c0 < opL; c0 += kPpoWideChunk) {
                const int cw = opL - c0 < kPpoWideChunk ? opL - c0 : kPpoWideChunk;
                ppo_wide_stage_w(wbuf, a.img + a.off_w[0][L] + c0, ipL, cw, opL);
                __syncthreads();
                head_z(c0, cw);
                __syncthreads();
                const int nc = a.A - c0 < cw ? a.A - c0 : cw;
                for (int c = pt; c < nc; c += 8) {
                    const double z = dzh[c * kPpoLd + r];
                    s += z * z;
                }
                if (!one_chunk) __syncthreads();      // the stage and z are free
            }
            ppo_row_weight(g, rowsrc, rowstat, wrow, s, sum_logstd, inv_n);
            __syncthreads();
        }
        // the tile's statistic sums, rows in order, one thread per statistic
        if (tid >= 128 && tid < 128 + kPpoRowStats) {
            const float *rs = rowstat + (tid - 128) * kPpoTile;
            double s = 0.0;
            for (int r = 0; r < kPpoTile; ++r) s += rs[r];
            stat_acc += s;
        }

        // ----------------------------------------------------------- backward
        {   // the head layer over its N-chunks (pass 2 of the policy's head)
            float *x = xbase + L * g.act_floats;
            ppo_f32x16 accx = {};     // dX = dZ W^T, one chain across the chunks
            for (int c0 = 0; c0 < opL; c0 += kPpoWideChunk) {
                const int cw = opL - c0 < kPpoWideChunk ? opL - c0 : kPpoWideChunk;
                const int ld = cw + 1;
                if (net == 0) {
                    if (!one_chunk) {
                        ppo_wide_stage_w(wbuf, a.img + a.off_w[0][L] + c0, ipL, cw, opL);
                        __syncthreads();
                        head_z(c0, cw);
                        __syncthreads();
                    }
                    // dZ = -w z / std over z, column by column; dlogstd on the way
                    if (tid < cw) {
                        const int colg = c0 + tid;
                        const bool on = colg < a.A;
                        const float inv_sd = on ? expf(-a.img[a.off_logstd + colg]) : 0.0f;
                        float *col = dzh + tid * kPpoLd;
                        float s = 0.0f;
                        for (int r = 0; r < kPpoTile; ++r) {
                            const float z = col[r], w = wrow[r];
                            s += w * (1.0f - z * z);
                            col[r] = -w * z * inv_sd;
                        }
                        if (on) {
                            float *at = part + a.off_logstd + colg;
                            float dls = first ? 0.0f : *at;
                            dls += s;
                            *at = dls;
                        }
                    }
                    __syncthreads();
                }
                // dW_L += X_L^T dZ_L in the slab partial
                const int nni = cw >> 5, nb = (ipL >> 5) * nni;      // ipL is a hidden width
#pragma unroll 1
                for (int b = wave; b < nb; b += 4) {                 // wave-uniform
                    const int mi = b / nni, ni = b - mi * nni;
                    ppo_wide_dw_slab(part + a.off_w[net][L] + static_cast<long long>(mi) * 32 * opL +
                                         c0 + ni * 32 + li,
                                     opL, 32, first, x + (mi * 32 + li) * kPpoLd + h,
                                     dzh + (ni * 32 + li) * kPpoLd + h, true, true, h);
                }
                if (tid < cw) {       // ppo_col_sum's text (see ppo_grad_tile.h's header)
                    const float *col = dzh + tid * kPpoLd;
                    float s = 0.0f;
                    for (int r = 0; r < kPpoTile; ++r) s += col[r];
                    float *at = part + a.off_b[net][L] + c0 + tid;
                    float v = first ? 0.0f : *at;
                    v += s;
                    *at = v;
                }
                if (n0 < ipL) {       // this chunk's columns of the dX chain: ppo_dx_mfma's text
                    const float *za = dzh + h * kPpoLd + li;
                    const float *wb = wbuf + (n0 + li) * ld + h;
                    for (int k = 0; k < cw; k += 2)
                        accx = __builtin_amdgcn_mfma_f32_32x32x2f32(za[k * kPpoLd], wb[k], accx, 0, 0, 0);
                }
                __syncthreads();      // every read of the stage, dZ and X_L is done
            }
            if (n0 < ipL) {
                float *col = x + (n0 + li) * kPpoLd;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = ppo_acc_row(r, h);
                    const float u = fabsf(col[row]);
                    col[row] = accx[r] * (u * (2.0f - u));      // 1 - y^2 = u (2 - u)
                }
            }
            __syncthreads();
        }
        // the hidden-to-hidden layers, top down: the narrow body
#pragma unroll
        for (int l = kPlanLayers - 2; l >= 1; --l) {
            if (l >= L) continue;
            const int ip = a.in_pad[l], op = a.out_pad[net][l], ld = op + 1;
            float *x = xbase + l * g.act_floats;
            const float *dz = xbase + (l + 1) * g.act_floats;
            ppo_wide_stage_w(wbuf, a.img + a.off_w[net][l], ip, op, op);
            const int nni = op >> 5, nb = (ip >> 5) * nni;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int b = wave + 4 * j;
                if (b < nb) {   // wave-uniform
                    const int mi = b / nni, ni = b - mi * nni;
                    dwh[l - 1][j] = ppo_dw_mfma(dwh[l - 1][j], x + (mi * 32 + li) * kPpoLd + h,
                                                dz + (ni * 32 + li) * kPpoLd + h, true, true);
                }
            }
            if (tid < op) db[l] += ppo_col_sum(dz + tid * kPpoLd);
            __syncthreads();      // W_l staged
            ppo_f32x16 acc = {};
            if (n0 < ip)          // dX = dZ_l W_l^T
                acc = ppo_dx_mfma(acc, dz + h * kPpoLd + li, wbuf + (n0 + li) * ld + h, op);
            __syncthreads();      // every dW_l read of X_l is done
            if (n0 < ip) {
                float *col = x + (n0 + li) * kPpoLd;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int row = ppo_acc_row(r, h);
                    const float u = fabsf(col[row]);
                    col[row] = acc[r] * (u * (2.0f - u));
                }
            }
            __syncthreads();
        }
        {   // the first layer: db_0, and dW_0 += X_0^T dZ_0 over the K-chunks in
            // the slab partial
            const int ip = a.in_pad[0], op = a.out_pad[net][0];
            const float *dz = xbase + g.act_floats;
            if (tid < op) db[0] += ppo_col_sum(dz + tid * kPpoLd);
            const int nni = op >> 5;
            for (int k0 = 0; k0 < ip; k0 += kPpoWideChunk) {
                const int kc = ip - k0 < kPpoWideChunk ? ip - k0 : kPpoWideChunk;
                if (k0 > 0) __syncthreads();      // the previous chunk is read
                ppo_wide_stage_obs(xbase, g.obs, rowsrc, a.D, k0, kc);
                __syncthreads();
                const int nb = ((kc + 31) >> 5) * nni;
#pragma unroll 1
                for (int b = wave; b < nb; b += 4) {                 // wave-uniform
                    const int mi = b / nni, ni = b - mi * nni;
                    const int mrow = mi * 32 + li;
                    const bool valid = mrow < kc;
                    ppo_wide_dw_slab(part + a.off_w[net][0] +
                                         static_cast<long long>(k0 + mi * 32) * op + ni * 32 + li,
                                     op, kc - mi * 32, first, xbase + (valid ? mrow : 0) * kPpoLd + h,
                                     dz + (ni * 32 + li) * kPpoLd + h, valid, false, h);
                }
            }
        }
    }

    // ------------------------------- what stayed on chip: this workgroup's partial
#pragma unroll
    for (int l = 0; l < kPlanLayers - 1; ++l) {
        if (l >= L) continue;
        const int ip = a.in_pad[l], op = a.out_pad[net][l];
        if (l > 0) {
            const int nni = op >> 5, nb = (ip >> 5) * nni;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int b = wave + 4 * j;
                if (b < nb) {
                    const int mi = b / nni, ni = b - mi * nni;
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        part[a.off_w[net][l] + (mi * 32 + ppo_acc_row(r, h)) * op + ni * 32 + li] =
                            dwh[l - 1][j][r];
                }
            }
        }
        if (tid < op) part[a.off_b[net][l] + tid] = db[l];
    }
    ppo_store_stats(g, stat_acc);
}

}  // namespace ce
