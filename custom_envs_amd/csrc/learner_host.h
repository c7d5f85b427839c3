// The host shell the two learners share (ppo2_engine.hip, a2c_engine.hip):
// what every learner holds besides its optimiser state (ce::LearnerCore), its
// construction and teardown, the parameter entry points, the argument checks
// that do not depend on the loss, and the launches around the gradient kernel.
//
// A learner keeps its config check, its per-tensor null checks, the launch of
// its own gradient kernel (its loss head's arguments) and its optimiser:
//   struct ce_x { ce_x_config cfg; <optimiser state>; ce::LearnerCore core; };
//   create    learner_core_create(l->core, policy, grid_limit, x_grad_kernel, bail),
//             then its own buffers and one hipDeviceSynchronize
//   destroy   its own buffers, then learner_core_destroy
//   gradient  learner_fill_grad_args(g, core, ...), its own fields, the launch,
//             then learner_enqueue_reduce_finish<x_finish_kernel>(...)
//   exchange  the same launch with the ranks' row count, then
//             learner_enqueue_partial(...); from the gathered records
//             learner_enqueue_combine_finish<x_finish_kernel>(...) and its
//             optimiser ("the gradient exchange" below)
// Dispatch is static (a kernel that differs is a template parameter); nothing
// here allocates on a call path, and every argument check precedes the first
// HIP call.
//
// The checks that need neither a PolicyPlan nor a kernel (rows, a partial's
// record, the gathered records, the parameter vector, the optimiser's blocks)
// are learner_checks.h's, which the DDPG learner (ddpg_engine.hip) shares; what
// is left here is bound to a policy.
#pragma once

#include <algorithm>
#include <climits>
#include <cstdint>
#include <string>

#include "common.h"
#include "learner_checks.h"
#include "policy_engine.h"
#include "ppo_grad_tile.h"
#include "ppo_grad_wide_tile.h"

namespace ce {

struct LearnerCore {
    ce_policy *policy = nullptr;
    PolicyPlan plan{};
    int grid_max = 0;            // workgroups per network the slab holds
    int n_sq = 0;                // blocks of ppo2_reduce_kernel
    int w_floats = 0, act_floats = 0;
    size_t lds_bytes = 0;        // of the gradient kernel for this policy's shape
    bool wide = false;           // from ce_<x>_create_wide: the wide gradient kernel
    float *params = nullptr;     // the master flat parameters
    float *grad = nullptr, *slab = nullptr;
    double *stat_slab = nullptr, *sq = nullptr;
};

// Workgroups per network of a wide learner unless grid_limit names another
// number: a partial is img_floats floats (0.7 MB at 981 -> 64 -> 64 -> 490,
// 1.6 MB at the limits), the reduce reads `grid` of them every step, and the
// first layer's and the head's dW blocks travel to the partial and back once
// per tile: one partial per CU would be a 175 MB (410 MB) slab.
constexpr int kLearnerWideGrid = 64;

// The wide gradient kernel's limits against a plan (no HIP call).  Only the
// first branch can be reached from outside: ce_policy_create_wide holds a wide
// handle to the same limits (kPlanWideMaxD / A, the hidden widths); the rest
// guards the kernel's LDS plan should the two ever part.
inline int learner_wide_shape_ok(const char *who, const PolicyPlan &pa) {
    const auto bad = [who](int code, const std::string &what) {
        return fail(code, std::string(who) + what);
    };
    if (!pa.wide)
        return bad(CE_EINVAL, ": the policy must come from ce_policy_create_wide (a narrow "
                              "handle trains under the narrow create)");
    if (pa.D > kPpoWideMaxD)
        return bad(CE_EUNSUPPORTED, ": obs_dim " + std::to_string(pa.D) + " exceeds the limit of " +
                                        std::to_string(kPpoWideMaxD));
    if (pa.A > kPpoWideMaxA)
        return bad(CE_EUNSUPPORTED, ": act_dim " + std::to_string(pa.A) + " exceeds the limit of " +
                                        std::to_string(kPpoWideMaxA));
    if (pa.n_hidden < 1 || pa.n_hidden > kPlanLayers - 1)
        return bad(CE_EUNSUPPORTED, ": the learner takes 1 to 3 hidden layers, got " +
                                        std::to_string(pa.n_hidden));
    for (int l = 1; l <= pa.n_hidden; ++l)
        if (pa.in_pad[l] % 32 != 0 || pa.in_pad[l] < 32 || pa.in_pad[l] > 128)
            return bad(CE_EUNSUPPORTED, ": hidden width " + std::to_string(pa.in_pad[l]) +
                                            " is not a multiple of 32 up to 128");
    return CE_OK;
}

// What both kinds of learner do after their LDS plan: the device, grid_max
// (grid_limit, else `grid_default`, else the CU count), the kernel's
// dynamic-LDS attribute and the shared buffers, `params` zeroed.
template <class Bail>
int learner_core_alloc(LearnerCore &c, int grid_limit, int grid_default, const void *grad_kernel,
                       int max_lds_bytes, Bail &&bail) {
    const PolicyPlan &pa = c.plan;
    c.n_sq = (pa.n_params + 255) / 256;
    CE_TRY(hipSetDevice(pa.device));
    hipDeviceProp_t prop;
    CE_TRY(hipGetDeviceProperties(&prop, pa.device));
    const int cus = std::max(1, prop.multiProcessorCount);
    c.grid_max = grid_limit > 0 ? grid_limit : (grid_default > 0 ? std::min(grid_default, cus) : cus);
    CE_TRY(hipFuncSetAttribute(grad_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                               max_lds_bytes));   // the limits' need
    const size_t np = static_cast<size_t>(pa.n_params) * sizeof(float);
    CE_TRY(hipMalloc(&c.params, np));
    CE_TRY(hipMalloc(&c.grad, np));
    CE_TRY(hipMalloc(&c.slab, static_cast<size_t>(c.grid_max) * pa.img_floats * sizeof(float)));
    CE_TRY(hipMalloc(&c.stat_slab, static_cast<size_t>(c.grid_max) * 2 * kPpoRowStats * sizeof(double)));
    CE_TRY(hipMalloc(&c.sq, static_cast<size_t>(c.n_sq) * sizeof(double)));
    CE_TRY(hipMemset(c.params, 0, np));
    return CE_OK;
}

// The gradient kernel's LDS plan for c.plan (ppo_lds_floats): the weight stage
// holds the largest layer and an activation buffer the widest input, each
// clamped to `chunk` rows and columns; the head buffer has head_cols columns.
inline void learner_lds_plan(LearnerCore &c, int chunk, int head_cols) {
    const PolicyPlan &pa = c.plan;
    int wmax = 0, kmax = 0;
    for (int net = 0; net < 2; ++net)
        for (int i = 0; i <= pa.n_hidden; ++i) {
            const int ipc = std::min(pa.in_pad[i], chunk);
            wmax = std::max(wmax, ipc * (std::min(pa.out_pad[net][i], chunk) + 1));
            kmax = std::max(kmax, ipc);
        }
    c.w_floats = (wmax + 3) / 4 * 4;
    c.act_floats = kmax * kPpoLd;
    c.lds_bytes = static_cast<size_t>(ppo_lds_floats(c.w_floats, c.act_floats, pa.n_hidden,
                                                     head_cols)) * sizeof(float);
}

// The plan and the gradient kernel's LDS sizes, the device, grid_max, the
// kernel's dynamic-LDS attribute and the shared buffers, `params` zeroed.  A
// failed HIP call goes through the caller's `bail(code)`, which destroys the
// half-built learner.  The caller synchronises after its own initialisation.
// `wide`: called for ce_<x>_create_wide with the wide instance of the gradient
// kernel (ppo_grad_wide_tile.h): a wide policy handle, that kernel's LDS plan,
// and kLearnerWideGrid workgroups per network unless grid_limit says otherwise.
template <class Bail>
int learner_core_create(LearnerCore &c, ce_policy *policy, int grid_limit,
                        const void *grad_kernel, Bail &&bail, bool wide = false,
                        const char *who = "") {
    c.policy = policy;
    c.plan = policy_plan(policy);
    const PolicyPlan &pa = c.plan;
    if (wide) {
        const int rc = learner_wide_shape_ok(who, pa);
        if (rc != CE_OK) return bail(rc);
        c.wide = true;
        learner_lds_plan(c, kPpoWideChunk, kPpoWideChunk);
        return learner_core_alloc(c, grid_limit, kLearnerWideGrid, grad_kernel,
                                  kPpoWideMaxLdsBytes, bail);
    }
    // the gradient kernel holds a whole [in_pad][out_pad + 1] layer in LDS: a
    // wide handle (ce_policy_create_wide) acts, it is not trained here
    if (pa.wide)
        return bail(fail(CE_EUNSUPPORTED,
                         "the learners take obs_dim <= 128, act_dim <= 64: a policy from "
                         "ce_policy_create_wide (obs_dim " + std::to_string(pa.D) + ", act_dim " +
                             std::to_string(pa.A) + ") acts and rolls out only"));
    learner_lds_plan(c, INT_MAX, kPpoMaxA);      // whole layers staged
    return learner_core_alloc(c, grid_limit, 0, grad_kernel, kPpoMaxLdsBytes, bail);
}

inline void learner_core_destroy(LearnerCore &c) {
    for (void *q : {static_cast<void *>(c.params), static_cast<void *>(c.grad),
                    static_cast<void *>(c.slab), static_cast<void *>(c.stat_slab),
                    static_cast<void *>(c.sq)})
        if (q) (void)hipFree(q);
}

// ---- the parameter entry points (`core` null: a null learner) ---------------

inline int learner_n_params(const LearnerCore *core) { return core ? core->plan.n_params : -1; }

// `flat` into the master parameters and through to the policy's image.
inline int learner_set_params(const char *who, LearnerCore *core, const float *flat, int64_t n,
                              uint32_t flags, void *hip_stream) {
    const int rc = learner_params_ok(who, learner_n_params(core), "policy", flat, n, ": got ");
    if (rc != CE_OK) return rc;
    CE_CLEAR_STALE_ERROR_AT(who);
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const bool dev = (flags & CE_PTR_DEVICE) != 0;
    CE_HIP(hipMemcpyAsync(core->params, flat, n * sizeof(float),
                          dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
    if (!dev) CE_HIP(hipStreamSynchronize(stream));   // `flat` may be pageable
    policy_repack(core->policy, core->params, stream);
    CE_HIP(hipGetLastError());
    if (!dev) CE_HIP(hipStreamSynchronize(stream));
    return CE_OK;
}

inline int learner_get_params(const char *who, LearnerCore *core, float *flat, int64_t n,
                              uint32_t flags, void *hip_stream) {
    const int rc = learner_params_ok(who, learner_n_params(core), "policy", flat, n,
                                     ": got room for ");
    if (rc != CE_OK) return rc;
    CE_CLEAR_STALE_ERROR_AT(who);
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const bool dev = (flags & CE_PTR_DEVICE) != 0;
    CE_HIP(hipMemcpyAsync(flat, core->params, n * sizeof(float),
                          dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream));
    policy_repack(core->policy, core->params, stream);
    CE_HIP(hipGetLastError());
    if (!dev) CE_HIP(hipStreamSynchronize(stream));
    return CE_OK;
}

// ---- the optimiser's state in and out (learner_checks.h; `core` null: a null
// learner) -------------------------------------------------------------------
inline int learner_opt_state(const char *who, const LearnerCore *core, float *dev_a, float *dev_b,
                             const char *name_a, const char *name_b, void *a, void *b, int64_t n,
                             bool set, uint32_t flags, void *hip_stream) {
    return learner_opt_state(who, learner_n_params(core), "policy", dev_a, dev_b, name_a, name_b, a,
                             b, n, set, flags, hip_stream);
}

// ---- argument checks --------------------------------------------------------

// the record stride of a [k][rows] float view (`name`: "reward", "value")
inline int learner_stride_ok(const char *who, const char *name, int64_t stride_bytes,
                             int64_t rows) {
    if (stride_bytes < rows * 4 || stride_bytes % 4 != 0)
        return fail(CE_EINVAL, std::string(who) + ": " + name + "_stride_bytes must be a multiple "
                                   "of 4 of at least rows * 4");
    return CE_OK;
}

// k, rows and the reward / done records of a rollout (`cap_total`: k * rows
// is bounded as a batch's rows are, for a gradient over all of them)
inline int learner_records_ok(const char *who, int32_t k, int64_t rows, const float *rewards,
                              int64_t reward_stride_bytes, const uint8_t *dones,
                              int64_t done_stride_bytes, const float *last_values,
                              bool cap_total) {
    const auto bad = [who](const std::string &what) { return fail(CE_EINVAL, who + what); };
    if (k < 1) return bad(": k must be at least 1, got " + std::to_string(k));
    if (rows < 1 || rows > kLearnerMaxRows)
        return bad(": rows must be in [1, 2^24], got " + std::to_string(rows));
    if (cap_total && int64_t(k) * rows > kLearnerMaxRows)
        return bad(": k * rows must be at most 2^24, got " + std::to_string(int64_t(k) * rows));
    if (!rewards) return bad(": null rewards");
    if (!dones) return bad(": null dones");
    if (!last_values) return bad(": null last_values");
    const int rc = learner_stride_ok(who, "reward", reward_stride_bytes, rows);
    if (rc != CE_OK) return rc;
    if (done_stride_bytes < rows) return bad(": done_stride_bytes must be at least rows");
    if (reinterpret_cast<uintptr_t>(rewards) & 3) return bad(": rewards must be 4-byte aligned");
    return CE_OK;
}

// ---- the launches around a gradient kernel ----------------------------------

// The fields of a gradient kernel's arguments every learner sets alike
// (Ppo2GradArgs names them); the loss head's own are the caller's.
template <class Args>
void learner_fill_grad_args(Args &g, const LearnerCore &c, float vf_coef, int64_t n,
                            int64_t n_total, int64_t m, const int32_t *idx, const float *obs) {
    g.p = c.plan;
    g.n = static_cast<int>(n);
    g.n_total = static_cast<int>(n_total);
    g.m = static_cast<int>(m);
    g.tiles = static_cast<int>((n + kPpoTile - 1) / kPpoTile);
    g.grid = std::min(g.tiles, c.grid_max);
    g.img_floats = c.plan.img_floats;
    g.w_floats = c.w_floats;
    g.act_floats = c.act_floats;
    g.vf_coef = vf_coef;
    g.idx = idx;
    g.obs = obs;
    g.slab = c.slab;
    g.stat_slab = c.stat_slab;
}

// [finish]: the statistics of n rows from `parts` statistic partials,
// `stat_stride` doubles apart, and the |grad|^2 blocks in c.sq.
template <void (*Finish)(Ppo2FinishArgs)>
void learner_enqueue_finish(const LearnerCore &c, int n, int parts, const double *stat_parts,
                            int stat_stride, float ent_coef, float vf_coef, float *stats,
                            hipStream_t stream) {
    Ppo2FinishArgs f{};
    f.n = n;
    f.grid = parts;
    f.n_sq = c.n_sq;
    f.A = c.plan.A;
    f.off_logstd = c.plan.off_logstd;
    f.stat_stride = stat_stride;
    f.ent_coef = ent_coef;
    f.vf_coef = vf_coef;
    f.img = c.plan.img;
    f.stat_slab = stat_parts;
    f.sq = c.sq;
    f.stats = stats;
    hipLaunchKernelGGL(Finish, dim3(1), dim3(256), 0, stream, f);
}

// [reduce, finish] after a gradient kernel of `grid` workgroups per network
// over n rows: the slab into grad, the statistics and |grad|^2 into stats.
template <void (*Finish)(Ppo2FinishArgs)>
void learner_enqueue_reduce_finish(const LearnerCore &c, int n, int grid, float ent_coef,
                                   float vf_coef, float *grad, float *stats,
                                   hipStream_t stream) {
    Ppo2ReduceArgs q{};
    q.p = c.plan;
    q.grid = grid;
    q.ent_coef = ent_coef;
    q.slab = c.slab;
    q.grad = grad;
    q.sq = c.sq;
    ppo2_launch_reduce(q, stream);
    learner_enqueue_finish<Finish>(c, n, grid, c.stat_slab, 2 * kPpoRowStats, ent_coef, vf_coef,
                                   stats, stream);
}

// ---- the gradient exchange ---------------------------------------------------
// W ranks, rank r with n_r rows, take the single learner's step on all N =
// sum n_r rows.  Each rank runs
//   partial   [its moments' merge (PPO2), gradient kernel with N, partial
//             reduce]: its record (ppo_grad_tile.h) into slot r of a
//             [W][record] buffer
// the caller all-gathers the buffer in place, and each rank runs
//   apply     [combine, finish, optimiser, repack] from the W records
// Every rank adds the same float64 values in rank order, so every rank gets
// the same bits; at W = 1 they are the bits of [gradient, reduce, finish].

// [partial reduce] after a gradient kernel of `grid` workgroups per network
// over this rank's n rows: the slab and the statistic sums into `record`.
inline void learner_enqueue_partial(const LearnerCore &c, int n, int grid, double *record,
                                    hipStream_t stream) {
    Ppo2PartialArgs q{};
    q.p = c.plan;
    q.grid = grid;
    q.n = n;
    q.slab = c.slab;
    q.stat_slab = c.stat_slab;
    q.record = record;
    ppo2_launch_partial(q, stream);
}

// [combine, finish] from the gathered records: grad, and the statistics of
// all n_total rows into stats.
template <void (*Finish)(Ppo2FinishArgs)>
void learner_enqueue_combine_finish(const LearnerCore &c, int world, const double *records,
                                    int64_t n_total, float ent_coef, float vf_coef, float *grad,
                                    float *stats, hipStream_t stream) {
    Ppo2CombineArgs q{};
    q.n_params = c.plan.n_params;
    q.off_logstd_flat = c.plan.seg_src[c.plan.n_segs - 1];
    q.world = world;
    q.record_doubles = ppo_record_doubles(c.plan.n_params);
    q.ent_coef = ent_coef;
    q.records = records;
    q.grad = grad;
    q.sq = c.sq;
    ppo2_launch_combine(q, stream);
    learner_enqueue_finish<Finish>(c, static_cast<int>(n_total), world, records + c.plan.n_params,
                                   q.record_doubles, ent_coef, vf_coef, stats, stream);
}

}  // namespace ce
