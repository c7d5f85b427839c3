// C-ABI implementation of the A2C learner (ce_a2c_* in
// include/custom_envs_amd.h): owns the master flat parameters, RMSProp's ms
// and mom, the partial slab of a2c_grad_kernel and the returns buffer of
// ce_a2c_update, and enqueues [gradient, reduce, finish, RMSProp, repack] --
// ce_a2c_update: the returns scan first, the gradient on the rollout records
// in place -- on the caller's stream.  Every argument check precedes the first
// HIP call, and the checks of the plain arguments precede the check of the
// handle, so they run without a device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <string>
#include <vector>

#include "a2c_kernels.h"
#include "common.h"
#include "policy_engine.h"

struct ce_a2c {
    ce_a2c_config cfg{};
    ce_policy *policy = nullptr;
    ce::PolicyPlan plan{};
    int grid_max = 0;            // workgroups per network the slab holds
    int n_sq = 0;                // blocks of ppo2_reduce_kernel
    int w_floats = 0, act_floats = 0;
    size_t lds_bytes = 0;
    float *params = nullptr, *ms = nullptr, *mom = nullptr, *grad = nullptr;
    float *slab = nullptr;
    double *stat_slab = nullptr, *sq = nullptr;
    float *ret = nullptr;        // ce_a2c_update's returns, [ret_cap]
    int64_t ret_cap = 0;
};

namespace {

using ce::fail;

constexpr int64_t kMaxRows = int64_t(1) << 24;

int config_ok(const char *who, const ce_a2c_config *c) {
    const std::string w(who);
    if (!c) return fail(CE_EINVAL, w + ": null config");
    if (!(c->gamma >= 0.0f && c->gamma <= 1.0f)) return fail(CE_EINVAL, w + ": gamma must be in [0, 1]");
    if (!std::isfinite(c->ent_coef) || !std::isfinite(c->vf_coef))
        return fail(CE_EINVAL, w + ": ent_coef and vf_coef must be finite");
    if (std::isnan(c->max_grad_norm)) return fail(CE_EINVAL, w + ": max_grad_norm is not a number");
    if (!(c->lr > 0.0f)) return fail(CE_EINVAL, w + ": lr must be positive");
    if (!(c->alpha >= 0.0f && c->alpha < 1.0f)) return fail(CE_EINVAL, w + ": alpha must be in [0, 1)");
    if (!(c->eps > 0.0f)) return fail(CE_EINVAL, w + ": eps must be positive");
    if (!(c->momentum >= 0.0f && c->momentum < 1.0f))
        return fail(CE_EINVAL, w + ": momentum must be in [0, 1)");
    if (c->grid_limit < 0) return fail(CE_EINVAL, w + ": grid_limit must not be negative");
    return CE_OK;
}

int batch_ok(const char *who, const ce_a2c *l, int64_t n, int64_t m, const int32_t *idx,
             const float *obs, const float *actions, const float *ret, const float *old_values,
             const float *stats) {
    const std::string w(who);
    if (n < 1) return fail(CE_EINVAL, w + ": n must be at least 1, got " + std::to_string(n));
    if (m < 1 || m > kMaxRows)
        return fail(CE_EINVAL, w + ": m must be in [1, 2^24], got " + std::to_string(m));
    if (n > kMaxRows) return fail(CE_EINVAL, w + ": n must be at most 2^24");
    if (!idx && n > m)
        return fail(CE_EINVAL, w + ": n exceeds m and there is no idx to gather by");
    if (!obs) return fail(CE_EINVAL, w + ": null obs");
    if (!actions) return fail(CE_EINVAL, w + ": null actions");
    if (!ret) return fail(CE_EINVAL, w + ": null returns");
    if (!old_values) return fail(CE_EINVAL, w + ": null old_values");
    if (!stats) return fail(CE_EINVAL, w + ": null stats");
    if (!l) return fail(CE_EINVAL, w + ": null learner");
    return CE_OK;
}

// k, rows and the reward / done records of a rollout
int records_ok(const std::string &w, int32_t k, int64_t rows, const float *rewards,
               int64_t reward_stride_bytes, const uint8_t *dones, int64_t done_stride_bytes,
               const float *last_values) {
    if (k < 1) return fail(CE_EINVAL, w + ": k must be at least 1, got " + std::to_string(k));
    if (rows < 1 || rows > kMaxRows)
        return fail(CE_EINVAL, w + ": rows must be in [1, 2^24], got " + std::to_string(rows));
    if (int64_t(k) * rows > kMaxRows)
        return fail(CE_EINVAL, w + ": k * rows must be at most 2^24, got " +
                                   std::to_string(int64_t(k) * rows));
    if (!rewards) return fail(CE_EINVAL, w + ": null rewards");
    if (!dones) return fail(CE_EINVAL, w + ": null dones");
    if (!last_values) return fail(CE_EINVAL, w + ": null last_values");
    if (reward_stride_bytes < rows * 4 || reward_stride_bytes % 4 != 0)
        return fail(CE_EINVAL, w + ": reward_stride_bytes must be a multiple of 4 of at least "
                                   "rows * 4");
    if (done_stride_bytes < rows) return fail(CE_EINVAL, w + ": done_stride_bytes must be at least rows");
    if (reinterpret_cast<uintptr_t>(rewards) & 3)
        return fail(CE_EINVAL, w + ": rewards must be 4-byte aligned");
    return CE_OK;
}

void enqueue_returns(const ce_a2c *l, int32_t k, int64_t rows, const float *rewards,
                     int64_t reward_stride_bytes, const uint8_t *dones, int64_t done_stride_bytes,
                     const float *last_values, float *ret, hipStream_t stream) {
    hipLaunchKernelGGL(ce::a2c_returns_kernel, dim3(static_cast<unsigned>((rows + 255) / 256)),
                       dim3(256), 0, stream, k, static_cast<int>(rows),
                       reinterpret_cast<const char *>(rewards),
                       static_cast<long long>(reward_stride_bytes), dones,
                       static_cast<long long>(done_stride_bytes), last_values, l->cfg.gamma, ret);
}

// [gradient, reduce, finish] into grad / stats.  Row s of the m-row batch is
// row s % rec_rows of record s / rec_rows of actions / old_values.
void enqueue_grad(const ce_a2c *l, int64_t n, int64_t m, const int32_t *idx, const float *obs,
                  const float *actions, int64_t action_stride, const float *ret,
                  const float *old_values, int64_t value_stride, int64_t rec_rows, float *grad,
                  float *stats, hipStream_t stream) {
    const ce_a2c_config &c = l->cfg;
    const ce::PolicyPlan &pa = l->plan;
    ce::A2cGradArgs g{};
    g.p = pa;
    g.n = static_cast<int>(n);
    g.m = static_cast<int>(m);
    g.tiles = static_cast<int>((n + ce::kPpoTile - 1) / ce::kPpoTile);
    g.grid = std::min(g.tiles, l->grid_max);
    g.img_floats = pa.img_floats;
    g.w_floats = l->w_floats;
    g.act_floats = l->act_floats;
    g.vf_coef = c.vf_coef;
    g.rec_rows = static_cast<int>(rec_rows);
    g.action_stride = action_stride;
    g.value_stride = value_stride;
    g.idx = idx;
    g.obs = obs;
    g.actions = actions;
    g.ret = ret;
    g.old_values = old_values;
    g.slab = l->slab;
    g.stat_slab = l->stat_slab;
    hipLaunchKernelGGL(ce::a2c_grad_kernel, dim3(g.grid, 2), dim3(ce::kPpoBlock), l->lds_bytes,
                       stream, g);
    ce::Ppo2ReduceArgs q{};
    q.p = pa;
    q.grid = g.grid;
    q.ent_coef = c.ent_coef;
    q.slab = l->slab;
    q.grad = grad;
    q.sq = l->sq;
    ce::ppo2_launch_reduce(q, stream);
    ce::Ppo2FinishArgs f{};
    f.n = g.n;
    f.grid = g.grid;
    f.n_sq = l->n_sq;
    f.A = pa.A;
    f.off_logstd = pa.off_logstd;
    f.ent_coef = c.ent_coef;
    f.vf_coef = c.vf_coef;
    f.img = pa.img;
    f.stat_slab = l->stat_slab;
    f.sq = l->sq;
    f.stats = stats;
    hipLaunchKernelGGL(ce::a2c_finish_kernel, dim3(1), dim3(256), 0, stream, f);
}

// [RMSProp, repack] from l->grad and the |grad|^2 in stats
void enqueue_rmsprop(ce_a2c *l, float lr, const float *stats, hipStream_t stream) {
    const ce_a2c_config &c = l->cfg;
    hipLaunchKernelGGL(ce::a2c_rmsprop_kernel, dim3((l->plan.n_params + 255) / 256), dim3(256), 0,
                       stream, l->plan.n_params, l->grad, stats, c.max_grad_norm,
                       lr > 0.0f ? lr : c.lr, c.alpha, static_cast<float>(1.0 - double(c.alpha)),
                       c.eps, c.momentum, l->params, l->ms, l->mom);
    ce::policy_repack(l->policy, l->params, stream);
}

}  // namespace

extern "C" {

int ce_a2c_create(ce_policy *policy, const ce_a2c_config *cfg, ce_a2c **out) {
    if (!out) return fail(CE_EINVAL, "ce_a2c_create: null output handle");
    *out = nullptr;
    int rc = config_ok("ce_a2c_create", cfg);
    if (rc != CE_OK) return rc;
    if (!policy) return fail(CE_EINVAL, "ce_a2c_create: null policy");
    ce_a2c *l = new (std::nothrow) ce_a2c();
    if (!l) return fail(CE_ENOMEM, "ce_a2c_create: host allocation failed");
    l->cfg = *cfg;
    l->policy = policy;
    l->plan = ce::policy_plan(policy);
    const ce::PolicyPlan &pa = l->plan;
    int wmax = 0, kmax = 0;
    for (int net = 0; net < 2; ++net)
        for (int i = 0; i <= pa.n_hidden; ++i) {
            wmax = std::max(wmax, pa.in_pad[i] * (pa.out_pad[net][i] + 1));
            kmax = std::max(kmax, pa.in_pad[i]);
        }
    l->w_floats = (wmax + 3) / 4 * 4;
    l->act_floats = kmax * ce::kPpoLd;
    l->lds_bytes = static_cast<size_t>(l->w_floats + (pa.n_hidden + 1) * l->act_floats +
                                       ce::kPpoMaxA * ce::kPpoLd +
                                       (ce::kPpoRowStats + 2) * ce::kPpoTile) * sizeof(float);
    l->n_sq = (pa.n_params + 255) / 256;
    auto bail = [&](int code) {
        ce_a2c_destroy(l);
        return code;
    };
#define CE_TRY(call)                                                           \
    do {                                                                       \
        hipError_t err_ = (call);                                              \
        if (err_ != hipSuccess)                                                \
            return bail(fail(CE_EHIP, std::string(#call " failed: ") +         \
                                          hipGetErrorString(err_)));           \
    } while (0)
    CE_TRY(hipSetDevice(pa.device));
    hipDeviceProp_t prop;
    CE_TRY(hipGetDeviceProperties(&prop, pa.device));
    l->grid_max = cfg->grid_limit > 0 ? cfg->grid_limit : std::max(1, prop.multiProcessorCount);
    CE_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(ce::a2c_grad_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize,
                               static_cast<int>(ce::kPpoMaxLdsBytes)));   // the limits' need
    const size_t np = static_cast<size_t>(pa.n_params) * sizeof(float);
    CE_TRY(hipMalloc(&l->params, np));
    CE_TRY(hipMalloc(&l->ms, np));
    CE_TRY(hipMalloc(&l->mom, np));
    CE_TRY(hipMalloc(&l->grad, np));
    CE_TRY(hipMalloc(&l->slab, static_cast<size_t>(l->grid_max) * pa.img_floats * sizeof(float)));
    CE_TRY(hipMalloc(&l->stat_slab, static_cast<size_t>(l->grid_max) * 2 * ce::kPpoRowStats * sizeof(double)));
    CE_TRY(hipMalloc(&l->sq, static_cast<size_t>(l->n_sq) * sizeof(double)));
    const std::vector<float> ones(pa.n_params, 1.0f);     // TF's slot initialiser of ms
    CE_TRY(hipMemset(l->params, 0, np));
    CE_TRY(hipMemcpy(l->ms, ones.data(), np, hipMemcpyHostToDevice));
    CE_TRY(hipMemset(l->mom, 0, np));
    CE_TRY(hipDeviceSynchronize());
#undef CE_TRY
    *out = l;
    return CE_OK;
}

void ce_a2c_destroy(ce_a2c *l) {
    if (!l) return;
    for (void *q : {static_cast<void *>(l->params), static_cast<void *>(l->ms),
                    static_cast<void *>(l->mom), static_cast<void *>(l->grad),
                    static_cast<void *>(l->slab), static_cast<void *>(l->stat_slab),
                    static_cast<void *>(l->sq), static_cast<void *>(l->ret)})
        if (q) (void)hipFree(q);
    delete l;
}

int ce_a2c_set_params(ce_a2c *l, const float *flat, int64_t n, uint32_t flags, void *hip_stream) {
    if (!flat) return fail(CE_EINVAL, "ce_a2c_set_params: null parameter vector");
    if (!l) return fail(CE_EINVAL, "ce_a2c_set_params: null learner");
    if (n != l->plan.n_params)
        return fail(CE_EINVAL, "ce_a2c_set_params: got " + std::to_string(n) +
                                   " parameters, the policy has " + std::to_string(l->plan.n_params));
    CE_CLEAR_STALE_ERROR();
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const bool dev = (flags & CE_PTR_DEVICE) != 0;
    CE_HIP(hipMemcpyAsync(l->params, flat, n * sizeof(float),
                          dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
    if (!dev) CE_HIP(hipStreamSynchronize(stream));   // `flat` may be pageable
    ce::policy_repack(l->policy, l->params, stream);
    CE_HIP(hipGetLastError());
    if (!dev) CE_HIP(hipStreamSynchronize(stream));
    return CE_OK;
}

int ce_a2c_get_params(ce_a2c *l, float *flat, int64_t n, uint32_t flags, void *hip_stream) {
    if (!flat) return fail(CE_EINVAL, "ce_a2c_get_params: null parameter vector");
    if (!l) return fail(CE_EINVAL, "ce_a2c_get_params: null learner");
    if (n != l->plan.n_params)
        return fail(CE_EINVAL, "ce_a2c_get_params: got room for " + std::to_string(n) +
                                   " parameters, the policy has " + std::to_string(l->plan.n_params));
    CE_CLEAR_STALE_ERROR();
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const bool dev = (flags & CE_PTR_DEVICE) != 0;
    CE_HIP(hipMemcpyAsync(flat, l->params, n * sizeof(float),
                          dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream));
    ce::policy_repack(l->policy, l->params, stream);
    CE_HIP(hipGetLastError());
    if (!dev) CE_HIP(hipStreamSynchronize(stream));
    return CE_OK;
}

int ce_a2c_returns(const ce_a2c *l, int32_t k, int64_t rows, const float *rewards,
                   int64_t reward_stride_bytes, const uint8_t *dones, int64_t done_stride_bytes,
                   const float *last_values, float *ret, void *hip_stream) {
    const std::string w("ce_a2c_returns");
    const int rc = records_ok(w, k, rows, rewards, reward_stride_bytes, dones, done_stride_bytes,
                              last_values);
    if (rc != CE_OK) return rc;
    if (!ret) return fail(CE_EINVAL, w + ": null ret output");
    if (!l) return fail(CE_EINVAL, w + ": null learner");
    CE_CLEAR_STALE_ERROR();
    enqueue_returns(l, k, rows, rewards, reward_stride_bytes, dones, done_stride_bytes,
                    last_values, ret, static_cast<hipStream_t>(hip_stream));
    CE_HIP(hipGetLastError());
    return CE_OK;
}

int ce_a2c_grad(ce_a2c *l, int64_t n, int64_t m, const int32_t *idx, const float *obs,
                const float *actions, const float *returns, const float *old_values, float *grad,
                float *stats, void *hip_stream) {
    if (!grad) return fail(CE_EINVAL, "ce_a2c_grad: null grad");
    const int rc = batch_ok("ce_a2c_grad", l, n, m, idx, obs, actions, returns, old_values, stats);
    if (rc != CE_OK) return rc;
    CE_CLEAR_STALE_ERROR();
    enqueue_grad(l, n, m, idx, obs, actions, 0, returns, old_values, 0, m, grad, stats,
                 static_cast<hipStream_t>(hip_stream));
    CE_HIP(hipGetLastError());
    return CE_OK;
}

int ce_a2c_step(ce_a2c *l, int64_t n, int64_t m, const int32_t *idx, const float *obs,
                const float *actions, const float *returns, const float *old_values, float lr,
                float *stats, void *hip_stream) {
    const int rc = batch_ok("ce_a2c_step", l, n, m, idx, obs, actions, returns, old_values, stats);
    if (rc != CE_OK) return rc;
    CE_CLEAR_STALE_ERROR();
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    enqueue_grad(l, n, m, idx, obs, actions, 0, returns, old_values, 0, m, l->grad, stats, stream);
    enqueue_rmsprop(l, lr, stats, stream);
    CE_HIP(hipGetLastError());
    return CE_OK;
}

int ce_a2c_update(ce_a2c *l, int32_t k, int64_t rows, const float *obs, const float *actions,
                  int64_t action_stride_bytes, const float *values, int64_t value_stride_bytes,
                  const float *rewards, int64_t reward_stride_bytes, const uint8_t *dones,
                  int64_t done_stride_bytes, const float *last_values, float lr, float *stats,
                  void *hip_stream) {
    const std::string w("ce_a2c_update");
    const int rc = records_ok(w, k, rows, rewards, reward_stride_bytes, dones, done_stride_bytes,
                              last_values);
    if (rc != CE_OK) return rc;
    if (!obs) return fail(CE_EINVAL, w + ": null obs");
    if (!actions) return fail(CE_EINVAL, w + ": null actions");
    if (!values) return fail(CE_EINVAL, w + ": null values");
    if (!stats) return fail(CE_EINVAL, w + ": null stats");
    if (value_stride_bytes < rows * 4 || value_stride_bytes % 4 != 0)
        return fail(CE_EINVAL, w + ": value_stride_bytes must be a multiple of 4 of at least "
                                   "rows * 4");
    if (action_stride_bytes < rows * 4 || action_stride_bytes % 4 != 0)
        return fail(CE_EINVAL, w + ": action_stride_bytes must be a multiple of 4 of at least "
                                   "one record");
    if ((reinterpret_cast<uintptr_t>(actions) | reinterpret_cast<uintptr_t>(values)) & 3)
        return fail(CE_EINVAL, w + ": actions and values must be 4-byte aligned");
    if (!l) return fail(CE_EINVAL, w + ": null learner");
    if (action_stride_bytes < rows * l->plan.A * 4)
        return fail(CE_EINVAL, w + ": action_stride_bytes is shorter than one record (rows * "
                                   "act_dim * 4 = " + std::to_string(rows * l->plan.A * 4) + ")");
    CE_CLEAR_STALE_ERROR();
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const int64_t total = int64_t(k) * rows;
    if (total > l->ret_cap) {    // grows as needed; the steady state allocates nothing
        if (l->ret) CE_HIP(hipFree(l->ret));      // waits for the launches that read it
        l->ret = nullptr;
        l->ret_cap = 0;
        CE_HIP(hipMalloc(&l->ret, static_cast<size_t>(total) * sizeof(float)));
        l->ret_cap = total;
    }
    enqueue_returns(l, k, rows, rewards, reward_stride_bytes, dones, done_stride_bytes,
                    last_values, l->ret, stream);
    enqueue_grad(l, total, total, nullptr, obs, actions, action_stride_bytes / 4, l->ret, values,
                 value_stride_bytes / 4, rows, l->grad, stats, stream);
    enqueue_rmsprop(l, lr, stats, stream);
    CE_HIP(hipGetLastError());
    return CE_OK;
}

}  // extern "C"
