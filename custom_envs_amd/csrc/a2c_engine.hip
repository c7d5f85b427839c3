// C-ABI implementation of the A2C learner (ce_a2c_* in
// include/custom_envs_amd.h): RMSProp's ms and mom and the returns buffer of
// ce_a2c_update on top of the shell both learners share (learner_host.h), and
// the launches [gradient, reduce, finish, RMSProp, repack] -- ce_a2c_update:
// the returns scan first, the gradient on the rollout records in place -- on
// the caller's stream; under a gradient exchange (learner_host.h) the list
// splits into ce_a2c_partial / ce_a2c_update_partial [(returns,) gradient,
// partial reduce] and ce_a2c_apply [combine, finish, RMSProp, repack] around
// the caller's all-gather.  Every argument check precedes the first HIP call, and
// the checks of the plain arguments precede the check of the handle, so they
// run without a device.
#include <hip/hip_runtime.h>

#include <cmath>
#include <new>
#include <string>
#include <vector>

#include "a2c_kernels.h"
#include "learner_host.h"

struct ce_a2c {
    ce_a2c_config cfg{};
    float *ms = nullptr, *mom = nullptr;
    float *ret = nullptr;        // ce_a2c_update's returns, [ret_cap]
    int64_t ret_cap = 0;
    ce::LearnerCore core;
};

namespace {

using ce::fail;

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
    const int rc = ce::learner_rows_ok(who, n, m, idx);
    if (rc != CE_OK) return rc;
    const auto null = [who](const char *what) { return fail(CE_EINVAL, std::string(who) + ": null " + what); };
    if (!obs) return null("obs");
    if (!actions) return null("actions");
    if (!ret) return null("returns");
    if (!old_values) return null("old_values");
    if (!stats) return null("stats");
    if (!l) return null("learner");
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

// [gradient] of n rows weighted 1 / n_total into the slab; returns the grid.
// Row s of the m-row batch is row s % rec_rows of record s / rec_rows of
// actions / old_values.
int enqueue_grad_kernel(const ce_a2c *l, int64_t n, int64_t n_total, int64_t m,
                        const int32_t *idx, const float *obs, const float *actions,
                        int64_t action_stride, const float *ret, const float *old_values,
                        int64_t value_stride, int64_t rec_rows, hipStream_t stream) {
    ce::A2cGradArgs g{};
    ce::learner_fill_grad_args(g, l->core, l->cfg.vf_coef, n, n_total, m, idx, obs);
    g.rec_rows = static_cast<int>(rec_rows);
    g.action_stride = action_stride;
    g.value_stride = value_stride;
    g.actions = actions;
    g.ret = ret;
    g.old_values = old_values;
    // the one place the learner's kind picks its gradient kernel
    if (l->core.wide)
        hipLaunchKernelGGL(ce::a2c_grad_wide_kernel, dim3(g.grid, 2), dim3(ce::kPpoBlock),
                           l->core.lds_bytes, stream, g);
    else
        hipLaunchKernelGGL(ce::a2c_grad_kernel, dim3(g.grid, 2), dim3(ce::kPpoBlock),
                           l->core.lds_bytes, stream, g);
    return g.grid;
}

// [gradient, reduce, finish] into grad / stats
void enqueue_grad(const ce_a2c *l, int64_t n, int64_t m, const int32_t *idx, const float *obs,
                  const float *actions, int64_t action_stride, const float *ret,
                  const float *old_values, int64_t value_stride, int64_t rec_rows, float *grad,
                  float *stats, hipStream_t stream) {
    const int grid = enqueue_grad_kernel(l, n, n, m, idx, obs, actions, action_stride, ret,
                                         old_values, value_stride, rec_rows, stream);
    ce::learner_enqueue_reduce_finish<ce::a2c_finish_kernel>(l->core, static_cast<int>(n), grid,
                                                             l->cfg.ent_coef, l->cfg.vf_coef, grad,
                                                             stats, stream);
}

// The checks of ce_a2c_update and ce_a2c_update_partial but the handle's, and
// then the handle's own (the action stride against act_dim).
int update_ok(const char *who, const ce_a2c *l, int32_t k, int64_t rows, const float *obs,
              const float *actions, int64_t action_stride_bytes, const float *values,
              int64_t value_stride_bytes, const float *rewards, int64_t reward_stride_bytes,
              const uint8_t *dones, int64_t done_stride_bytes, const float *last_values,
              const void *out, const char *out_name) {
    const auto bad = [who](const std::string &what) { return fail(CE_EINVAL, who + what); };
    int rc = ce::learner_records_ok(who, k, rows, rewards, reward_stride_bytes, dones,
                                    done_stride_bytes, last_values, true);
    if (rc != CE_OK) return rc;
    if (!obs) return bad(": null obs");
    if (!actions) return bad(": null actions");
    if (!values) return bad(": null values");
    if (!out) return bad(std::string(": null ") + out_name);
    if ((rc = ce::learner_stride_ok(who, "value", value_stride_bytes, rows)) != CE_OK) return rc;
    if (action_stride_bytes < rows * 4 || action_stride_bytes % 4 != 0)
        return bad(": action_stride_bytes must be a multiple of 4 of at least one record");
    if ((reinterpret_cast<uintptr_t>(actions) | reinterpret_cast<uintptr_t>(values)) & 3)
        return bad(": actions and values must be 4-byte aligned");
    if (!l) return bad(": null learner");
    if (action_stride_bytes < rows * l->core.plan.A * 4)
        return bad(": action_stride_bytes is shorter than one record (rows * act_dim * 4 = " +
                   std::to_string(rows * l->core.plan.A * 4) + ")");
    return CE_OK;
}

// the returns buffer for `total` rows: grows as needed; the steady state
// allocates nothing
int reserve_returns(ce_a2c *l, int64_t total) {
    if (total <= l->ret_cap) return CE_OK;
    if (l->ret) CE_HIP(hipFree(l->ret));      // waits for the launches that read it
    l->ret = nullptr;
    l->ret_cap = 0;
    CE_HIP(hipMalloc(&l->ret, static_cast<size_t>(total) * sizeof(float)));
    l->ret_cap = total;
    return CE_OK;
}

// [RMSProp, repack] from the core's grad and the |grad|^2 in stats
void enqueue_rmsprop(ce_a2c *l, float lr, const float *stats, hipStream_t stream) {
    const ce_a2c_config &c = l->cfg;
    const ce::LearnerCore &core = l->core;
    hipLaunchKernelGGL(ce::a2c_rmsprop_kernel, dim3((core.plan.n_params + 255) / 256), dim3(256), 0,
                       stream, core.plan.n_params, core.grad, stats, c.max_grad_norm,
                       lr > 0.0f ? lr : c.lr, c.alpha, static_cast<float>(1.0 - double(c.alpha)),
                       c.eps, c.momentum, core.params, l->ms, l->mom);
    ce::policy_repack(core.policy, core.params, stream);
}

// what ce_a2c_create and ce_a2c_create_wide share
int create(const char *who, bool wide, ce_policy *policy, const ce_a2c_config *cfg, ce_a2c **out) {
    const std::string w(who);
    if (!out) return fail(CE_EINVAL, w + ": null output handle");
    *out = nullptr;
    int rc = config_ok(who, cfg);
    if (rc != CE_OK) return rc;
    if (!policy) return fail(CE_EINVAL, w + ": null policy");
    ce_a2c *l = new (std::nothrow) ce_a2c();
    if (!l) return fail(CE_ENOMEM, w + ": host allocation failed");
    l->cfg = *cfg;
    auto bail = [&](int code) {
        ce_a2c_destroy(l);
        return code;
    };
    rc = ce::learner_core_create(l->core, policy, cfg->grid_limit,
                                 wide ? reinterpret_cast<const void *>(ce::a2c_grad_wide_kernel)
                                      : reinterpret_cast<const void *>(ce::a2c_grad_kernel),
                                 bail, wide, who);
    if (rc != CE_OK) return rc;
    const int n_params = l->core.plan.n_params;
    const size_t np = static_cast<size_t>(n_params) * sizeof(float);
    CE_TRY(hipMalloc(&l->ms, np));
    CE_TRY(hipMalloc(&l->mom, np));
    const std::vector<float> ones(n_params, 1.0f);        // TF's slot initialiser of ms
    CE_TRY(hipMemcpy(l->ms, ones.data(), np, hipMemcpyHostToDevice));
    CE_TRY(hipMemset(l->mom, 0, np));
    CE_TRY(hipDeviceSynchronize());
    *out = l;
    return CE_OK;
}

}  // namespace

extern "C" {

int ce_a2c_create(ce_policy *policy, const ce_a2c_config *cfg, ce_a2c **out) {
    return create("ce_a2c_create", false, policy, cfg, out);
}

int ce_a2c_create_wide(ce_policy *policy, const ce_a2c_config *cfg, ce_a2c **out) {
    return create("ce_a2c_create_wide", true, policy, cfg, out);
}

void ce_a2c_destroy(ce_a2c *l) {
    if (!l) return;
    for (float *q : {l->ms, l->mom, l->ret})
        if (q) (void)hipFree(q);
    ce::learner_core_destroy(l->core);
    delete l;
}

int ce_a2c_set_params(ce_a2c *l, const float *flat, int64_t n, uint32_t flags, void *hip_stream) {
    return ce::learner_set_params("ce_a2c_set_params", l ? &l->core : nullptr, flat, n, flags,
                                  hip_stream);
}

int ce_a2c_get_params(ce_a2c *l, float *flat, int64_t n, uint32_t flags, void *hip_stream) {
    return ce::learner_get_params("ce_a2c_get_params", l ? &l->core : nullptr, flat, n, flags,
                                  hip_stream);
}

int ce_a2c_get_opt_state(ce_a2c *l, float *ms, float *mom, int64_t n, int64_t *step,
                         uint32_t flags, void *hip_stream) {
    if (!step) return fail(CE_EINVAL, "ce_a2c_get_opt_state: null step");
    const int rc = ce::learner_opt_state("ce_a2c_get_opt_state", l ? &l->core : nullptr,
                                         l ? l->ms : nullptr, l ? l->mom : nullptr, "ms", "mom", ms,
                                         mom, n, false, flags, hip_stream);
    if (rc == CE_OK) *step = 0;      // RMSProp keeps no counter
    return rc;
}

int ce_a2c_set_opt_state(ce_a2c *l, const float *ms, const float *mom, int64_t n, int64_t step,
                         uint32_t flags, void *hip_stream) {
    if (step != 0)
        return fail(CE_EINVAL, "ce_a2c_set_opt_state: RMSProp keeps no counter, step must be 0");
    return ce::learner_opt_state("ce_a2c_set_opt_state", l ? &l->core : nullptr,
                                 l ? l->ms : nullptr, l ? l->mom : nullptr, "ms", "mom",
                                 const_cast<float *>(ms), const_cast<float *>(mom), n, true, flags,
                                 hip_stream);
}

int ce_a2c_returns(const ce_a2c *l, int32_t k, int64_t rows, const float *rewards,
                   int64_t reward_stride_bytes, const uint8_t *dones, int64_t done_stride_bytes,
                   const float *last_values, float *ret, void *hip_stream) {
    const char *who = "ce_a2c_returns";
    const int rc = ce::learner_records_ok(who, k, rows, rewards, reward_stride_bytes, dones,
                                          done_stride_bytes, last_values, true);
    if (rc != CE_OK) return rc;
    if (!ret) return fail(CE_EINVAL, std::string(who) + ": null ret output");
    if (!l) return fail(CE_EINVAL, std::string(who) + ": null learner");
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
    enqueue_grad(l, n, m, idx, obs, actions, 0, returns, old_values, 0, m, l->core.grad, stats,
                 stream);
    enqueue_rmsprop(l, lr, stats, stream);
    CE_HIP(hipGetLastError());
    return CE_OK;
}

int ce_a2c_update(ce_a2c *l, int32_t k, int64_t rows, const float *obs, const float *actions,
                  int64_t action_stride_bytes, const float *values, int64_t value_stride_bytes,
                  const float *rewards, int64_t reward_stride_bytes, const uint8_t *dones,
                  int64_t done_stride_bytes, const float *last_values, float lr, float *stats,
                  void *hip_stream) {
    int rc = update_ok("ce_a2c_update", l, k, rows, obs, actions, action_stride_bytes, values,
                       value_stride_bytes, rewards, reward_stride_bytes, dones, done_stride_bytes,
                       last_values, stats, "stats");
    if (rc != CE_OK) return rc;
    CE_CLEAR_STALE_ERROR();
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const int64_t total = int64_t(k) * rows;
    if ((rc = reserve_returns(l, total)) != CE_OK) return rc;
    enqueue_returns(l, k, rows, rewards, reward_stride_bytes, dones, done_stride_bytes,
                    last_values, l->ret, stream);
    enqueue_grad(l, total, total, nullptr, obs, actions, action_stride_bytes / 4, l->ret, values,
                 value_stride_bytes / 4, rows, l->core.grad, stats, stream);
    enqueue_rmsprop(l, lr, stats, stream);
    CE_HIP(hipGetLastError());
    return CE_OK;
}

int ce_a2c_partial(ce_a2c *l, int64_t n, int64_t n_total, int64_t m, const int32_t *idx,
                   const float *obs, const float *actions, const float *returns,
                   const float *old_values, double *record, void *hip_stream) {
    const char *who = "ce_a2c_partial";
    int rc = ce::learner_rows_ok(who, n, m, idx);
    if (rc != CE_OK) return rc;
    if ((rc = ce::learner_partial_ok(who, n, n_total, record)) != CE_OK) return rc;
    // `record` stands in for stats in the null checks the entry points share
    rc = batch_ok(who, l, n, m, idx, obs, actions, returns, old_values,
                  reinterpret_cast<const float *>(record));
    if (rc != CE_OK) return rc;
    CE_CLEAR_STALE_ERROR();
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const int grid = enqueue_grad_kernel(l, n, n_total, m, idx, obs, actions, 0, returns,
                                         old_values, 0, m, stream);
    ce::learner_enqueue_partial(l->core, static_cast<int>(n), grid, record, stream);
    CE_HIP(hipGetLastError());
    return CE_OK;
}

int ce_a2c_update_partial(ce_a2c *l, int32_t k, int64_t rows, int64_t n_total, const float *obs,
                          const float *actions, int64_t action_stride_bytes, const float *values,
                          int64_t value_stride_bytes, const float *rewards,
                          int64_t reward_stride_bytes, const uint8_t *dones,
                          int64_t done_stride_bytes, const float *last_values, double *record,
                          void *hip_stream) {
    const char *who = "ce_a2c_update_partial";
    int rc = ce::learner_records_ok(who, k, rows, rewards, reward_stride_bytes, dones,
                                    done_stride_bytes, last_values, true);
    if (rc != CE_OK) return rc;
    const int64_t total = int64_t(k) * rows;
    if ((rc = ce::learner_partial_ok(who, total, n_total, record)) != CE_OK) return rc;
    rc = update_ok(who, l, k, rows, obs, actions, action_stride_bytes, values, value_stride_bytes,
                   rewards, reward_stride_bytes, dones, done_stride_bytes, last_values, record,
                   "record");
    if (rc != CE_OK) return rc;
    CE_CLEAR_STALE_ERROR();
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    if ((rc = reserve_returns(l, total)) != CE_OK) return rc;
    enqueue_returns(l, k, rows, rewards, reward_stride_bytes, dones, done_stride_bytes,
                    last_values, l->ret, stream);
    const int grid = enqueue_grad_kernel(l, total, n_total, total, nullptr, obs, actions,
                                         action_stride_bytes / 4, l->ret, values,
                                         value_stride_bytes / 4, rows, stream);
    ce::learner_enqueue_partial(l->core, static_cast<int>(total), grid, record, stream);
    CE_HIP(hipGetLastError());
    return CE_OK;
}

int ce_a2c_combine(ce_a2c *l, int32_t world, const double *records, int64_t n_total, float *grad,
                   float *stats, void *hip_stream) {
    const char *who = "ce_a2c_combine";
    const int rc = ce::learner_apply_ok(who, world, records, n_total, stats);
    if (rc != CE_OK) return rc;
    if (!grad) return fail(CE_EINVAL, std::string(who) + ": null grad");
    if (!l) return fail(CE_EINVAL, std::string(who) + ": null learner");
    CE_CLEAR_STALE_ERROR();
    ce::learner_enqueue_combine_finish<ce::a2c_finish_kernel>(
        l->core, world, records, n_total, l->cfg.ent_coef, l->cfg.vf_coef, grad, stats,
        static_cast<hipStream_t>(hip_stream));
    CE_HIP(hipGetLastError());
    return CE_OK;
}

int ce_a2c_apply(ce_a2c *l, int32_t world, const double *records, int64_t n_total, float lr,
                 float *stats, void *hip_stream) {
    const char *who = "ce_a2c_apply";
    const int rc = ce::learner_apply_ok(who, world, records, n_total, stats);
    if (rc != CE_OK) return rc;
    if (!l) return fail(CE_EINVAL, std::string(who) + ": null learner");
    CE_CLEAR_STALE_ERROR();
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    ce::learner_enqueue_combine_finish<ce::a2c_finish_kernel>(
        l->core, world, records, n_total, l->cfg.ent_coef, l->cfg.vf_coef, l->core.grad, stats,
        stream);
    enqueue_rmsprop(l, lr, stats, stream);
    CE_HIP(hipGetLastError());
    return CE_OK;
}

}  // extern "C"
