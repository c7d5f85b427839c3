// C-ABI implementation of the PPO2 learner (ce_ppo2_* in
// include/custom_envs_amd.h): Adam's moments, the step count and the advantage
// statistics on top of the shell both learners share (learner_host.h), and
// the launches [advantage statistics, gradient, reduce, finish, Adam, repack]
// on the caller's stream; under a gradient exchange (learner_host.h) the list
// splits into ce_ppo2_partial [moments' merge, gradient, partial reduce] and
// ce_ppo2_apply [combine, finish, Adam, repack] around the caller's
// all-gather.  Every argument check precedes the first HIP call,
// and the checks of the plain arguments precede the check of the handle, so
// they run without a device.
#include <hip/hip_runtime.h>

#include <cmath>
#include <new>
#include <string>

#include "learner_host.h"
#include "ppo2_kernels.h"

struct ce_ppo2 {
    ce_ppo2_config cfg{};
    long long t = 0;             // Adam steps taken
    float *m = nullptr, *v = nullptr, *advstat = nullptr;
    ce::LearnerCore core;
};

namespace ce {

void ppo2_launch_reduce(const Ppo2ReduceArgs &q, hipStream_t stream) {
    hipLaunchKernelGGL(ppo2_reduce_kernel, dim3((q.p.n_params + 255) / 256), dim3(256), 0, stream, q);
}

void ppo2_launch_partial(const Ppo2PartialArgs &q, hipStream_t stream) {
    hipLaunchKernelGGL(ppo2_partial_kernel, dim3((q.p.n_params + 255) / 256), dim3(256), 0, stream, q);
}

void ppo2_launch_combine(const Ppo2CombineArgs &q, hipStream_t stream) {
    hipLaunchKernelGGL(ppo2_combine_kernel, dim3((q.n_params + 255) / 256), dim3(256), 0, stream, q);
}

}  // namespace ce

namespace {

using ce::fail;

int config_ok(const char *who, const ce_ppo2_config *c) {
    const std::string w(who);
    if (!c) return fail(CE_EINVAL, w + ": null config");
    if (!(c->gamma >= 0.0f && c->gamma <= 1.0f)) return fail(CE_EINVAL, w + ": gamma must be in [0, 1]");
    if (!(c->lam >= 0.0f && c->lam <= 1.0f)) return fail(CE_EINVAL, w + ": lam must be in [0, 1]");
    if (!(c->cliprange > 0.0f)) return fail(CE_EINVAL, w + ": cliprange must be positive");
    if (std::isnan(c->cliprange_vf)) return fail(CE_EINVAL, w + ": cliprange_vf is not a number");
    if (!std::isfinite(c->ent_coef) || !std::isfinite(c->vf_coef))
        return fail(CE_EINVAL, w + ": ent_coef and vf_coef must be finite");
    if (std::isnan(c->max_grad_norm)) return fail(CE_EINVAL, w + ": max_grad_norm is not a number");
    if (!(c->lr > 0.0f)) return fail(CE_EINVAL, w + ": lr must be positive");
    if (!(c->beta1 >= 0.0f && c->beta1 < 1.0f)) return fail(CE_EINVAL, w + ": beta1 must be in [0, 1)");
    if (!(c->beta2 >= 0.0f && c->beta2 < 1.0f)) return fail(CE_EINVAL, w + ": beta2 must be in [0, 1)");
    if (!(c->eps > 0.0f)) return fail(CE_EINVAL, w + ": eps must be positive");
    if (c->grid_limit < 0) return fail(CE_EINVAL, w + ": grid_limit must not be negative");
    return CE_OK;
}

int batch_ok(const char *who, const ce_ppo2 *l, int64_t n, int64_t m, const int32_t *idx,
             const float *obs, const float *actions, const float *adv, const float *ret,
             const float *old_neglogp, const float *old_values, const float *stats) {
    const int rc = ce::learner_rows_ok(who, n, m, idx);
    if (rc != CE_OK) return rc;
    const auto null = [who](const char *what) { return fail(CE_EINVAL, std::string(who) + ": null " + what); };
    if (!obs) return null("obs");
    if (!actions) return null("actions");
    if (!adv) return null("advantages");
    if (!ret) return null("returns");
    if (!old_neglogp) return null("old_neglogp");
    if (!old_values) return null("old_values");
    if (!stats) return null("stats");
    if (!l) return null("learner");
    return CE_OK;
}

// [gradient] of n rows weighted 1 / n_total, normalised by l->advstat, into
// the slab; returns the grid
int enqueue_grad_kernel(const ce_ppo2 *l, int64_t n, int64_t n_total, int64_t m,
                        const int32_t *idx, const float *obs, const float *actions,
                        const float *adv, const float *ret, const float *old_neglogp,
                        const float *old_values, float cliprange, hipStream_t stream) {
    const ce_ppo2_config &c = l->cfg;
    ce::Ppo2GradArgs g{};
    ce::learner_fill_grad_args(g, l->core, c.vf_coef, n, n_total, m, idx, obs);
    g.cliprange = cliprange > 0.0f ? cliprange : c.cliprange;
    // a per-call cliprange moves the policy clip only
    g.cliprange_vf = c.cliprange_vf;
    g.actions = actions;
    g.adv = adv;
    g.ret = ret;
    g.old_neglogp = old_neglogp;
    g.old_values = old_values;
    g.advstat = l->advstat;
    // the one place the learner's kind picks its gradient kernel
    if (l->core.wide)
        hipLaunchKernelGGL(ce::ppo2_grad_wide_kernel, dim3(g.grid, 2), dim3(ce::kPpoBlock),
                           l->core.lds_bytes, stream, g);
    else
        hipLaunchKernelGGL(ce::ppo2_grad_kernel, dim3(g.grid, 2), dim3(ce::kPpoBlock),
                           l->core.lds_bytes, stream, g);
    return g.grid;
}

// [advantage statistics, gradient, reduce, finish] into grad / stats
void enqueue_grad(const ce_ppo2 *l, int64_t n, int64_t m, const int32_t *idx, const float *obs,
                  const float *actions, const float *adv, const float *ret,
                  const float *old_neglogp, const float *old_values, float cliprange,
                  float *grad, float *stats, hipStream_t stream) {
    const ce_ppo2_config &c = l->cfg;
    hipLaunchKernelGGL(ce::ppo2_advstat_kernel, dim3(1), dim3(ce::kPpoStatBlock), 0, stream,
                       static_cast<int>(n), static_cast<int>(m), idx, adv, c.normalize_adv,
                       l->advstat);
    const int grid = enqueue_grad_kernel(l, n, n, m, idx, obs, actions, adv, ret, old_neglogp,
                                         old_values, cliprange, stream);
    ce::learner_enqueue_reduce_finish<ce::ppo2_finish_kernel>(l->core, static_cast<int>(n), grid,
                                                              c.ent_coef, c.vf_coef, grad, stats,
                                                              stream);
}

// [Adam, repack] from the core's grad and the |grad|^2 in stats; one more step
void enqueue_adam(ce_ppo2 *l, float lr, const float *stats, hipStream_t stream) {
    const ce_ppo2_config &c = l->cfg;
    ce::LearnerCore &core = l->core;
    const long long t = ++l->t;
    const double lr_t = (lr > 0.0f ? lr : c.lr) * std::sqrt(1.0 - std::pow(double(c.beta2), double(t))) /
                        (1.0 - std::pow(double(c.beta1), double(t)));
    hipLaunchKernelGGL(ce::ppo2_adam_kernel, dim3((core.plan.n_params + 255) / 256), dim3(256), 0,
                       stream, core.plan.n_params, core.grad, stats, c.max_grad_norm,
                       static_cast<float>(lr_t), c.beta1, c.beta2,
                       static_cast<float>(1.0 - double(c.beta1)),
                       static_cast<float>(1.0 - double(c.beta2)), c.eps, core.params, l->m, l->v);
    ce::policy_repack(core.policy, core.params, stream);
}

// what ce_ppo2_create and ce_ppo2_create_wide share
int create(const char *who, bool wide, ce_policy *policy, const ce_ppo2_config *cfg, ce_ppo2 **out) {
    const std::string w(who);
    if (!out) return fail(CE_EINVAL, w + ": null output handle");
    *out = nullptr;
    int rc = config_ok(who, cfg);
    if (rc != CE_OK) return rc;
    if (!policy) return fail(CE_EINVAL, w + ": null policy");
    ce_ppo2 *l = new (std::nothrow) ce_ppo2();
    if (!l) return fail(CE_ENOMEM, w + ": host allocation failed");
    l->cfg = *cfg;
    auto bail = [&](int code) {
        ce_ppo2_destroy(l);
        return code;
    };
    rc = ce::learner_core_create(l->core, policy, cfg->grid_limit,
                                 wide ? reinterpret_cast<const void *>(ce::ppo2_grad_wide_kernel)
                                      : reinterpret_cast<const void *>(ce::ppo2_grad_kernel),
                                 bail, wide, who);
    if (rc != CE_OK) return rc;
    const size_t np = static_cast<size_t>(l->core.plan.n_params) * sizeof(float);
    CE_TRY(hipMalloc(&l->m, np));
    CE_TRY(hipMalloc(&l->v, np));
    CE_TRY(hipMalloc(&l->advstat, 2 * sizeof(float)));
    CE_TRY(hipMemset(l->m, 0, np));
    CE_TRY(hipMemset(l->v, 0, np));
    CE_TRY(hipDeviceSynchronize());
    *out = l;
    return CE_OK;
}

}  // namespace

extern "C" {

int ce_ppo2_create(ce_policy *policy, const ce_ppo2_config *cfg, ce_ppo2 **out) {
    return create("ce_ppo2_create", false, policy, cfg, out);
}

int ce_ppo2_create_wide(ce_policy *policy, const ce_ppo2_config *cfg, ce_ppo2 **out) {
    return create("ce_ppo2_create_wide", true, policy, cfg, out);
}

void ce_ppo2_destroy(ce_ppo2 *l) {
    if (!l) return;
    for (float *q : {l->m, l->v, l->advstat})
        if (q) (void)hipFree(q);
    ce::learner_core_destroy(l->core);
    delete l;
}

int ce_ppo2_set_params(ce_ppo2 *l, const float *flat, int64_t n, uint32_t flags,
                       void *hip_stream) {
    return ce::learner_set_params("ce_ppo2_set_params", l ? &l->core : nullptr, flat, n, flags,
                                  hip_stream);
}

int ce_ppo2_get_params(ce_ppo2 *l, float *flat, int64_t n, uint32_t flags, void *hip_stream) {
    return ce::learner_get_params("ce_ppo2_get_params", l ? &l->core : nullptr, flat, n, flags,
                                  hip_stream);
}

int ce_ppo2_get_opt_state(ce_ppo2 *l, float *m, float *v, int64_t n, int64_t *step,
                          uint32_t flags, void *hip_stream) {
    if (!step) return fail(CE_EINVAL, "ce_ppo2_get_opt_state: null step");
    const int rc = ce::learner_opt_state("ce_ppo2_get_opt_state", l ? &l->core : nullptr,
                                         l ? l->m : nullptr, l ? l->v : nullptr, "m", "v", m, v, n,
                                         false, flags, hip_stream);
    if (rc == CE_OK) *step = l->t;
    return rc;
}

int ce_ppo2_set_opt_state(ce_ppo2 *l, const float *m, const float *v, int64_t n, int64_t step,
                          uint32_t flags, void *hip_stream) {
    if (step < 0) return fail(CE_EINVAL, "ce_ppo2_set_opt_state: step must not be negative");
    const int rc = ce::learner_opt_state("ce_ppo2_set_opt_state", l ? &l->core : nullptr,
                                         l ? l->m : nullptr, l ? l->v : nullptr, "m", "v",
                                         const_cast<float *>(m), const_cast<float *>(v), n, true,
                                         flags, hip_stream);
    if (rc == CE_OK) l->t = step;
    return rc;
}

int ce_ppo2_gae(const ce_ppo2 *l, int32_t k, int64_t rows, const float *rewards,
                int64_t reward_stride_bytes, const uint8_t *dones, int64_t done_stride_bytes,
                const float *values, int64_t value_stride_bytes, const float *last_values,
                float *adv, float *ret, void *hip_stream) {
    const char *who = "ce_ppo2_gae";
    const auto bad = [who](const char *what) { return fail(CE_EINVAL, std::string(who) + what); };
    int rc = ce::learner_records_ok(who, k, rows, rewards, reward_stride_bytes, dones,
                                    done_stride_bytes, last_values, false);
    if (rc != CE_OK) return rc;
    if (!values) return bad(": null values");
    if (!adv || !ret) return bad(": null adv or ret output");
    if ((rc = ce::learner_stride_ok(who, "value", value_stride_bytes, rows)) != CE_OK) return rc;
    if (reinterpret_cast<uintptr_t>(values) & 3)
        return bad(": rewards and values must be 4-byte aligned");
    if (!l) return bad(": null learner");
    CE_CLEAR_STALE_ERROR();
    hipLaunchKernelGGL(ce::ppo2_gae_kernel, dim3(static_cast<unsigned>((rows + 255) / 256)),
                       dim3(256), 0, static_cast<hipStream_t>(hip_stream), k,
                       static_cast<int>(rows), reinterpret_cast<const char *>(rewards),
                       static_cast<long long>(reward_stride_bytes), dones,
                       static_cast<long long>(done_stride_bytes),
                       reinterpret_cast<const char *>(values),
                       static_cast<long long>(value_stride_bytes), last_values, l->cfg.gamma,
                       l->cfg.gamma * l->cfg.lam, adv, ret);
    CE_HIP(hipGetLastError());
    return CE_OK;
}

int ce_ppo2_grad(ce_ppo2 *l, int64_t n, int64_t m, const int32_t *idx, const float *obs,
                 const float *actions, const float *advantages, const float *returns,
                 const float *old_neglogp, const float *old_values, float cliprange,
                 float *grad, float *stats, void *hip_stream) {
    if (!grad) return fail(CE_EINVAL, "ce_ppo2_grad: null grad");
    const int rc = batch_ok("ce_ppo2_grad", l, n, m, idx, obs, actions, advantages, returns,
                            old_neglogp, old_values, stats);
    if (rc != CE_OK) return rc;
    CE_CLEAR_STALE_ERROR();
    enqueue_grad(l, n, m, idx, obs, actions, advantages, returns, old_neglogp, old_values,
                 cliprange, grad, stats, static_cast<hipStream_t>(hip_stream));
    CE_HIP(hipGetLastError());
    return CE_OK;
}

int ce_ppo2_step(ce_ppo2 *l, int64_t n, int64_t m, const int32_t *idx, const float *obs,
                 const float *actions, const float *advantages, const float *returns,
                 const float *old_neglogp, const float *old_values, float lr, float cliprange,
                 float *stats, void *hip_stream) {
    const int rc = batch_ok("ce_ppo2_step", l, n, m, idx, obs, actions, advantages, returns,
                            old_neglogp, old_values, stats);
    if (rc != CE_OK) return rc;
    CE_CLEAR_STALE_ERROR();
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    enqueue_grad(l, n, m, idx, obs, actions, advantages, returns, old_neglogp, old_values,
                 cliprange, l->core.grad, stats, stream);
    enqueue_adam(l, lr, stats, stream);
    CE_HIP(hipGetLastError());
    return CE_OK;
}

int64_t ce_learner_record_bytes(const ce_policy *policy) {
    if (!policy) {
        fail(CE_EINVAL, "ce_learner_record_bytes: null policy");
        return -1;
    }
    return int64_t(ce::ppo_record_doubles(ce::policy_plan(policy).n_params)) * 8;
}

int ce_ppo2_adv_moments(const ce_ppo2 *l, int64_t n, int64_t m, const int32_t *idx,
                        const float *advantages, double *out3, void *hip_stream) {
    const char *who = "ce_ppo2_adv_moments";
    const int rc = ce::learner_rows_ok(who, n, m, idx);
    if (rc != CE_OK) return rc;
    if (!advantages) return fail(CE_EINVAL, std::string(who) + ": null advantages");
    if (!out3) return fail(CE_EINVAL, std::string(who) + ": null output");
    if (reinterpret_cast<uintptr_t>(out3) & 7)
        return fail(CE_EINVAL, std::string(who) + ": the output must be 8-byte aligned");
    if (!l) return fail(CE_EINVAL, std::string(who) + ": null learner");
    CE_CLEAR_STALE_ERROR();
    hipLaunchKernelGGL(ce::ppo2_advmoments_kernel, dim3(1), dim3(ce::kPpoStatBlock), 0,
                       static_cast<hipStream_t>(hip_stream), static_cast<int>(n),
                       static_cast<int>(m), idx, advantages, out3);
    CE_HIP(hipGetLastError());
    return CE_OK;
}

int ce_ppo2_partial(ce_ppo2 *l, int64_t n, int64_t n_total, int64_t m, const int32_t *idx,
                    const float *obs, const float *actions, const float *advantages,
                    const float *returns, const float *old_neglogp, const float *old_values,
                    float cliprange, int32_t world, const double *moments, double *record,
                    void *hip_stream) {
    const char *who = "ce_ppo2_partial";
    int rc = ce::learner_rows_ok(who, n, m, idx);
    if (rc != CE_OK) return rc;
    if ((rc = ce::learner_partial_ok(who, n, n_total, record)) != CE_OK) return rc;
    if (world < 1 || world > ce::kLearnerMaxWorld)
        return fail(CE_EINVAL, std::string(who) + ": world must be in [1, 2^16], got " +
                                   std::to_string(world));
    if (reinterpret_cast<uintptr_t>(moments) & 7)
        return fail(CE_EINVAL, std::string(who) + ": the moments must be 8-byte aligned");
    // `record` stands in for stats in the null checks the entry points share
    rc = batch_ok(who, l, n, m, idx, obs, actions, advantages, returns, old_neglogp, old_values,
                  reinterpret_cast<const float *>(record));
    if (rc != CE_OK) return rc;
    if (l->cfg.normalize_adv && !moments)
        return fail(CE_EINVAL, std::string(who) + ": the learner normalises advantages and "
                                                  "got no moments");
    CE_CLEAR_STALE_ERROR();
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    if (l->cfg.normalize_adv)
        hipLaunchKernelGGL(ce::ppo2_advmerge_kernel, dim3(1), dim3(64), 0, stream, world, moments,
                           l->advstat);
    else
        hipLaunchKernelGGL(ce::ppo2_advstat_kernel, dim3(1), dim3(ce::kPpoStatBlock), 0, stream,
                           static_cast<int>(n), static_cast<int>(m), idx, advantages, 0,
                           l->advstat);
    const int grid = enqueue_grad_kernel(l, n, n_total, m, idx, obs, actions, advantages, returns,
                                         old_neglogp, old_values, cliprange, stream);
    ce::learner_enqueue_partial(l->core, static_cast<int>(n), grid, record, stream);
    CE_HIP(hipGetLastError());
    return CE_OK;
}

int ce_ppo2_combine(ce_ppo2 *l, int32_t world, const double *records, int64_t n_total,
                    float *grad, float *stats, void *hip_stream) {
    const char *who = "ce_ppo2_combine";
    const int rc = ce::learner_apply_ok(who, world, records, n_total, stats);
    if (rc != CE_OK) return rc;
    if (!grad) return fail(CE_EINVAL, std::string(who) + ": null grad");
    if (!l) return fail(CE_EINVAL, std::string(who) + ": null learner");
    CE_CLEAR_STALE_ERROR();
    ce::learner_enqueue_combine_finish<ce::ppo2_finish_kernel>(
        l->core, world, records, n_total, l->cfg.ent_coef, l->cfg.vf_coef, grad, stats,
        static_cast<hipStream_t>(hip_stream));
    CE_HIP(hipGetLastError());
    return CE_OK;
}

int ce_ppo2_apply(ce_ppo2 *l, int32_t world, const double *records, int64_t n_total, float lr,
                  float *stats, void *hip_stream) {
    const char *who = "ce_ppo2_apply";
    const int rc = ce::learner_apply_ok(who, world, records, n_total, stats);
    if (rc != CE_OK) return rc;
    if (!l) return fail(CE_EINVAL, std::string(who) + ": null learner");
    CE_CLEAR_STALE_ERROR();
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    ce::learner_enqueue_combine_finish<ce::ppo2_finish_kernel>(
        l->core, world, records, n_total, l->cfg.ent_coef, l->cfg.vf_coef, l->core.grad, stats,
        stream);
    enqueue_adam(l, lr, stats, stream);
    CE_HIP(hipGetLastError());
    return CE_OK;
}

}  // extern "C"
