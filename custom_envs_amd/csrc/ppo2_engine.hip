// C-ABI implementation of the PPO2 learner (ce_ppo2_* in
// include/custom_envs_amd.h): owns the master flat parameters, Adam's moments,
// the step count and the partial slab of ppo2_grad_kernel, and enqueues
// [advantage statistics, gradient, reduce, finish, Adam, repack] on the
// caller's stream.  Every argument check precedes the first HIP call, and the
// checks of the plain arguments precede the check of the handle, so they run
// without a device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <string>

#include "common.h"
#include "policy_engine.h"
#include "ppo2_kernels.h"

struct ce_ppo2 {
    ce_ppo2_config cfg{};
    ce_policy *policy = nullptr;
    ce::PolicyPlan plan{};
    int grid_max = 0;            // workgroups per network the slab holds
    int n_sq = 0;                // blocks of ppo2_reduce_kernel
    int w_floats = 0, act_floats = 0;
    size_t lds_bytes = 0;
    long long t = 0;             // Adam steps taken
    float *params = nullptr, *m = nullptr, *v = nullptr, *grad = nullptr;
    float *slab = nullptr, *advstat = nullptr;
    double *stat_slab = nullptr, *sq = nullptr;
};

namespace ce {

void ppo2_launch_reduce(const Ppo2ReduceArgs &q, hipStream_t stream) {
    hipLaunchKernelGGL(ppo2_reduce_kernel, dim3((q.p.n_params + 255) / 256), dim3(256), 0, stream, q);
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
    const std::string w(who);
    if (n < 1) return fail(CE_EINVAL, w + ": n must be at least 1, got " + std::to_string(n));
    if (m < 1 || m > (int64_t(1) << 24))
        return fail(CE_EINVAL, w + ": m must be in [1, 2^24], got " + std::to_string(m));
    if (n > (int64_t(1) << 24)) return fail(CE_EINVAL, w + ": n must be at most 2^24");
    if (!idx && n > m)
        return fail(CE_EINVAL, w + ": n exceeds m and there is no idx to gather by");
    if (!obs) return fail(CE_EINVAL, w + ": null obs");
    if (!actions) return fail(CE_EINVAL, w + ": null actions");
    if (!adv) return fail(CE_EINVAL, w + ": null advantages");
    if (!ret) return fail(CE_EINVAL, w + ": null returns");
    if (!old_neglogp) return fail(CE_EINVAL, w + ": null old_neglogp");
    if (!old_values) return fail(CE_EINVAL, w + ": null old_values");
    if (!stats) return fail(CE_EINVAL, w + ": null stats");
    if (!l) return fail(CE_EINVAL, w + ": null learner");
    return CE_OK;
}

void repack(const ce_ppo2 *l, hipStream_t stream) {
    ce::policy_repack(l->policy, l->params, stream);
}

// [advantage statistics, gradient, reduce, finish] into grad / stats
void enqueue_grad(const ce_ppo2 *l, int64_t n, int64_t m, const int32_t *idx, const float *obs,
                  const float *actions, const float *adv, const float *ret,
                  const float *old_neglogp, const float *old_values, float cliprange,
                  float *grad, float *stats, hipStream_t stream) {
    const ce_ppo2_config &c = l->cfg;
    const ce::PolicyPlan &pa = l->plan;
    hipLaunchKernelGGL(ce::ppo2_advstat_kernel, dim3(1), dim3(ce::kPpoStatBlock), 0, stream,
                       static_cast<int>(n), static_cast<int>(m), idx, adv, c.normalize_adv,
                       l->advstat);
    ce::Ppo2GradArgs g{};
    g.p = pa;
    g.n = static_cast<int>(n);
    g.m = static_cast<int>(m);
    g.tiles = static_cast<int>((n + ce::kPpoTile - 1) / ce::kPpoTile);
    g.grid = std::min(g.tiles, l->grid_max);
    g.img_floats = l->plan.img_floats;
    g.w_floats = l->w_floats;
    g.act_floats = l->act_floats;
    g.cliprange = cliprange > 0.0f ? cliprange : c.cliprange;
    // a per-call cliprange moves the policy clip only
    g.cliprange_vf = c.cliprange_vf;
    g.vf_coef = c.vf_coef;
    g.idx = idx;
    g.obs = obs;
    g.actions = actions;
    g.adv = adv;
    g.ret = ret;
    g.old_neglogp = old_neglogp;
    g.old_values = old_values;
    g.advstat = l->advstat;
    g.slab = l->slab;
    g.stat_slab = l->stat_slab;
    hipLaunchKernelGGL(ce::ppo2_grad_kernel, dim3(g.grid, 2), dim3(ce::kPpoBlock), l->lds_bytes,
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
    f.img = l->plan.img;
    f.stat_slab = l->stat_slab;
    f.sq = l->sq;
    f.stats = stats;
    hipLaunchKernelGGL(ce::ppo2_finish_kernel, dim3(1), dim3(256), 0, stream, f);
}

}  // namespace

extern "C" {

int ce_ppo2_create(ce_policy *policy, const ce_ppo2_config *cfg, ce_ppo2 **out) {
    if (!out) return fail(CE_EINVAL, "ce_ppo2_create: null output handle");
    *out = nullptr;
    int rc = config_ok("ce_ppo2_create", cfg);
    if (rc != CE_OK) return rc;
    if (!policy) return fail(CE_EINVAL, "ce_ppo2_create: null policy");
    ce_ppo2 *l = new (std::nothrow) ce_ppo2();
    if (!l) return fail(CE_ENOMEM, "ce_ppo2_create: host allocation failed");
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
    l->n_sq = (l->plan.n_params + 255) / 256;
    auto bail = [&](int code) {
        ce_ppo2_destroy(l);
        return code;
    };
#define CE_TRY(call)                                                           \
    do {                                                                       \
        hipError_t err_ = (call);                                              \
        if (err_ != hipSuccess)                                                \
            return bail(fail(CE_EHIP, std::string(#call " failed: ") +         \
                                          hipGetErrorString(err_)));           \
    } while (0)
    CE_TRY(hipSetDevice(l->plan.device));
    hipDeviceProp_t prop;
    CE_TRY(hipGetDeviceProperties(&prop, l->plan.device));
    l->grid_max = cfg->grid_limit > 0 ? cfg->grid_limit : std::max(1, prop.multiProcessorCount);
    CE_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(ce::ppo2_grad_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize,
                               static_cast<int>(ce::kPpoMaxLdsBytes)));   // the limits' need
    const size_t np = static_cast<size_t>(l->plan.n_params) * sizeof(float);
    CE_TRY(hipMalloc(&l->params, np));
    CE_TRY(hipMalloc(&l->m, np));
    CE_TRY(hipMalloc(&l->v, np));
    CE_TRY(hipMalloc(&l->grad, np));
    CE_TRY(hipMalloc(&l->slab, static_cast<size_t>(l->grid_max) * l->plan.img_floats * sizeof(float)));
    CE_TRY(hipMalloc(&l->stat_slab, static_cast<size_t>(l->grid_max) * 2 * ce::kPpoRowStats * sizeof(double)));
    CE_TRY(hipMalloc(&l->sq, static_cast<size_t>(l->n_sq) * sizeof(double)));
    CE_TRY(hipMalloc(&l->advstat, 2 * sizeof(float)));
    CE_TRY(hipMemset(l->params, 0, np));
    CE_TRY(hipMemset(l->m, 0, np));
    CE_TRY(hipMemset(l->v, 0, np));
    CE_TRY(hipDeviceSynchronize());
#undef CE_TRY
    *out = l;
    return CE_OK;
}

void ce_ppo2_destroy(ce_ppo2 *l) {
    if (!l) return;
    for (void *q : {static_cast<void *>(l->params), static_cast<void *>(l->m),
                    static_cast<void *>(l->v), static_cast<void *>(l->grad),
                    static_cast<void *>(l->slab), static_cast<void *>(l->advstat),
                    static_cast<void *>(l->stat_slab), static_cast<void *>(l->sq)})
        if (q) (void)hipFree(q);
    delete l;
}

int ce_ppo2_set_params(ce_ppo2 *l, const float *flat, int64_t n, uint32_t flags,
                       void *hip_stream) {
    if (!flat) return fail(CE_EINVAL, "ce_ppo2_set_params: null parameter vector");
    if (!l) return fail(CE_EINVAL, "ce_ppo2_set_params: null learner");
    if (n != l->plan.n_params)
        return fail(CE_EINVAL, "ce_ppo2_set_params: got " + std::to_string(n) +
                                   " parameters, the policy has " + std::to_string(l->plan.n_params));
    CE_CLEAR_STALE_ERROR();
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const bool dev = (flags & CE_PTR_DEVICE) != 0;
    CE_HIP(hipMemcpyAsync(l->params, flat, n * sizeof(float),
                          dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream));
    if (!dev) CE_HIP(hipStreamSynchronize(stream));   // `flat` may be pageable
    repack(l, stream);
    CE_HIP(hipGetLastError());
    if (!dev) CE_HIP(hipStreamSynchronize(stream));
    return CE_OK;
}

int ce_ppo2_get_params(ce_ppo2 *l, float *flat, int64_t n, uint32_t flags, void *hip_stream) {
    if (!flat) return fail(CE_EINVAL, "ce_ppo2_get_params: null parameter vector");
    if (!l) return fail(CE_EINVAL, "ce_ppo2_get_params: null learner");
    if (n != l->plan.n_params)
        return fail(CE_EINVAL, "ce_ppo2_get_params: got room for " + std::to_string(n) +
                                   " parameters, the policy has " + std::to_string(l->plan.n_params));
    CE_CLEAR_STALE_ERROR();
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const bool dev = (flags & CE_PTR_DEVICE) != 0;
    CE_HIP(hipMemcpyAsync(flat, l->params, n * sizeof(float),
                          dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream));
    repack(l, stream);
    CE_HIP(hipGetLastError());
    if (!dev) CE_HIP(hipStreamSynchronize(stream));
    return CE_OK;
}

int ce_ppo2_gae(const ce_ppo2 *l, int32_t k, int64_t rows, const float *rewards,
                int64_t reward_stride_bytes, const uint8_t *dones, int64_t done_stride_bytes,
                const float *values, int64_t value_stride_bytes, const float *last_values,
                float *adv, float *ret, void *hip_stream) {
    const std::string w("ce_ppo2_gae");
    if (k < 1) return fail(CE_EINVAL, w + ": k must be at least 1, got " + std::to_string(k));
    if (rows < 1 || rows > (int64_t(1) << 24))
        return fail(CE_EINVAL, w + ": rows must be in [1, 2^24], got " + std::to_string(rows));
    if (!rewards) return fail(CE_EINVAL, w + ": null rewards");
    if (!dones) return fail(CE_EINVAL, w + ": null dones");
    if (!values) return fail(CE_EINVAL, w + ": null values");
    if (!last_values) return fail(CE_EINVAL, w + ": null last_values");
    if (!adv || !ret) return fail(CE_EINVAL, w + ": null adv or ret output");
    if (reward_stride_bytes < rows * 4 || reward_stride_bytes % 4 != 0)
        return fail(CE_EINVAL, w + ": reward_stride_bytes must be a multiple of 4 of at least "
                                   "rows * 4");
    if (value_stride_bytes < rows * 4 || value_stride_bytes % 4 != 0)
        return fail(CE_EINVAL, w + ": value_stride_bytes must be a multiple of 4 of at least "
                                   "rows * 4");
    if (done_stride_bytes < rows) return fail(CE_EINVAL, w + ": done_stride_bytes must be at least rows");
    if ((reinterpret_cast<uintptr_t>(rewards) | reinterpret_cast<uintptr_t>(values)) & 3)
        return fail(CE_EINVAL, w + ": rewards and values must be 4-byte aligned");
    if (!l) return fail(CE_EINVAL, w + ": null learner");
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
                 cliprange, l->grad, stats, stream);
    const ce_ppo2_config &c = l->cfg;
    const long long t = ++l->t;
    const double lr_t = (lr > 0.0f ? lr : c.lr) * std::sqrt(1.0 - std::pow(double(c.beta2), double(t))) /
                        (1.0 - std::pow(double(c.beta1), double(t)));
    hipLaunchKernelGGL(ce::ppo2_adam_kernel, dim3((l->plan.n_params + 255) / 256), dim3(256), 0,
                       stream, l->plan.n_params, l->grad, stats, c.max_grad_norm,
                       static_cast<float>(lr_t), c.beta1, c.beta2,
                       static_cast<float>(1.0 - double(c.beta1)),
                       static_cast<float>(1.0 - double(c.beta2)), c.eps, l->params, l->m, l->v);
    repack(l, stream);
    CE_HIP(hipGetLastError());
    return CE_OK;
}

}  // extern "C"
