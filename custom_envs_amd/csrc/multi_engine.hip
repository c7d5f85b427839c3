// C-ABI implementation of the MultiOptLRs-v0 engine (ce_multi_* in
// include/custom_envs_amd.h).  Same conventions as engine.hip: the engine
// owns the struct-of-arrays state; host mode stages actions/outputs through
// pinned buffers and synchronises; CE_PTR_DEVICE calls are stream-ordered
// (engine_host.h holds those bodies).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "engine_host.h"
#include "multiopt_kernels.h"

namespace {

using ce::fail;

using MultiFn = void (*)(const ce::MultiArgs &, hipStream_t);

// one lane per (env, agent): E groups of Group<P>::G lanes
template <int P>
int multi_grid(int E) {
    const long lanes = static_cast<long>(E) * ce::Group<P>::G;
    return static_cast<int>((lanes + ce::kMultiBlock - 1) / ce::kMultiBlock);
}
template <int P>
void launch_multi_step(const ce::MultiArgs &a, hipStream_t s) {
    // LDS stage of the observation rows: per wave 64/G envs x P rows x 3H
    const size_t lds = a.H <= ce::kMultiStageH
                           ? ce::kMultiBlock / 64 * (64 / ce::Group<P>::G) * P * 3 * a.H * sizeof(float)
                           : 0;
    if (a.H == 5)   // the reference's default history (multioptlrs.py:39)
        hipLaunchKernelGGL((ce::multi_step_kernel<P, 5>), dim3(multi_grid<P>(a.E)),
                           dim3(ce::kMultiBlock), lds, s, a);
    else
        hipLaunchKernelGGL((ce::multi_step_kernel<P, 0>), dim3(multi_grid<P>(a.E)),
                           dim3(ce::kMultiBlock), lds, s, a);
}
// K steps in one launch (multi_persist5_kernel: five waves per 64 lanes): the
// reference default history H = 5 only, the compile-time instance it needs
template <int P>
void launch_multi_persist(const ce::MultiArgs &a, int k, long long act_stride, long long out_step,
                          hipStream_t s) {
    const long lanes = static_cast<long>(a.E) * ce::Group<P>::G;
    const dim3 grid(static_cast<int>((lanes + 63) / 64));
    hipLaunchKernelGGL((ce::multi_persist5_kernel<P, 5>), grid, dim3(320), 0, s, a, k, act_stride,
                       out_step);
}
template <int P>
void launch_multi_reset(const ce::MultiArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(ce::multi_reset_kernel<P>, dim3(multi_grid<P>(a.E)),
                       dim3(ce::kMultiBlock), 0, s, a);
}

using MultiPersistFn = void (*)(const ce::MultiArgs &, int, long long, long long, hipStream_t);

struct MultiEntry {
    int P;
    MultiFn step, reset;
    MultiPersistFn persist;
};

// every even dimension count up to CE_MULTI_MAX_PARAMS (one lane per agent:
// an env's agents are a group of 2..64 lanes of one wave)
#define CE_MULTI_ENTRY(P) {P, launch_multi_step<P>, launch_multi_reset<P>, launch_multi_persist<P>},
#define CE_MULTI_ENTRY8(P) CE_MULTI_ENTRY(P) CE_MULTI_ENTRY(P + 2) CE_MULTI_ENTRY(P + 4) CE_MULTI_ENTRY(P + 6)
const MultiEntry kMulti[] = {CE_MULTI_ENTRY8(2) CE_MULTI_ENTRY8(10) CE_MULTI_ENTRY8(18)
                                 CE_MULTI_ENTRY8(26) CE_MULTI_ENTRY8(34) CE_MULTI_ENTRY8(42)
                                     CE_MULTI_ENTRY8(50) CE_MULTI_ENTRY8(58)};

}  // namespace

struct ce_multi_engine {
    ce_multi_config cfg{};
    const MultiEntry *kern = nullptr;
    // stream, staging buffers, step_many bookkeeping; host.persist (the
    // K-step launch, multi_persist5_kernel): max_history == 5
    ce::Host<ce_multi_outputs> host;
    int32_t agent_row[ce::kMultiMaxP] = {};   // output row of each agent (sorted names)
    float *theta = nullptr, *grad = nullptr, *hl = nullptr, *hg = nullptr, *hw = nullptr;
    float *ol = nullptr, *og = nullptr, *ow = nullptr;   // adjusted history, observation form
    double *sa = nullptr;                               // its per-entry |.| sums
    int32_t *step = nullptr;
    std::string many_name, step_name;
};

namespace {

ce::MultiArgs make_args(const ce_multi_engine *e, const float *act, const ce_multi_outputs &o) {
    ce::MultiArgs a;
    a.E = e->cfg.num_envs;
    a.H = e->cfg.max_history;
    a.max_batches = e->cfg.max_batches;
    a.auto_reset = e->cfg.auto_reset;
    for (int i = 0; i < ce::kMultiMaxP; ++i) {
        a.init[i] = i < e->cfg.n_params ? e->cfg.initial_points[i] : 0.0f;
        a.init_g[i] = 0.0f;
        a.agent_row[i] = e->agent_row[i];
    }
    ce::rosenbrock_ref(a.init, e->cfg.n_params, a.init_g, &a.init_l);
    a.theta = e->theta;
    a.grad = e->grad;
    a.hl = e->hl;
    a.hg = e->hg;
    a.hw = e->hw;
    a.ol = e->ol;
    a.og = e->og;
    a.ow = e->ow;
    a.sa = e->sa;
    a.step = e->step;
    a.act = act;
    a.obs = o.obs;
    a.reward = o.reward;
    a.done = o.done;
    a.info = o.info;
    a.episode_len = o.episode_len;
    return a;
}

// what this engine launches (engine_host.h)
struct MultiOps {
    static int step(ce_multi_engine *e, const float *act, const ce_multi_outputs &o, bool) {
        e->kern->step(make_args(e, act, o), e->host.stream);
        return CE_OK;
    }
    static int reset(ce_multi_engine *e, const ce_multi_outputs &o, bool) {
        e->kern->reset(make_args(e, nullptr, o), e->host.stream);
        return CE_OK;
    }
    static int persist(ce_multi_engine *e, int k, const float *act, int64_t stride,
                       const ce_multi_outputs &o, int64_t out_step) {
        e->kern->persist(make_args(e, act, o), k, stride, out_step, e->host.stream);
        return CE_OK;
    }
    // one policy row per (env, agent): 3H observation columns, one action
    static void policy_shape(const ce_multi_engine *e, int *obs_dim, int *act_dim, int64_t *rows) {
        *obs_dim = 3 * e->cfg.max_history;
        *act_dim = 1;
        *rows = static_cast<int64_t>(e->cfg.num_envs) * e->cfg.n_params;
    }
};

}  // namespace

extern "C" {

int ce_multi_create(const ce_multi_config *cfg, ce_multi_engine **out) {
    if (!cfg || !out) return fail(CE_EINVAL, "ce_multi_create: null argument");
    *out = nullptr;
    if (cfg->abi_version != CE_ABI_VERSION)
        return fail(CE_EINVAL, "ce_multi_create: ABI version mismatch");
    if (cfg->function != CE_FUNC_ROSENBROCK_PAIRS)
        return fail(CE_EUNSUPPORTED, "ce_multi_create: unknown function");
    if (cfg->num_envs <= 0 || cfg->max_history <= 0 || cfg->max_batches <= 0)
        return fail(CE_EINVAL, "ce_multi_create: sizes must be positive");
    if (cfg->n_params < 2 || cfg->n_params % 2 || cfg->n_params > CE_MULTI_MAX_PARAMS)
        return fail(CE_EINVAL, "ce_multi_create: n_params must be even, 2..16");
    {   // the step kernel's 32-bit element offsets: every ring plane and the
        // observation block stay below 2^31 elements
        const long long EP = static_cast<long long>(cfg->num_envs) * cfg->n_params;
        const long long planes = std::max(cfg->max_history, 5);
        if (EP * planes >= (1LL << 28) || EP * 3 * cfg->max_history >= (1LL << 28))
            return fail(CE_EUNSUPPORTED, "ce_multi_create: num_envs * n_params * max(max_history, 5) "
                                         "and the observation block must stay below 2^28 elements");
    }
    const MultiEntry *kern = nullptr;
    for (const auto &k : kMulti)
        if (k.P == cfg->n_params) kern = &k;
    if (!kern)
        return fail(CE_EUNSUPPORTED, "ce_multi_create: no kernel for n_params=" +
                                         std::to_string(cfg->n_params));
    ce_multi_engine *e = new (std::nothrow) ce_multi_engine();
    if (!e) return fail(CE_ENOMEM, "ce_multi_create: host allocation failed");
    e->cfg = *cfg;
    e->kern = kern;
    e->host.persist = cfg->max_history == 5;
    e->step_name = "multi_step_kernel<" + std::to_string(cfg->n_params) + "," +
                   std::to_string(cfg->max_history == 5 ? 5 : 0) + ">";
    e->many_name = "multi_persist5_kernel<" + std::to_string(cfg->n_params) + ",5>";
    auto bail = [&](int code) {
        ce_multi_destroy(e);
        return code;
    };
    const size_t E = cfg->num_envs, P = cfg->n_params, H = cfg->max_history;
    const int rc = e->host.create(cfg->device, E * P * sizeof(float),
                                  {E * P * 3 * H * sizeof(float), E * P * sizeof(float),
                                   E * CE_MULTI_INFO * sizeof(float), E * sizeof(int32_t), E * P});
    if (rc != CE_OK) return bail(rc);
    CE_TRY(hipMalloc(&e->theta, P * E * sizeof(float)));
    CE_TRY(hipMalloc(&e->grad, P * E * sizeof(float)));
    CE_TRY(hipMalloc(&e->hl, ce::kRawHist * E * sizeof(float)));
    CE_TRY(hipMalloc(&e->hg, ce::kRawHist * P * E * sizeof(float)));
    CE_TRY(hipMalloc(&e->hw, ce::kRawHist * P * E * sizeof(float)));
    CE_TRY(hipMalloc(&e->ol, H * E * sizeof(float)));
    CE_TRY(hipMalloc(&e->og, H * P * E * sizeof(float)));
    CE_TRY(hipMalloc(&e->ow, H * P * E * sizeof(float)));
    CE_TRY(hipMalloc(&e->sa, H * P * E * sizeof(double)));
    CE_TRY(hipMalloc(&e->step, E * sizeof(int32_t)));
    std::vector<int32_t> order, row;
    ce::sorted_agent_rows(P, &order, &row);
    std::copy(row.begin(), row.end(), e->agent_row);
    *out = e;
    return CE_OK;
}

void ce_multi_destroy(ce_multi_engine *e) {
    if (!e) return;
    e->host.destroy({e->theta, e->grad, e->hl, e->hg, e->hw, e->ol, e->og, e->ow, e->sa, e->step});
    delete e;
}

int ce_multi_set_stream(ce_multi_engine *e, void *stream) { return ce::host_set_stream(e, stream); }

int ce_multi_reset(ce_multi_engine *e, const ce_multi_outputs *out, uint32_t flags) {
    return ce::host_reset<MultiOps>(e, out, flags);
}

int ce_multi_step(ce_multi_engine *e, const float *actions, const ce_multi_outputs *out,
                  uint32_t flags) {
    return ce::host_step<MultiOps>(e, actions, out, flags, true);
}

int ce_multi_step_async(ce_multi_engine *e, const float *actions, const ce_multi_outputs *out,
                        uint32_t flags) {
    return ce::host_step<MultiOps>(e, actions, out, flags, false);
}

int ce_multi_wait(ce_multi_engine *e) { return ce::host_wait(e); }

int ce_multi_step_many(ce_multi_engine *e, int32_t k, const float *actions, int64_t stride,
                       const ce_multi_outputs *out) {
    return ce::host_step_many<MultiOps>(e, k, actions, stride, out, true);
}

int ce_multi_step_many_prepare(ce_multi_engine *e, int32_t k, const float *actions,
                               int64_t stride, const ce_multi_outputs *out) {
    return ce::host_step_many<MultiOps>(e, k, actions, stride, out, false);
}

int ce_multi_step_many_strided(ce_multi_engine *e, int32_t k, const float *actions, int64_t stride,
                               const ce_multi_outputs *out, int64_t out_step) {
    return ce::host_step_many_strided<MultiOps>(e, k, actions, stride, out, out_step);
}

int ce_multi_rollout_policy(ce_multi_engine *e, const ce_policy *p, int32_t k, const float *obs0,
                            const float *noise, int64_t noise_stride, const ce_multi_outputs *out,
                            int64_t out_step, const ce_policy_outputs *pout, int64_t pout_step) {
    return ce::host_rollout_policy<MultiOps>("ce_multi_rollout_policy", e, p, k, obs0,
                                             ce::PolicyNoise::block(noise, noise_stride), out,
                                             out_step, pout, pout_step);
}

int ce_multi_rollout_policy_rng(ce_multi_engine *e, const ce_policy *p, int32_t k,
                                const float *obs0, uint64_t seed, uint32_t t0, uint32_t row0,
                                const ce_multi_outputs *out, int64_t out_step,
                                const ce_policy_outputs *pout, int64_t pout_step) {
    return ce::host_rollout_policy<MultiOps>("ce_multi_rollout_policy_rng", e, p, k, obs0,
                                             ce::PolicyNoise::rng(seed, t0, row0), out, out_step,
                                             pout, pout_step);
}

int ce_multi_rollout_policy_vecnorm(ce_multi_engine *e, const ce_policy *p, ce_vecnorm *vn,
                                    int32_t k, float *obs_norm, int64_t obs_norm_step,
                                    float *reward_norm, int64_t reward_norm_step,
                                    uint32_t vn_flags, const ce_rollout_noise *noise,
                                    const ce_multi_outputs *out, int64_t out_step,
                                    const ce_policy_outputs *pout, int64_t pout_step) {
    const char *who = "ce_multi_rollout_policy_vecnorm";
    const int rc = ce::vecnorm_rollout_plain_ok(who, e != nullptr, p, vn, k, obs_norm,
                                                obs_norm_step, reward_norm, reward_norm_step,
                                                vn_flags, noise, out, pout);
    if (rc != CE_OK) return rc;
    const ce::VecnormRollout v{vn, obs_norm, obs_norm_step, reward_norm, reward_norm_step, vn_flags};
    return ce::host_rollout_policy<MultiOps>(who, e, p, k, obs_norm, ce::vecnorm_noise(noise), out,
                                             out_step, pout, pout_step, &v);
}

int ce_multi_set_persistent(ce_multi_engine *e, int32_t on) { return ce::host_set_persistent(e, on); }

const char *ce_multi_step_many_kernel(const ce_multi_engine *e) {
    if (!e) return "";
    return (e->host.persistent() ? e->many_name : e->step_name).c_str();
}

int ce_multi_host_outputs(ce_multi_engine *e, ce_multi_outputs *view) {
    return ce::host_outputs(e, view);
}

int ce_multi_get_state(ce_multi_engine *e, float *theta, int32_t *step) {
    if (!e) return fail(CE_EINVAL, "null engine");
    const size_t E = e->cfg.num_envs, P = e->cfg.n_params;
    CE_HIP(hipStreamSynchronize(e->host.stream));
    if (theta) {
        CE_HIP(hipMemcpy(theta, e->theta, P * E * sizeof(float), hipMemcpyDeviceToHost));
    }
    if (step) CE_HIP(hipMemcpy(step, e->step, E * sizeof(int32_t), hipMemcpyDeviceToHost));
    return CE_OK;
}

}  // extern "C"
