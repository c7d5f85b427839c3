// C-ABI implementation of the DDPG learner (ce_ddpg_* in
// include/custom_envs_amd.h): owns the flat parameters, the targets, Adam's
// moments, the two padded images the tile kernels stage from
// (ddpg_kernels.h) and the slab of gradient partials, and enqueues on the
// caller's stream
//   ce_ddpg_act     [act]
//   ce_ddpg_target  [target]
//   ce_ddpg_grad    [target, gradient, reduce, statistics]
//   ce_ddpg_step    [target, gradient, reduce, statistics, update]    (five)
//   ce_ddpg_act_rng [act, the noise formed in the kernel]
//   ce_ddpg_train   [replay indices] + steps x the five of ce_ddpg_step
//   ce_ddpg_partial [target, gradient with 1 / n_total, partial]   (one rank's record)
//   ce_ddpg_combine [combine, statistics]                  (from the W records)
//   ce_ddpg_apply   [combine, statistics, update]
// where update is Adam on both blocks, the soft update and both images'
// repack.  Every argument check precedes the first HIP call, and the checks of
// the plain arguments precede the check of the handle, so they run without a
// device.  Nothing is allocated on a call path (the targets y of a grad / step
// call go into the caller's [n] buffer); status codes, never throws.
//
// The checks DDPG shares with the PPO2 and A2C learners (rows, a partial's
// record, the gathered records, the parameter vector, Adam's blocks) are
// learner_checks.h's: one text per refusal.
//
// A handle's kind is chosen once: ddpg_create fills the handle's DdpgKind
// (ddpg_kind) from ce_ddpg_create or ce_ddpg_create_wide, and every launch of
// an act, target or gradient kernel goes through that table; a wide handle's
// entries are ddpg_wide_kernels.h's.  The reduce, statistics, partial, combine,
// update and pack kernels serve both kinds unchanged: they work on the flat
// vector, the image and the slab through DdpgPlan, whose members are sized by
// the layer count alone.  Two fixed-size members cannot describe a wide shape
// and have wide twins: the device `scale` array (the table's scale_cap floats)
// and the by-value mean / sigma of DdpgActRng (2 x 64 floats; 2 x 512 would
// not go through the kernel arguments, so a wide handle keeps them in device
// memory and uploads them when a call's values differ from the previous
// call's).  That last difference is what ddpg_act_rng still asks the kind for.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "common.h"
#include "ddpg_kernels.h"
#include "ddpg_wide_kernels.h"
#include "learner_checks.h"
#include "policy_engine.h"     // rng_replay_args_ok, rng_enqueue_replay

// What a handle's kind decides (ddpg_kind): the tile kernels and their sizes.
struct DdpgKind {
    bool wide = false;           // ce_ddpg_create_wide's
    void (*act)(ce::DdpgActArgs) = nullptr;
    void (*target)(ce::DdpgTargetArgs) = nullptr;
    void (*grad)(ce::DdpgGradArgs) = nullptr;
    const void *act_rng = nullptr;      // its second argument differs: launch_act_rng
    size_t lds_grad = 0, lds_act = 0;
    int max_lds_bytes = 0;       // the four kernels' dynamic-LDS limit
    int grid_default = 0;        // workgroups per branch at grid_limit 0 (0: one per CU)
    int scale_cap = 0;           // floats of the device `scale` array
};

struct ce_ddpg {
    ce_ddpg_config cfg{};
    ce::DdpgPlan plan{};
    DdpgKind kind{};
    int grid_max = 0;            // workgroups per branch the slab holds
    long long t = 0;             // Adam's step count, shared by both blocks
    float *params = nullptr, *target = nullptr, *m = nullptr, *v = nullptr;
    float *img = nullptr, *timg = nullptr;
    float *grad = nullptr, *slab = nullptr, *scale = nullptr;
    double *stat_slab = nullptr;
    float *d_flat = nullptr;     // staging of a host-pointer set_params
    // wide only: the generated noise's [mean | sigma], 2 x kDdpgWideMaxA floats,
    // on the device, and the values that were uploaded last
    float *noise_dev = nullptr;
    mutable std::vector<float> noise_host;
    mutable bool noise_set = false;
};

namespace {

using ce::fail;

int round_up(int v, int m) { return (v + m - 1) / m * m; }

// shape limits and hyper-parameters (no HIP call); `who` prefixes the message
int shape_ok(const char *who, const ce_ddpg_config *c, int max_d = ce::kDdpgMaxD,
             int max_a = ce::kDdpgMaxA) {
    const std::string w(who);
    if (!c) return fail(CE_EINVAL, w + ": null config");
    if (c->abi_version != CE_ABI_VERSION) return fail(CE_EINVAL, w + ": ABI version mismatch");
    if (c->obs_dim <= 0 || c->act_dim <= 0 || c->n_hidden < 0)
        return fail(CE_EINVAL, w + ": obs_dim and act_dim must be positive");
    if (c->n_hidden < 1 || c->n_hidden > ce::kDdpgMaxHidden)
        return fail(CE_EUNSUPPORTED, w + ": the DDPG networks take 1 or 2 hidden layers, got " +
                                         std::to_string(c->n_hidden));
    if (c->obs_dim > max_d)
        return fail(CE_EUNSUPPORTED, w + ": obs_dim " + std::to_string(c->obs_dim) +
                                         " exceeds the limit of " + std::to_string(max_d));
    if (c->act_dim > max_a)
        return fail(CE_EUNSUPPORTED, w + ": act_dim " + std::to_string(c->act_dim) +
                                         " exceeds the limit of " + std::to_string(max_a));
    for (int l = 0; l < c->n_hidden; ++l)
        if (c->hidden[l] != 32 && c->hidden[l] != 64)
            return fail(CE_EUNSUPPORTED, w + ": hidden width " + std::to_string(c->hidden[l]) +
                                             " is neither 32 nor 64");
    return CE_OK;
}

// `scale`: the config's [act_dim] (the wide config's is longer than c->scale)
int config_ok(const char *who, const ce_ddpg_config *c, const float *scale,
              int max_d = ce::kDdpgMaxD, int max_a = ce::kDdpgMaxA) {
    const int rc = shape_ok(who, c, max_d, max_a);
    if (rc != CE_OK) return rc;
    const std::string w(who);
    if (!(c->gamma >= 0.0 && c->gamma <= 1.0)) return fail(CE_EINVAL, w + ": gamma must be in [0, 1]");
    if (!(c->tau >= 0.0 && c->tau <= 1.0)) return fail(CE_EINVAL, w + ": tau must be in [0, 1]");
    if (!(c->actor_lr > 0.0) || !(c->critic_lr > 0.0))
        return fail(CE_EINVAL, w + ": actor_lr and critic_lr must be positive");
    if (!(c->beta1 >= 0.0 && c->beta1 < 1.0) || !(c->beta2 >= 0.0 && c->beta2 < 1.0))
        return fail(CE_EINVAL, w + ": beta1 and beta2 must be in [0, 1)");
    if (!(c->eps > 0.0)) return fail(CE_EINVAL, w + ": eps must be positive");
    if (!(c->obs_lo < c->obs_hi)) return fail(CE_EINVAL, w + ": obs_lo must be below obs_hi");
    if (c->grid_limit < 0) return fail(CE_EINVAL, w + ": grid_limit must not be negative");
    for (int i = 0; i < c->act_dim; ++i)
        if (!std::isfinite(scale[i])) return fail(CE_EINVAL, w + ": scale must be finite");
    return CE_OK;
}

// the members a wide config shares with ce_ddpg_config (scale stays zero: a
// wide handle reads the wide config's own array)
ce_ddpg_config plain_config(const ce_ddpg_wide_config &w) {
    ce_ddpg_config c{};
    c.abi_version = w.abi_version;
    c.device = w.device;
    c.obs_dim = w.obs_dim;
    c.act_dim = w.act_dim;
    c.n_hidden = w.n_hidden;
    for (int i = 0; i < 4; ++i) c.hidden[i] = w.hidden[i];
    c.grid_limit = w.grid_limit;
    c.gamma = w.gamma;
    c.tau = w.tau;
    c.actor_lr = w.actor_lr;
    c.critic_lr = w.critic_lr;
    c.beta1 = w.beta1;
    c.beta2 = w.beta2;
    c.eps = w.eps;
    c.obs_lo = w.obs_lo;
    c.obs_hi = w.obs_hi;
    return c;
}

// the images' layout, the flat vector's segments and the LDS sizes
ce::DdpgPlan make_plan(const ce_ddpg_config &c) {
    ce::DdpgPlan a{};
    a.D = c.obs_dim;
    a.A = c.act_dim;
    a.n_hidden = c.n_hidden;
    a.obs_lo = static_cast<float>(c.obs_lo);
    a.obs_hi = static_cast<float>(c.obs_hi);
    int img = 0, src = 0, seg = 0, wmax = 0, kmax = 0;
    auto add = [&](int rows, int cols, int rows_pad, int cols_pad) {
        a.seg_dst[seg] = img;
        a.seg_src[seg] = src;
        a.seg_cols[seg] = cols;
        a.seg_cols_pad[seg] = cols_pad;
        ++seg;
        src += rows * cols;
        const int at = img;
        img += rows_pad * cols_pad;
        return at;
    };
    for (int net = 0; net < 2; ++net) {
        if (net == 1) a.n_actor = src;
        int in = c.obs_dim;
        for (int l = 0; l <= c.n_hidden; ++l) {
            const int out = l < c.n_hidden ? c.hidden[l] : (net == 0 ? c.act_dim : 1);
            const int ip = round_up(in, 4), op = round_up(out, 32);
            a.out_dim[net][l] = out;
            a.in_pad[net][l] = ip;
            a.out_pad[net][l] = op;
            a.off_w[net][l] = add(in, out, ip, op);
            a.off_b[net][l] = add(1, out, 1, op);
            // dZ W^T reads whole 32-row chunks of the stage
            wmax = std::max(wmax, round_up(ip, 32) * (op + 1));
            kmax = std::max(kmax, ip);
            in = (net == 1 && l == 0) ? out + c.act_dim : out;      // the concat
        }
    }
    a.n_segs = seg;
    a.n_params = src;
    a.img_floats = img;
    a.w_floats = round_up(wmax, 4);
    a.act_floats = kmax * ce::kDdpgLd;
    return a;
}

size_t lds_bytes(const ce::DdpgPlan &a, int bufs) {
    const int sech2 = bufs == ce::kDdpgBufs ? a.out_pad[0][a.n_hidden] * ce::kDdpgLd : 0;
    return static_cast<size_t>(a.w_floats + bufs * a.act_floats + ce::kDdpgRowFloats + sech2) *
           sizeof(float);
}

// the table of a handle's kind: the one place where it is chosen
DdpgKind ddpg_kind(bool wide, const ce::DdpgPlan &a) {
    DdpgKind k{};
    k.wide = wide;
    if (wide) {
        k.act = ce::ddpg_act_wide_kernel;
        k.act_rng = reinterpret_cast<const void *>(ce::ddpg_act_rng_wide_kernel);
        k.target = ce::ddpg_target_wide_kernel;
        k.grad = ce::ddpg_grad_wide_kernel;
        k.lds_grad = k.lds_act = static_cast<size_t>(ce::ddpg_wide_lds_floats(a.A)) * sizeof(float);
        k.max_lds_bytes = ce::kDdpgWideMaxLdsBytes;
        k.grid_default = ce::kDdpgWideGrid;
        k.scale_cap = ce::kDdpgWideMaxA;
    } else {
        k.act = ce::ddpg_act_kernel;
        k.act_rng = reinterpret_cast<const void *>(ce::ddpg_act_rng_kernel);
        k.target = ce::ddpg_target_kernel;
        k.grad = ce::ddpg_grad_kernel;
        k.lds_grad = lds_bytes(a, ce::kDdpgBufs);
        k.lds_act = lds_bytes(a, ce::kDdpgActBufs);
        k.max_lds_bytes = ce::kDdpgMaxLdsBytes;
        k.scale_cap = ce::kDdpgMaxA;
    }
    return k;
}

int n_params_of(const ce_ddpg *l) { return l ? l->plan.n_params : -1; }

unsigned tiles_of(int64_t rows) {
    return static_cast<unsigned>((rows + ce::kDdpgTile - 1) / ce::kDdpgTile);
}

ce::DdpgActArgs act_args(const ce_ddpg *l, const float *obs, const float *noise, int64_t rows,
                         float *action, float *env_action) {
    ce::DdpgActArgs g{};
    g.p = l->plan;
    g.rows = static_cast<int>(rows);
    g.img = l->img;
    g.scale = l->scale;
    g.obs = obs;
    g.noise = noise;
    g.action = action;
    g.env_action = env_action;
    return g;
}

// what DdpgActRng and DdpgWideActRng share; mean and sigma are the caller's
template <class Rng>
Rng act_rng_args(uint64_t seed, uint32_t t, uint32_t row0, bool ou, double theta, double dt,
                 float *ou_state, const uint8_t *reset) {
    Rng n{};
    n.seed_lo = static_cast<uint32_t>(seed);
    n.seed_hi = static_cast<uint32_t>(seed >> 32);
    n.t = t;
    n.row0 = row0;
    n.kind = ou ? ce::kDdpgNoiseOu : ce::kDdpgNoiseNormal;
    n.theta = ou ? static_cast<float>(theta) : 0.0f;
    n.dt = ou ? static_cast<float>(dt) : 0.0f;
    n.ou = ou ? ou_state : nullptr;
    n.reset = ou ? reset : nullptr;
    return n;
}

// the generated-noise act kernel of the handle's kind, `noise_lds` bytes for
// the tile's N(0,1) block on top of the act kernel's
template <class Rng>
void launch_act_rng(const ce_ddpg *l, const ce::DdpgActArgs &g, const Rng &n, size_t noise_lds,
                    hipStream_t stream) {
    const auto kernel = reinterpret_cast<void (*)(ce::DdpgActArgs, Rng)>(
        const_cast<void *>(l->kind.act_rng));
    hipLaunchKernelGGL(kernel, dim3(tiles_of(g.rows)), dim3(ce::kDdpgBlock),
                       l->kind.lds_act + noise_lds, stream, g, n);
}

int batch_ok(const char *who, const ce_ddpg *l, int64_t n, int64_t m, const int32_t *idx,
             const float *obs0, const float *actions, const float *rewards, const float *obs1,
             const uint8_t *dones, const float *y, const float *stats) {
    const int rc = ce::learner_rows_ok(who, n, m, idx);
    if (rc != CE_OK) return rc;
    const auto null = [who](const char *what) { return fail(CE_EINVAL, std::string(who) + ": null " + what); };
    if (!obs0) return null("obs0");
    if (!actions) return null("actions");
    if (!rewards) return null("rewards");
    if (!obs1) return null("obs1");
    if (!dones) return null("dones");
    if (!y) return null("y buffer");
    if (!stats) return null("stats");
    if (!l) return null("learner");
    return CE_OK;
}

void enqueue_target(const ce_ddpg *l, int64_t n, int64_t m, const int32_t *idx, const float *obs1,
                    const float *rewards, const uint8_t *dones, float *y, hipStream_t stream) {
    ce::DdpgTargetArgs g{};
    g.p = l->plan;
    g.n = static_cast<int>(n);
    g.m = static_cast<int>(m);
    g.gamma = static_cast<float>(l->cfg.gamma);
    g.timg = l->timg;
    g.idx = idx;
    g.obs1 = obs1;
    g.rewards = rewards;
    g.dones = dones;
    g.y = y;
    hipLaunchKernelGGL(l->kind.target, dim3(tiles_of(n)), dim3(ce::kDdpgBlock), l->kind.lds_grad,
                       stream, g);
}

// [target, gradient] of this call's n rows with the row weight 1 / n_total
// into y and the slab; returns the gradient kernel's workgroups per branch
int enqueue_slab(const ce_ddpg *l, int64_t n, int64_t n_total, int64_t m, const int32_t *idx,
                 const float *obs0, const float *actions, const float *rewards, const float *obs1,
                 const uint8_t *dones, float *y, hipStream_t stream) {
    enqueue_target(l, n, m, idx, obs1, rewards, dones, y, stream);
    ce::DdpgGradArgs g{};
    g.p = l->plan;
    g.n = static_cast<int>(n);
    g.n_total = static_cast<int>(n_total);
    g.m = static_cast<int>(m);
    g.tiles = static_cast<int>((n + ce::kDdpgTile - 1) / ce::kDdpgTile);
    g.grid = std::min(g.tiles, l->grid_max);
    g.img = l->img;
    g.idx = idx;
    g.obs0 = obs0;
    g.actions = actions;
    g.y = y;
    g.slab = l->slab;
    g.stat_slab = l->stat_slab;
    hipLaunchKernelGGL(l->kind.grad, dim3(g.grid, 2), dim3(ce::kDdpgBlock), l->kind.lds_grad,
                       stream, g);
    return g.grid;
}

// [target, gradient, reduce, statistics] into y / grad / stats
void enqueue_grad(const ce_ddpg *l, int64_t n, int64_t m, const int32_t *idx, const float *obs0,
                  const float *actions, const float *rewards, const float *obs1,
                  const uint8_t *dones, float *y, float *grad, float *stats, hipStream_t stream) {
    const int grid = enqueue_slab(l, n, n, m, idx, obs0, actions, rewards, obs1, dones, y, stream);
    ce::DdpgReduceArgs q{};
    q.p = l->plan;
    q.grid = grid;
    q.slab = l->slab;
    q.grad = grad;
    const int np = l->plan.n_params;
    hipLaunchKernelGGL(ce::ddpg_reduce_kernel, dim3((np + 255) / 256), dim3(256), 0, stream, q);
    hipLaunchKernelGGL(ce::ddpg_stats_kernel, dim3(1), dim3(256), 0, stream, static_cast<int>(n),
                       grid, 2 * ce::kDdpgRowStats, np, l->plan.n_actor, l->stat_slab, grad, stats);
}

// [combine, statistics] from the W gathered records into grad / stats
void enqueue_combine(const ce_ddpg *l, int32_t world, const double *records, int64_t n_total,
                     float *grad, float *stats, hipStream_t stream) {
    const int np = l->plan.n_params;
    ce::DdpgCombineArgs q{};
    q.n_params = np;
    q.world = world;
    q.record_doubles = ce::ddpg_record_doubles(np);
    q.records = records;
    q.grad = grad;
    hipLaunchKernelGGL(ce::ddpg_combine_kernel, dim3((np + 255) / 256), dim3(256), 0, stream, q);
    hipLaunchKernelGGL(ce::ddpg_stats_kernel, dim3(1), dim3(256), 0, stream,
                       static_cast<int>(n_total), world, q.record_doubles, np, l->plan.n_actor,
                       records + np, grad, stats);
}

// [update] from l->grad: Adam on both blocks, one more step; soft update; images.
// A rate below zero means the config's; zero leaves that block where it is.
void enqueue_update(ce_ddpg *l, double actor_lr, double critic_lr, hipStream_t stream) {
    const ce_ddpg_config &c = l->cfg;
    const double t = static_cast<double>(++l->t);
    const double corr = std::sqrt(1.0 - std::pow(c.beta2, t)) / (1.0 - std::pow(c.beta1, t));
    ce::DdpgUpdateArgs u{};
    u.p = l->plan;
    u.lr_t_actor = static_cast<float>((actor_lr >= 0.0 ? actor_lr : c.actor_lr) * corr);
    u.lr_t_critic = static_cast<float>((critic_lr >= 0.0 ? critic_lr : c.critic_lr) * corr);
    u.beta1 = static_cast<float>(c.beta1);
    u.beta2 = static_cast<float>(c.beta2);
    u.omb1 = static_cast<float>(1.0 - c.beta1);
    u.omb2 = static_cast<float>(1.0 - c.beta2);
    u.eps = static_cast<float>(c.eps);
    u.tau = static_cast<float>(c.tau);
    u.omt = static_cast<float>(1.0 - c.tau);
    u.grad = l->grad;
    u.params = l->params;
    u.target = l->target;
    u.m = l->m;
    u.v = l->v;
    u.img = l->img;
    u.timg = l->timg;
    hipLaunchKernelGGL(ce::ddpg_update_kernel, dim3((l->plan.n_params + 255) / 256), dim3(256), 0,
                       stream, u);
}

}  // namespace

extern "C" {

int ce_ddpg_n_params(const ce_ddpg_config *cfg) {
    const int rc = shape_ok("ce_ddpg_n_params", cfg);
    if (rc != CE_OK) return rc;
    return make_plan(*cfg).n_params;
}

// the handle of a checked config; `scale` [act_dim] is the config's own array
static int ddpg_create(const ce_ddpg_config &cfg, const float *scale, bool wide, ce_ddpg **out) {
    const std::string who = wide ? "ce_ddpg_create_wide" : "ce_ddpg_create";
    ce_ddpg *l = new (std::nothrow) ce_ddpg();
    if (!l) return fail(CE_ENOMEM, who + ": host allocation failed");
    l->cfg = cfg;
    l->plan = make_plan(cfg);
    l->kind = ddpg_kind(wide, l->plan);
    const DdpgKind &k = l->kind;
    if (wide) l->noise_host.assign(2 * ce::kDdpgWideMaxA, 0.0f);
    auto bail = [&](int code) {
        ce_ddpg_destroy(l);
        return code;
    };
    const ce::DdpgPlan &a = l->plan;
    CE_TRY(hipSetDevice(cfg.device));
    hipDeviceProp_t prop;
    CE_TRY(hipGetDeviceProperties(&prop, cfg.device));
    const int cus = std::max(1, prop.multiProcessorCount);
    l->grid_max = cfg.grid_limit > 0 ? cfg.grid_limit
                                     : (k.grid_default > 0 ? std::min(cus, k.grid_default) : cus);
    // the dynamic LDS of the tile kernels, once, from the limits' need
    for (const void *f : {reinterpret_cast<const void *>(k.act), k.act_rng,
                          reinterpret_cast<const void *>(k.target),
                          reinterpret_cast<const void *>(k.grad)})
        CE_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, k.max_lds_bytes));
    const size_t np = static_cast<size_t>(a.n_params) * sizeof(float);
    const size_t ni = static_cast<size_t>(a.img_floats) * sizeof(float);
    for (float **q : {&l->params, &l->target, &l->m, &l->v, &l->grad, &l->d_flat}) {
        CE_TRY(hipMalloc(q, np));
        CE_TRY(hipMemset(*q, 0, np));
    }
    for (float **q : {&l->img, &l->timg}) {
        CE_TRY(hipMalloc(q, ni));
        CE_TRY(hipMemset(*q, 0, ni));       // the padding stays zero
    }
    CE_TRY(hipMalloc(&l->slab, static_cast<size_t>(l->grid_max) * ni));
    CE_TRY(hipMalloc(&l->stat_slab,
                     static_cast<size_t>(l->grid_max) * 2 * ce::kDdpgRowStats * sizeof(double)));
    const size_t ns = static_cast<size_t>(k.scale_cap) * sizeof(float);
    CE_TRY(hipMalloc(&l->scale, ns));
    CE_TRY(hipMemcpy(l->scale, scale, ns, hipMemcpyHostToDevice));
    if (wide) {
        CE_TRY(hipMalloc(&l->noise_dev, 2 * ce::kDdpgWideMaxA * sizeof(float)));
        CE_TRY(hipMemset(l->noise_dev, 0, 2 * ce::kDdpgWideMaxA * sizeof(float)));
    }
    CE_TRY(hipDeviceSynchronize());
    *out = l;
    return CE_OK;
}

int ce_ddpg_create(const ce_ddpg_config *cfg, ce_ddpg **out) {
    if (!out) return fail(CE_EINVAL, "ce_ddpg_create: null output handle");
    *out = nullptr;
    const int rc = config_ok("ce_ddpg_create", cfg, cfg ? cfg->scale : nullptr);
    if (rc != CE_OK) return rc;
    return ddpg_create(*cfg, cfg->scale, false, out);
}

int ce_ddpg_n_params_wide(const ce_ddpg_wide_config *cfg) {
    if (!cfg) return fail(CE_EINVAL, "ce_ddpg_n_params_wide: null config");
    const ce_ddpg_config c = plain_config(*cfg);
    const int rc = shape_ok("ce_ddpg_n_params_wide", &c, ce::kDdpgWideMaxD, ce::kDdpgWideMaxA);
    if (rc != CE_OK) return rc;
    return make_plan(c).n_params;
}

int ce_ddpg_create_wide(const ce_ddpg_wide_config *cfg, ce_ddpg **out) {
    if (!out) return fail(CE_EINVAL, "ce_ddpg_create_wide: null output handle");
    *out = nullptr;
    if (!cfg) return fail(CE_EINVAL, "ce_ddpg_create_wide: null config");
    const ce_ddpg_config c = plain_config(*cfg);
    const int rc = config_ok("ce_ddpg_create_wide", &c, cfg->scale, ce::kDdpgWideMaxD,
                             ce::kDdpgWideMaxA);
    if (rc != CE_OK) return rc;
    return ddpg_create(c, cfg->scale, true, out);
}

void ce_ddpg_destroy(ce_ddpg *l) {
    if (!l) return;
    for (void *q : {static_cast<void *>(l->params), static_cast<void *>(l->target),
                    static_cast<void *>(l->m), static_cast<void *>(l->v),
                    static_cast<void *>(l->img), static_cast<void *>(l->timg),
                    static_cast<void *>(l->grad), static_cast<void *>(l->slab),
                    static_cast<void *>(l->scale), static_cast<void *>(l->stat_slab),
                    static_cast<void *>(l->d_flat), static_cast<void *>(l->noise_dev)})
        if (q) (void)hipFree(q);
    delete l;
}

int ce_ddpg_set_params(ce_ddpg *l, const float *flat, int64_t n, uint32_t flags, void *hip_stream) {
    const char *who = "ce_ddpg_set_params";
    const int rc = ce::learner_params_ok(who, n_params_of(l), "agent", flat, n, ": got ");
    if (rc != CE_OK) return rc;
    CE_CLEAR_STALE_ERROR_AT(who);
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const bool dev = (flags & CE_PTR_DEVICE) != 0;
    const float *src = flat;
    if (!dev) {
        CE_HIP(hipMemcpyAsync(l->d_flat, flat, n * sizeof(float), hipMemcpyHostToDevice, stream));
        CE_HIP(hipStreamSynchronize(stream));      // `flat` may be pageable
        src = l->d_flat;
    }
    const bool both = (flags & CE_DDPG_TARGET) == 0;
    hipLaunchKernelGGL(ce::ddpg_pack_kernel, dim3((l->plan.n_params + 255) / 256), dim3(256), 0,
                       stream, l->plan, src, both ? l->params : nullptr, l->target,
                       both ? l->img : nullptr, l->timg);
    CE_HIP(hipGetLastError());
    if (!dev) CE_HIP(hipStreamSynchronize(stream));
    return CE_OK;
}

int ce_ddpg_get_params(ce_ddpg *l, float *flat, int64_t n, uint32_t flags, void *hip_stream) {
    const char *who = "ce_ddpg_get_params";
    const int rc =
        ce::learner_params_ok(who, n_params_of(l), "agent", flat, n, ": got room for ");
    if (rc != CE_OK) return rc;
    CE_CLEAR_STALE_ERROR_AT(who);
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const bool dev = (flags & CE_PTR_DEVICE) != 0;
    const float *src = (flags & CE_DDPG_TARGET) ? l->target : l->params;
    CE_HIP(hipMemcpyAsync(flat, src, n * sizeof(float),
                          dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream));
    if (!dev) CE_HIP(hipStreamSynchronize(stream));
    return CE_OK;
}

int ce_ddpg_act(const ce_ddpg *l, const float *obs, const float *noise, int64_t rows,
                float *action, float *env_action, void *hip_stream) {
    const char *who = "ce_ddpg_act";
    const auto bad = [who](const std::string &what) { return fail(CE_EINVAL, who + what); };
    if (rows < 1 || rows > ce::kLearnerMaxRows)
        return bad(": rows must be in [1, 2^24], got " + std::to_string(rows));
    if (!obs) return bad(": null obs");
    if (!action) return bad(": null action output");
    if (!env_action) return bad(": null env_action output");
    if (!l) return bad(": null learner");
    CE_CLEAR_STALE_ERROR_AT(who);
    hipLaunchKernelGGL(l->kind.act, dim3(tiles_of(rows)), dim3(ce::kDdpgBlock), l->kind.lds_act,
                       static_cast<hipStream_t>(hip_stream),
                       act_args(l, obs, noise, rows, action, env_action));
    CE_HIP(hipGetLastError());
    return CE_OK;
}

// ce_ddpg_act_rng and ce_ddpg_act_rng_wide: `mean` / `sigma` hold `cap` columns
static int ddpg_act_rng(const char *who, const ce_ddpg *l, const float *obs, int64_t rows,
                        uint64_t seed, uint32_t t, uint32_t row0, bool have_noise, int32_t kind,
                        double theta, double dt, const float *mean, const float *sigma, int cap,
                        float *ou_state, const uint8_t *reset, float *action, float *env_action,
                        void *hip_stream) {
    const auto bad = [who](const std::string &what) { return fail(CE_EINVAL, who + what); };
    if (rows < 1 || rows > ce::kLearnerMaxRows)
        return bad(": rows must be in [1, 2^24], got " + std::to_string(rows));
    if (static_cast<uint64_t>(row0) + static_cast<uint64_t>(rows) > (uint64_t(1) << 32))
        return bad(": rows row0 .. row0 + rows - 1 must stay below 2^32");
    if (!obs) return bad(": null obs");
    if (!action) return bad(": null action output");
    if (!env_action) return bad(": null env_action output");
    if (!have_noise) return bad(": null noise description");
    if (kind != CE_DDPG_NOISE_NORMAL && kind != CE_DDPG_NOISE_OU)
        return bad(": unknown noise kind " + std::to_string(kind));
    const bool ou = kind == CE_DDPG_NOISE_OU;
    if (ou && !ou_state) return bad(": Ornstein-Uhlenbeck noise needs its state buffer");
    if (ou && (!std::isfinite(theta) || !std::isfinite(dt) || !(dt > 0.0)))
        return bad(": theta must be finite and dt positive");
    if (!l) return bad(": null learner");
    const int A = l->plan.A;
    if (A > cap)
        return bad(": the agent has " + std::to_string(A) + " action columns and the noise " +
                   "description " + std::to_string(cap) + ": use ce_ddpg_act_rng_wide");
    for (int c = 0; c < A; ++c)
        if (!std::isfinite(mean[c]) || !std::isfinite(sigma[c]) || sigma[c] < 0.0f)
            return bad(": mean must be finite and sigma finite and not negative");
    CE_CLEAR_STALE_ERROR_AT(who);
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const ce::DdpgActArgs g = act_args(l, obs, nullptr, rows, action, env_action);
    // OU: s = float32(sigma sqrt(dt)) formed in double
    const auto held_sigma = [&](int c) {
        return ou ? static_cast<float>(static_cast<double>(sigma[c]) * std::sqrt(dt)) : sigma[c];
    };
    if (l->kind.wide) {
        float held[2 * ce::kDdpgWideMaxA] = {};
        for (int c = 0; c < A; ++c) {
            held[c] = mean[c];
            held[ce::kDdpgWideMaxA + c] = held_sigma(c);
        }
        if (!l->noise_set || std::memcmp(held, l->noise_host.data(), sizeof(held)) != 0) {
            std::memcpy(l->noise_host.data(), held, sizeof(held));
            CE_HIP(hipMemcpyAsync(l->noise_dev, l->noise_host.data(), sizeof(held),
                                  hipMemcpyHostToDevice, stream));
            CE_HIP(hipStreamSynchronize(stream));      // the host copy may change at the next call
            l->noise_set = true;
        }
        auto n = act_rng_args<ce::DdpgWideActRng>(seed, t, row0, ou, theta, dt, ou_state, reset);
        n.mean = l->noise_dev;
        n.sigma = l->noise_dev + ce::kDdpgWideMaxA;
        launch_act_rng(l, g, n, 0, stream);      // the tile's N(0,1) block is the plan's S region
    } else {
        auto n = act_rng_args<ce::DdpgActRng>(seed, t, row0, ou, theta, dt, ou_state, reset);
        for (int c = 0; c < A; ++c) {
            n.mean[c] = mean[c];
            n.sigma[c] = held_sigma(c);
        }
        // + the tile's N(0,1) block [round4(A)][33] behind the row scalars
        launch_act_rng(l, g, n, static_cast<size_t>(round_up(A, 4)) * ce::kDdpgLd * sizeof(float),
                       stream);
    }
    CE_HIP(hipGetLastError());
    return CE_OK;
}

int ce_ddpg_act_rng(const ce_ddpg *l, const float *obs, int64_t rows, uint64_t seed, uint32_t t,
                    uint32_t row0, const ce_ddpg_noise *noise, float *ou_state,
                    const uint8_t *reset, float *action, float *env_action, void *hip_stream) {
    return ddpg_act_rng("ce_ddpg_act_rng", l, obs, rows, seed, t, row0, noise != nullptr,
                        noise ? noise->kind : 0, noise ? noise->theta : 0.0, noise ? noise->dt : 0.0,
                        noise ? noise->mean : nullptr, noise ? noise->sigma : nullptr,
                        ce::kDdpgMaxA, ou_state, reset, action, env_action, hip_stream);
}

int ce_ddpg_act_rng_wide(ce_ddpg *l, const float *obs, int64_t rows, uint64_t seed, uint32_t t,
                         uint32_t row0, const ce_ddpg_wide_noise *noise, float *ou_state,
                         const uint8_t *reset, float *action, float *env_action,
                         void *hip_stream) {
    return ddpg_act_rng("ce_ddpg_act_rng_wide", l, obs, rows, seed, t, row0, noise != nullptr,
                        noise ? noise->kind : 0, noise ? noise->theta : 0.0, noise ? noise->dt : 0.0,
                        noise ? noise->mean : nullptr, noise ? noise->sigma : nullptr,
                        ce::kDdpgWideMaxA, ou_state, reset, action, env_action, hip_stream);
}

int ce_ddpg_target(ce_ddpg *l, int64_t n, int64_t m, const int32_t *idx, const float *obs1,
                   const float *rewards, const uint8_t *dones, float *y, void *hip_stream) {
    const char *who = "ce_ddpg_target";
    const int rc = ce::learner_rows_ok(who, n, m, idx);
    if (rc != CE_OK) return rc;
    const auto null = [who](const char *what) { return fail(CE_EINVAL, std::string(who) + ": null " + what); };
    if (!obs1) return null("obs1");
    if (!rewards) return null("rewards");
    if (!dones) return null("dones");
    if (!y) return null("y output");
    if (!l) return null("learner");
    CE_CLEAR_STALE_ERROR_AT(who);
    enqueue_target(l, n, m, idx, obs1, rewards, dones, y, static_cast<hipStream_t>(hip_stream));
    CE_HIP(hipGetLastError());
    return CE_OK;
}

int ce_ddpg_grad(ce_ddpg *l, int64_t n, int64_t m, const int32_t *idx, const float *obs0,
                 const float *actions, const float *rewards, const float *obs1,
                 const uint8_t *dones, float *y, float *grad, float *stats, void *hip_stream) {
    const char *who = "ce_ddpg_grad";
    if (!grad) return fail(CE_EINVAL, std::string(who) + ": null grad");
    const int rc = batch_ok(who, l, n, m, idx, obs0, actions, rewards, obs1, dones, y, stats);
    if (rc != CE_OK) return rc;
    CE_CLEAR_STALE_ERROR_AT(who);
    enqueue_grad(l, n, m, idx, obs0, actions, rewards, obs1, dones, y, grad, stats,
                 static_cast<hipStream_t>(hip_stream));
    CE_HIP(hipGetLastError());
    return CE_OK;
}

int ce_ddpg_step(ce_ddpg *l, int64_t n, int64_t m, const int32_t *idx, const float *obs0,
                 const float *actions, const float *rewards, const float *obs1,
                 const uint8_t *dones, float *y, double actor_lr, double critic_lr, float *stats,
                 void *hip_stream) {
    const char *who = "ce_ddpg_step";
    if (std::isnan(actor_lr) || std::isnan(critic_lr))
        return fail(CE_EINVAL, std::string(who) + ": a learning rate is not a number");
    const int rc = batch_ok(who, l, n, m, idx, obs0, actions, rewards, obs1, dones, y, stats);
    if (rc != CE_OK) return rc;
    CE_CLEAR_STALE_ERROR_AT(who);
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    enqueue_grad(l, n, m, idx, obs0, actions, rewards, obs1, dones, y, l->grad, stats, stream);
    enqueue_update(l, actor_lr, critic_lr, stream);
    CE_HIP(hipGetLastError());
    return CE_OK;
}

int ce_ddpg_train(ce_ddpg *l, int32_t steps, int64_t n, int64_t size, uint64_t seed, uint32_t t0,
                  const float *obs0, const float *actions, const float *rewards,
                  const float *obs1, const uint8_t *dones, int32_t *idx_scratch, float *y,
                  double actor_lr, double critic_lr, float *stats, void *hip_stream) {
    const char *who = "ce_ddpg_train";
    if (std::isnan(actor_lr) || std::isnan(critic_lr))
        return fail(CE_EINVAL, std::string(who) + ": a learning rate is not a number");
    int rc = ce::rng_replay_args_ok(who, steps, n, size, t0);
    if (rc != CE_OK) return rc;
    if (!idx_scratch) return fail(CE_EINVAL, std::string(who) + ": null idx_scratch");
    if (reinterpret_cast<uintptr_t>(idx_scratch) & 3)
        return fail(CE_EINVAL, std::string(who) + ": idx_scratch must be 4-byte aligned");
    rc = batch_ok(who, l, n, size, idx_scratch, obs0, actions, rewards, obs1, dones, y, stats);
    if (rc != CE_OK) return rc;
    CE_CLEAR_STALE_ERROR_AT(who);
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    ce::rng_enqueue_replay(idx_scratch, steps, n, size, seed, t0, stream);
    for (int32_t s = 0; s < steps; ++s) {
        enqueue_grad(l, n, size, idx_scratch + s * n, obs0, actions, rewards, obs1, dones, y,
                     l->grad, stats + s * 8, stream);
        enqueue_update(l, actor_lr, critic_lr, stream);
    }
    CE_HIP(hipGetLastError());
    return CE_OK;
}

int64_t ce_ddpg_record_bytes(const ce_ddpg *l) {
    if (!l) {
        fail(CE_EINVAL, "ce_ddpg_record_bytes: null learner");
        return -1;
    }
    return int64_t(ce::ddpg_record_doubles(l->plan.n_params)) * 8;
}

int ce_ddpg_partial(ce_ddpg *l, int64_t n, int64_t n_total, int64_t m, const int32_t *idx,
                    const float *obs0, const float *actions, const float *rewards,
                    const float *obs1, const uint8_t *dones, float *y, double *record,
                    void *hip_stream) {
    const char *who = "ce_ddpg_partial";
    int rc = ce::learner_rows_ok(who, n, m, idx);
    if (rc != CE_OK) return rc;
    if ((rc = ce::learner_partial_ok(who, n, n_total, record)) != CE_OK) return rc;
    // `record` stands in for stats in the null checks the entry points share
    rc = batch_ok(who, l, n, m, idx, obs0, actions, rewards, obs1, dones, y,
                  reinterpret_cast<const float *>(record));
    if (rc != CE_OK) return rc;
    CE_CLEAR_STALE_ERROR_AT(who);
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    ce::DdpgPartialArgs q{};
    q.p = l->plan;
    q.n = static_cast<int>(n);
    q.grid = enqueue_slab(l, n, n_total, m, idx, obs0, actions, rewards, obs1, dones, y, stream);
    q.slab = l->slab;
    q.stat_slab = l->stat_slab;
    q.record = record;
    hipLaunchKernelGGL(ce::ddpg_partial_kernel, dim3((l->plan.n_params + 255) / 256), dim3(256), 0,
                       stream, q);
    CE_HIP(hipGetLastError());
    return CE_OK;
}

int ce_ddpg_combine(ce_ddpg *l, int32_t world, const double *records, int64_t n_total,
                    float *grad, float *stats, void *hip_stream) {
    const char *who = "ce_ddpg_combine";
    if (!grad) return fail(CE_EINVAL, std::string(who) + ": null grad");
    const int rc = ce::learner_apply_ok(who, world, records, n_total, stats);
    if (rc != CE_OK) return rc;
    if (!l) return fail(CE_EINVAL, std::string(who) + ": null learner");
    CE_CLEAR_STALE_ERROR_AT(who);
    enqueue_combine(l, world, records, n_total, grad, stats, static_cast<hipStream_t>(hip_stream));
    CE_HIP(hipGetLastError());
    return CE_OK;
}

int ce_ddpg_apply(ce_ddpg *l, int32_t world, const double *records, int64_t n_total,
                  double actor_lr, double critic_lr, float *stats, void *hip_stream) {
    const char *who = "ce_ddpg_apply";
    if (std::isnan(actor_lr) || std::isnan(critic_lr))
        return fail(CE_EINVAL, std::string(who) + ": a learning rate is not a number");
    const int rc = ce::learner_apply_ok(who, world, records, n_total, stats);
    if (rc != CE_OK) return rc;
    if (!l) return fail(CE_EINVAL, std::string(who) + ": null learner");
    CE_CLEAR_STALE_ERROR_AT(who);
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    enqueue_combine(l, world, records, n_total, l->grad, stats, stream);
    enqueue_update(l, actor_lr, critic_lr, stream);
    CE_HIP(hipGetLastError());
    return CE_OK;
}

// Adam's two blocks to (`set` false) or from the caller's
static int ddpg_opt_state(const char *who, ce_ddpg *l, void *m, void *v, int64_t n, bool set,
                          uint32_t flags, void *hip_stream) {
    return ce::learner_opt_state(who, n_params_of(l), "agent", l ? l->m : nullptr,
                                 l ? l->v : nullptr, "m", "v", m, v, n, set, flags, hip_stream);
}

int ce_ddpg_get_opt_state(ce_ddpg *l, float *m, float *v, int64_t n, int64_t *step,
                          uint32_t flags, void *hip_stream) {
    if (!step) return fail(CE_EINVAL, "ce_ddpg_get_opt_state: null step");
    const int rc = ddpg_opt_state("ce_ddpg_get_opt_state", l, m, v, n, false, flags, hip_stream);
    if (rc != CE_OK) return rc;
    *step = l->t;
    return CE_OK;
}

int ce_ddpg_set_opt_state(ce_ddpg *l, const float *m, const float *v, int64_t n, int64_t step,
                          uint32_t flags, void *hip_stream) {
    if (step < 0) return fail(CE_EINVAL, "ce_ddpg_set_opt_state: step must not be negative");
    const int rc = ddpg_opt_state("ce_ddpg_set_opt_state", l, const_cast<float *>(m),
                                  const_cast<float *>(v), n, true, flags, hip_stream);
    if (rc != CE_OK) return rc;
    l->t = step;
    return CE_OK;
}

}  // extern "C"
