// C-ABI implementation of the device-side MLP policy (ce_policy_* in
// include/custom_envs_amd.h): owns the parameter image policy_mlp_kernel
// stages from (policy_kernels.h), repacks a caller's flat parameter vector
// into it with one launch, and enqueues the fused forward.  Every argument
// check precedes the first HIP call, so the checks run without a device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <new>
#include <string>
#include <vector>

#include "common.h"
#include "policy_engine.h"
#include "policy_kernels.h"
#include "policy_wide_kernels.h"
#include "rng_kernels.h"

struct ce_policy {
    ce_policy_config cfg{};
    ce::PolicyArgs args{};       // shape, offsets and img filled at create
    ce::PolicyPack pack{};
    int n_params = 0, img_floats = 0;
    size_t lds_bytes = 0;
    bool wide = false;           // created by ce_policy_create_wide: policy_wide_kernel
    float *img = nullptr;        // the padded parameter image + logstd, low, high
    float *d_flat = nullptr;     // staging of a host-pointer set_params
};

namespace {

using ce::fail;

int round_up(int v, int m) { return (v + m - 1) / m * m; }

// shape limits (no HIP call); `who` prefixes the message; `wide`: the limits
// of policy_wide_kernel (policy_wide_kernels.h)
int shape_ok(const char *who, const ce_policy_config *cfg, bool wide = false) {
    const int max_d = wide ? ce::kPolWideMaxD : ce::kPolMaxD;
    const int max_a = wide ? ce::kPolWideMaxA : ce::kPolMaxA;
    const std::string w(who);
    if (!cfg) return fail(CE_EINVAL, w + ": null config");
    if (cfg->abi_version != CE_ABI_VERSION) return fail(CE_EINVAL, w + ": ABI version mismatch");
    if (cfg->obs_dim <= 0 || cfg->act_dim <= 0 || cfg->n_hidden <= 0)
        return fail(CE_EINVAL, w + ": obs_dim, act_dim and n_hidden must be positive");
    if (cfg->n_hidden > ce::kPolMaxHidden)
        return fail(CE_EUNSUPPORTED, w + ": the policy takes 1 to 3 hidden layers, got " +
                                         std::to_string(cfg->n_hidden));
    if (cfg->obs_dim > max_d)
        return fail(CE_EUNSUPPORTED, w + ": obs_dim " + std::to_string(cfg->obs_dim) +
                                         " exceeds the limit of " + std::to_string(max_d));
    if (cfg->act_dim > max_a)
        return fail(CE_EUNSUPPORTED, w + ": act_dim " + std::to_string(cfg->act_dim) +
                                         " exceeds the limit of " + std::to_string(max_a));
    for (int l = 0; l < cfg->n_hidden; ++l) {
        const int h = cfg->hidden[l];
        if (h <= 0) return fail(CE_EINVAL, w + ": hidden widths must be positive");
        if (h % 32 != 0 || h > ce::kPolMaxWidth)
            return fail(CE_EUNSUPPORTED, w + ": hidden width " + std::to_string(h) +
                                             " is not a multiple of 32 up to 128");
    }
    return CE_OK;
}

int count_params(const ce_policy_config *cfg) {
    int n = 0;
    for (int net = 0; net < 2; ++net) {
        int in = cfg->obs_dim;
        for (int l = 0; l <= cfg->n_hidden; ++l) {
            const int out = l < cfg->n_hidden ? cfg->hidden[l] : (net == 0 ? cfg->act_dim : 1);
            n += in * out + out;
            in = out;
        }
    }
    return n + cfg->act_dim;
}

// the image layout, the pack table and the kernel's shape arguments
void plan(ce_policy *p) {
    const ce_policy_config &c = p->cfg;
    ce::PolicyArgs &a = p->args;
    ce::PolicyPack &k = p->pack;
    a.D = c.obs_dim;
    a.A = c.act_dim;
    a.n_hidden = c.n_hidden;
    int img = 0, src = 0, seg = 0, wmax = 0, kmax = 0;
    auto add = [&](int rows, int cols, int rows_pad, int cols_pad) {
        k.dst[seg] = img;
        k.src[seg] = src;
        k.rows[seg] = rows;
        k.cols[seg] = cols;
        k.rows_pad[seg] = rows_pad;
        k.cols_pad[seg] = cols_pad;
        ++seg;
        src += rows * cols;
        const int at = img;
        img += rows_pad * cols_pad;
        return at;
    };
    for (int net = 0; net < 2; ++net) {
        int in = c.obs_dim;
        for (int l = 0; l <= c.n_hidden; ++l) {
            const int out = l < c.n_hidden ? c.hidden[l] : (net == 0 ? c.act_dim : 1);
            const int ip = round_up(in, 4), op = round_up(out, 32);
            a.in_pad[l] = ip;
            a.out_pad[net][l] = op;
            a.off_w[net][l] = add(in, out, ip, op);
            a.off_b[net][l] = add(1, out, 1, op);
            // one stage holds at most a 128 x 128 chunk (a wide handle's first
            // layer and head: policy_wide_kernels.h)
            wmax = std::max(wmax, std::min(ip, ce::kPolChunk) * std::min(op, ce::kPolChunk));
            kmax = std::max(kmax, std::min(ip, ce::kPolChunk));
            in = out;
        }
    }
    a.off_logstd = add(1, c.act_dim, 1, round_up(c.act_dim, 4));
    k.n = seg;
    a.off_low = img;
    img += round_up(c.act_dim, 4);
    a.off_high = img;
    img += round_up(c.act_dim, 4);
    p->n_params = src;
    p->img_floats = img;
    a.w_floats = wmax;
    a.act_floats = kmax * ce::kPolLd;
    p->lds_bytes = static_cast<size_t>(wmax + 2 * a.act_floats) * sizeof(float);
}

// the generated instance's noise tile: 32 rows x round4(A) floats
size_t gen_lds_bytes(int act_dim) {
    return static_cast<size_t>(ce::kPolTile) * round_up(act_dim, 4) * sizeof(float);
}

// the wide generated instance's: one head chunk of it
size_t gen_wide_lds_bytes(int act_dim) {
    return gen_lds_bytes(std::min(act_dim, ce::kPolChunk));
}

// what both creates do after the shape check
int create(const char *who, const ce_policy_config *cfg, bool wide, ce_policy **out) {
    const std::string w(who);
    ce_policy *p = new (std::nothrow) ce_policy();
    if (!p) return fail(CE_ENOMEM, w + ": host allocation failed");
    p->cfg = *cfg;
    p->wide = wide;
    plan(p);
    auto bail = [&](int code) {
        ce_policy_destroy(p);
        return code;
    };
    CE_TRY(hipSetDevice(cfg->device));
    // the limits' need; the same for both kernels: a 128 x 128 stage and two
    // 128-wide activation buffers
    const size_t max_lds = (ce::kPolMaxWidth * ce::kPolMaxWidth +
                            2 * ce::kPolMaxWidth * ce::kPolLd) * sizeof(float);
    if (wide) {
        CE_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(ce::policy_wide_kernel<false>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize,
                                   static_cast<int>(max_lds)));
        CE_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(ce::policy_wide_kernel<true>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize,
                                   static_cast<int>(max_lds + gen_wide_lds_bytes(ce::kPolWideMaxA))));
    } else {
        CE_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(ce::policy_mlp_kernel<false>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize,
                                   static_cast<int>(max_lds)));
        CE_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(ce::policy_mlp_kernel<true>),
                                   hipFuncAttributeMaxDynamicSharedMemorySize,
                                   static_cast<int>(max_lds + gen_lds_bytes(ce::kPolMaxA))));
    }
    CE_TRY(hipMalloc(&p->img, p->img_floats * sizeof(float)));
    CE_TRY(hipMalloc(&p->d_flat, p->n_params * sizeof(float)));
    // zero parameters, unbounded actions
    std::vector<float> init(p->img_floats, 0.0f);
    for (int c = 0; c < cfg->act_dim; ++c) {
        init[p->args.off_low + c] = -INFINITY;
        init[p->args.off_high + c] = INFINITY;
    }
    CE_TRY(hipMemcpy(p->img, init.data(), init.size() * sizeof(float), hipMemcpyHostToDevice));
    p->args.img = p->img;
    *out = p;
    return CE_OK;
}

bool complete(const ce_policy_outputs *o) {
    return o && o->action && o->env_action && o->neglogp && o->value;
}

}  // namespace

namespace ce {

void policy_dims(const ce_policy *p, int *obs_dim, int *act_dim) {
    *obs_dim = p->cfg.obs_dim;
    *act_dim = p->cfg.act_dim;
}

PolicyPlan policy_plan(const ce_policy *p) {
    static_assert(kPlanLayers == kPolLayers && kPlanSegs == kPolSegs, "plan sizes");
    static_assert(kPlanWideMaxD == kPolWideMaxD && kPlanWideMaxA == kPolWideMaxA,
                  "a wide handle and a wide learner have the same limits");
    const PolicyArgs &a = p->args;
    PolicyPlan q{};
    q.D = a.D;
    q.A = a.A;
    q.n_hidden = a.n_hidden;
    for (int l = 0; l < kPolLayers; ++l) {
        q.in_pad[l] = a.in_pad[l];
        for (int net = 0; net < 2; ++net) {
            q.out_pad[net][l] = a.out_pad[net][l];
            q.off_w[net][l] = a.off_w[net][l];
            q.off_b[net][l] = a.off_b[net][l];
        }
    }
    q.off_logstd = a.off_logstd;
    q.n_segs = p->pack.n;
    for (int s = 0; s < p->pack.n; ++s) {
        q.seg_dst[s] = p->pack.dst[s];
        q.seg_src[s] = p->pack.src[s];
        q.seg_cols[s] = p->pack.cols[s];
        q.seg_cols_pad[s] = p->pack.cols_pad[s];
    }
    q.n_params = p->n_params;
    q.img_floats = p->img_floats;
    q.device = p->cfg.device;
    q.wide = p->wide ? 1 : 0;
    q.img = p->img;
    return q;
}

void policy_repack(const ce_policy *p, const float *flat, hipStream_t stream) {
    hipLaunchKernelGGL(policy_pack_kernel, dim3(p->pack.n), dim3(256), 0, stream, p->pack, flat,
                       p->img);
}

void policy_launch(const ce_policy *p, const float *obs, const PolicyNoise &noise, int64_t rows,
                   const ce_policy_outputs &out, hipStream_t stream) {
    PolicyArgs a = p->args;
    a.rows = static_cast<int>(rows);
    a.obs = obs;
    a.noise = noise.generated ? nullptr : noise.ptr;
    a.seed_lo = static_cast<uint32_t>(noise.seed);
    a.seed_hi = static_cast<uint32_t>(noise.seed >> 32);
    a.t = noise.t0;
    a.row0 = noise.row0;
    a.action = out.action;
    a.env_action = out.env_action;
    a.neglogp = out.neglogp;
    a.value = out.value;
    const dim3 grid(static_cast<unsigned>((rows + kPolTile - 1) / kPolTile), 2);
    if (p->wide) {
        if (noise.generated)
            hipLaunchKernelGGL(policy_wide_kernel<true>, grid, dim3(kPolBlock),
                               p->lds_bytes + gen_wide_lds_bytes(a.A), stream, a);
        else
            hipLaunchKernelGGL(policy_wide_kernel<false>, grid, dim3(kPolBlock), p->lds_bytes,
                               stream, a);
        return;
    }
    if (noise.generated)
        hipLaunchKernelGGL(policy_mlp_kernel<true>, grid, dim3(kPolBlock),
                           p->lds_bytes + gen_lds_bytes(a.A), stream, a);
    else
        hipLaunchKernelGGL(policy_mlp_kernel<false>, grid, dim3(kPolBlock), p->lds_bytes, stream, a);
}

int policy_rng_args_ok(const char *who, int64_t k, int64_t rows, uint32_t t0, uint32_t row0) {
    const std::string w(who);
    if (k > 0 && static_cast<uint64_t>(t0) + static_cast<uint64_t>(k) > (uint64_t(1) << 32))
        return fail(CE_EINVAL, w + ": draws t0 .. t0 + k - 1 must stay below 2^32");
    if (rows > 0 && static_cast<uint64_t>(row0) + static_cast<uint64_t>(rows) > (uint64_t(1) << 32))
        return fail(CE_EINVAL, w + ": rows row0 .. row0 + rows - 1 must stay below 2^32");
    return CE_OK;
}

int rng_replay_args_ok(const char *who, int64_t steps, int64_t n, int64_t size, uint32_t t0) {
    const auto bad = [who](const std::string &what) { return fail(CE_EINVAL, who + what); };
    if (steps < 1) return bad(": steps must be at least 1, got " + std::to_string(steps));
    if (n < 1 || n > (int64_t(1) << 24))
        return bad(": n must be in [1, 2^24], got " + std::to_string(n));
    if (size < 1 || size > (int64_t(1) << 24))
        return bad(": size must be in [1, 2^24], got " + std::to_string(size));
    if (static_cast<uint64_t>(t0) + static_cast<uint64_t>(steps) > (uint64_t(1) << 32))
        return bad(": draws t0 .. t0 + steps - 1 must stay below 2^32");
    if (steps * ((n + 3) / 4) > (int64_t(1) << 31) || steps * n > (int64_t(1) << 31))
        return bad(": steps * n is too large for one launch");
    return CE_OK;
}

void rng_enqueue_replay(int32_t *out, int64_t steps, int64_t n, int64_t size, uint64_t seed,
                        uint32_t t0, hipStream_t stream) {
    const int64_t nb = (n + 3) / 4, total = steps * nb;
    hipLaunchKernelGGL(rng_replay_kernel, dim3(static_cast<unsigned>((total + 255) / 256)),
                       dim3(256), 0, stream, out, static_cast<long long>(total),
                       static_cast<int>(nb), static_cast<int>(n), static_cast<uint32_t>(size),
                       static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), t0);
}

ce_policy_outputs policy_advance(const ce_policy_outputs &o, int64_t bytes) {
    auto adv = [bytes](float *q) { return reinterpret_cast<float *>(reinterpret_cast<char *>(q) + bytes); };
    return ce_policy_outputs{adv(o.action), adv(o.env_action), adv(o.neglogp), adv(o.value)};
}

int policy_rollout_args_ok(const char *who, const ce_policy *p, int engine_obs_dim,
                           int engine_act_dim, int32_t k, const float *obs0, const float *noise,
                           int64_t noise_stride, int64_t rows, const void *env_obs,
                           int64_t out_step_bytes, const ce_policy_outputs *pout,
                           int64_t pout_step_bytes) {
    const std::string w(who);
    if (!p) return fail(CE_EINVAL, w + ": null policy");
    if (k <= 0 || !obs0) return fail(CE_EINVAL, w + ": k must be positive and obs0 set");
    if (!complete(pout)) return fail(CE_EINVAL, w + ": policy outputs must all be set");
    if (p->cfg.obs_dim != engine_obs_dim || p->cfg.act_dim != engine_act_dim)
        return fail(CE_EINVAL, w + ": the policy maps " + std::to_string(p->cfg.obs_dim) + " -> " +
                                   std::to_string(p->cfg.act_dim) + ", the engine's rows are " +
                                   std::to_string(engine_obs_dim) + " -> " +
                                   std::to_string(engine_act_dim));
    if (noise && (noise_stride < 0 || (k > 1 && noise_stride != 0 &&
                                       noise_stride < rows * p->cfg.act_dim)))
        return fail(CE_EINVAL, w + ": noise_stride must be 0 or at least rows * act_dim");
    if (out_step_bytes < 0 || out_step_bytes % 16 != 0 ||
        (reinterpret_cast<uintptr_t>(env_obs) & 15) != 0)
        return fail(CE_EINVAL, w + ": obs must be 16-byte aligned and out_step_bytes a "
                                   "non-negative multiple of 16");
    if (pout_step_bytes < 0 || pout_step_bytes % 16 != 0)
        return fail(CE_EINVAL, w + ": pout_step_bytes must be a non-negative multiple of 16");
    return CE_OK;
}

}  // namespace ce

extern "C" {

int ce_policy_n_params(const ce_policy_config *cfg) {
    const int rc = shape_ok("ce_policy_n_params", cfg);
    return rc != CE_OK ? rc : count_params(cfg);
}

int ce_policy_create(const ce_policy_config *cfg, ce_policy **out) {
    if (!cfg || !out) return fail(CE_EINVAL, "ce_policy_create: null argument");
    *out = nullptr;
    int rc = shape_ok("ce_policy_create", cfg);
    if (rc != CE_OK) return rc;
    return create("ce_policy_create", cfg, false, out);
}

int ce_policy_wide_n_params(const ce_policy_config *cfg) {
    const int rc = shape_ok("ce_policy_wide_n_params", cfg, true);
    return rc != CE_OK ? rc : count_params(cfg);
}

int ce_policy_create_wide(const ce_policy_config *cfg, ce_policy **out) {
    if (!cfg || !out) return fail(CE_EINVAL, "ce_policy_create_wide: null argument");
    *out = nullptr;
    const int rc = shape_ok("ce_policy_create_wide", cfg, true);
    if (rc != CE_OK) return rc;
    return create("ce_policy_create_wide", cfg, true, out);
}

void ce_policy_destroy(ce_policy *p) {
    if (!p) return;
    if (p->img) (void)hipFree(p->img);
    if (p->d_flat) (void)hipFree(p->d_flat);
    delete p;
}

int ce_policy_set_params(ce_policy *p, const float *flat, int64_t n, uint32_t flags,
                         void *hip_stream) {
    if (!p || !flat) return fail(CE_EINVAL, "ce_policy_set_params: null argument");
    if (n != p->n_params)
        return fail(CE_EINVAL, "ce_policy_set_params: got " + std::to_string(n) +
                                   " parameters, the policy has " + std::to_string(p->n_params));
    CE_CLEAR_STALE_ERROR();
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const bool dev = (flags & CE_PTR_DEVICE) != 0;
    if (!dev) {
        CE_HIP(hipMemcpyAsync(p->d_flat, flat, n * sizeof(float), hipMemcpyHostToDevice, stream));
        CE_HIP(hipStreamSynchronize(stream));   // `flat` may be pageable
    }
    hipLaunchKernelGGL(ce::policy_pack_kernel, dim3(p->pack.n), dim3(256), 0, stream, p->pack,
                       dev ? flat : p->d_flat, p->img);
    CE_HIP(hipGetLastError());
    if (!dev) CE_HIP(hipStreamSynchronize(stream));
    return CE_OK;
}

int ce_policy_set_bounds(ce_policy *p, const float *low, const float *high) {
    if (!p) return fail(CE_EINVAL, "ce_policy_set_bounds: null policy");
    const int A = p->cfg.act_dim;
    std::vector<float> lo(A, -INFINITY), hi(A, INFINITY);
    for (int c = 0; c < A; ++c) {
        if (low) lo[c] = low[c];
        if (high) hi[c] = high[c];
        if (!(lo[c] <= hi[c])) return fail(CE_EINVAL, "ce_policy_set_bounds: low must be <= high");
    }
    CE_CLEAR_STALE_ERROR();
    CE_HIP(hipMemcpy(p->img + p->args.off_low, lo.data(), A * sizeof(float), hipMemcpyHostToDevice));
    CE_HIP(hipMemcpy(p->img + p->args.off_high, hi.data(), A * sizeof(float), hipMemcpyHostToDevice));
    return CE_OK;
}

int ce_policy_forward(const ce_policy *p, const float *obs, const float *noise, int64_t rows,
                      const ce_policy_outputs *out, void *hip_stream) {
    if (!p || !obs) return fail(CE_EINVAL, "ce_policy_forward: null argument");
    if (!complete(out)) return fail(CE_EINVAL, "ce_policy_forward: policy outputs must all be set");
    if (rows < 1 || rows > (int64_t(1) << 24))
        return fail(CE_EINVAL, "ce_policy_forward: rows must be in [1, 2^24]");
    CE_CLEAR_STALE_ERROR();
    ce::policy_launch(p, obs, ce::PolicyNoise::block(noise, 0), rows, *out,
                      static_cast<hipStream_t>(hip_stream));
    CE_HIP(hipGetLastError());
    return CE_OK;
}

int ce_policy_forward_rng(const ce_policy *p, const float *obs, uint64_t seed, uint32_t t,
                          uint32_t row0, int64_t rows, const ce_policy_outputs *out,
                          void *hip_stream) {
    if (!p || !obs) return fail(CE_EINVAL, "ce_policy_forward_rng: null argument");
    if (!complete(out))
        return fail(CE_EINVAL, "ce_policy_forward_rng: policy outputs must all be set");
    if (rows < 1 || rows > (int64_t(1) << 24))
        return fail(CE_EINVAL, "ce_policy_forward_rng: rows must be in [1, 2^24]");
    const int rc = ce::policy_rng_args_ok("ce_policy_forward_rng", 1, rows, t, row0);
    if (rc != CE_OK) return rc;
    CE_CLEAR_STALE_ERROR();
    ce::policy_launch(p, obs, ce::PolicyNoise::rng(seed, t, row0), rows, *out,
                      static_cast<hipStream_t>(hip_stream));
    CE_HIP(hipGetLastError());
    return CE_OK;
}

// ce_rng_normal (purpose < 0: the policy-noise kernel, as before) and
// ce_rng_normal_purpose
static int rng_normal_entry(const char *who, float *out, int32_t k, int64_t rows, int32_t act_dim,
                            int64_t record_stride_bytes, uint64_t seed, uint32_t t0, uint32_t row0,
                            int64_t purpose, void *hip_stream, int max_act = ce::kPolMaxA) {
    const auto bad = [who](const std::string &what) { return fail(CE_EINVAL, who + what); };
    if (!out) return bad(": null output");
    if (k < 1) return bad(": k must be at least 1, got " + std::to_string(k));
    if (rows < 1 || rows > (int64_t(1) << 24))
        return bad(": rows must be in [1, 2^24], got " + std::to_string(rows));
    if (act_dim < 1 || act_dim > max_act)
        return bad(": act_dim must be in [1, " + std::to_string(max_act) + "], got " +
                   std::to_string(act_dim));
    if (record_stride_bytes % 4 != 0 || record_stride_bytes < rows * act_dim * 4)
        return bad(": record_stride_bytes must be a multiple of 4 of at least rows * act_dim * 4");
    if (reinterpret_cast<uintptr_t>(out) & 3) return bad(": the output must be 4-byte aligned");
    const int rc = ce::policy_rng_args_ok(who, k, rows, t0, row0);
    if (rc != CE_OK) return rc;
    const int64_t total = int64_t(k) * rows * ((act_dim + 3) / 4);
    const int64_t blocks = (total + 255) / 256;
    if (blocks > 0x7fffffff) return bad(": k * rows * act_dim is too large for one launch");
    CE_CLEAR_STALE_ERROR_AT(who);
    const dim3 grid(static_cast<unsigned>(blocks));
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const long long stride = record_stride_bytes / 4;
    const uint32_t lo = static_cast<uint32_t>(seed), hi = static_cast<uint32_t>(seed >> 32);
    if (purpose < 0)
        hipLaunchKernelGGL(ce::rng_normal_kernel, grid, dim3(256), 0, stream, out,
                           static_cast<long long>(total), static_cast<int>(rows), act_dim, stride,
                           lo, hi, t0, row0);
    else
        hipLaunchKernelGGL(ce::rng_normal_purpose_kernel, grid, dim3(256), 0, stream, out,
                           static_cast<long long>(total), static_cast<int>(rows), act_dim, stride,
                           lo, hi, t0, row0, static_cast<uint32_t>(purpose));
    CE_HIP(hipGetLastError());
    return CE_OK;
}

int ce_rng_normal(float *out, int32_t k, int64_t rows, int32_t act_dim,
                  int64_t record_stride_bytes, uint64_t seed, uint32_t t0, uint32_t row0,
                  void *hip_stream) {
    return rng_normal_entry("ce_rng_normal", out, k, rows, act_dim, record_stride_bytes, seed, t0,
                            row0, -1, hip_stream);
}

int ce_rng_normal_wide(float *out, int32_t k, int64_t rows, int32_t act_dim,
                       int64_t record_stride_bytes, uint64_t seed, uint32_t t0, uint32_t row0,
                       void *hip_stream) {
    return rng_normal_entry("ce_rng_normal_wide", out, k, rows, act_dim, record_stride_bytes, seed,
                            t0, row0, -1, hip_stream, ce::kPolWideMaxA);
}

int ce_rng_normal_purpose(float *out, int32_t k, int64_t rows, int32_t act_dim,
                          int64_t record_stride_bytes, uint64_t seed, uint32_t purpose, uint32_t t0,
                          uint32_t row0, void *hip_stream) {
    return rng_normal_entry("ce_rng_normal_purpose", out, k, rows, act_dim, record_stride_bytes,
                            seed, t0, row0, purpose, hip_stream);
}

int ce_rng_replay(int32_t *out, int64_t steps, int64_t n, int64_t size, uint64_t seed, uint32_t t0,
                  void *hip_stream) {
    const char *who = "ce_rng_replay";
    if (!out) return fail(CE_EINVAL, std::string(who) + ": null output");
    if (reinterpret_cast<uintptr_t>(out) & 3)
        return fail(CE_EINVAL, std::string(who) + ": the output must be 4-byte aligned");
    const int rc = ce::rng_replay_args_ok(who, steps, n, size, t0);
    if (rc != CE_OK) return rc;
    CE_CLEAR_STALE_ERROR();
    ce::rng_enqueue_replay(out, steps, n, size, seed, t0, static_cast<hipStream_t>(hip_stream));
    CE_HIP(hipGetLastError());
    return CE_OK;
}

int ce_rng_u32(uint32_t *out, int64_t n, uint64_t seed, uint32_t purpose, uint32_t t,
               void *hip_stream) {
    const char *who = "ce_rng_u32";
    const auto bad = [who](const std::string &what) { return fail(CE_EINVAL, who + what); };
    if (!out) return bad(": null output");
    if (n < 1 || n > (int64_t(1) << 31))
        return bad(": n must be in [1, 2^31], got " + std::to_string(n));
    if (reinterpret_cast<uintptr_t>(out) & 3) return bad(": the output must be 4-byte aligned");
    CE_CLEAR_STALE_ERROR();
    const int64_t blocks = ((n + 3) / 4 + 255) / 256;
    hipLaunchKernelGGL(ce::rng_u32_kernel, dim3(static_cast<unsigned>(blocks)), dim3(256), 0,
                       static_cast<hipStream_t>(hip_stream), out, static_cast<long long>(n),
                       static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32), purpose, t);
    CE_HIP(hipGetLastError());
    return CE_OK;
}

}  // extern "C"
