// C-ABI implementation of the device-side VecNormalize (ce_vecnorm_* in
// include/custom_envs_amd.h): owns the running moments and `ret` on the device
// and enqueues vecnorm_step_kernel (vecnorm_kernels.h), one launch per step.
// Every argument check precedes the first HIP call, and the checks of the
// plain arguments precede the check of the handle, so they run without a
// device.
#include <hip/hip_runtime.h>

#include <cmath>
#include <new>
#include <string>
#include <vector>

#include "common.h"
#include "vecnorm_engine.h"
#include "vecnorm_kernels.h"

struct ce_vecnorm {
    ce_vecnorm_config cfg{};
    int rows = 0, D = 0;
    // one allocation: obs_mean [D], obs_var [D], obs_count [D] (every entry the
    // same count), ret_stat [4] (mean, var, count, pad), ret [rows]
    double *state = nullptr;
    size_t lds_bytes = 0;        // of the staged form (0: not staged)

    double *obs_mean() const { return state; }
    double *obs_var() const { return state + D; }
    double *obs_count() const { return state + 2 * size_t(D); }
    double *ret_stat() const { return state + 3 * size_t(D); }
    double *ret() const { return state + 3 * size_t(D) + 4; }
    size_t state_doubles() const { return 3 * size_t(D) + 4 + size_t(rows); }
};

namespace {

using ce::fail;

constexpr uint32_t kVnKnownFlags = CE_VECNORM_TRAINING | CE_VECNORM_RESET | CE_VECNORM_OBS_ONLY;

}  // namespace

namespace ce {

void vecnorm_launch(ce_vecnorm *vn, const float *obs, const float *reward, const uint8_t *done,
                    float *obs_out, float *reward_out, uint32_t flags, hipStream_t stream) {
    VecnormArgs a{};
    a.rows = vn->rows;
    a.D = vn->D;
    a.norm_obs = vn->cfg.norm_obs != 0;
    a.norm_reward = vn->cfg.norm_reward != 0;
    a.training = (flags & CE_VECNORM_TRAINING) != 0;
    a.reset = (flags & CE_VECNORM_RESET) != 0;
    a.staged = vn->lds_bytes != 0;
    a.clip_obs = vn->cfg.clip_obs;
    a.clip_reward = vn->cfg.clip_reward;
    a.gamma = vn->cfg.gamma;
    a.epsilon = vn->cfg.epsilon;
    a.obs = obs;
    a.reward = reward;
    a.done = done;
    a.obs_out = obs_out;
    a.reward_out = reward_out;
    a.obs_mean = vn->obs_mean();
    a.obs_var = vn->obs_var();
    a.obs_count = vn->obs_count();
    a.ret_stat = vn->ret_stat();
    a.ret = vn->ret();
    const unsigned col_blocks = static_cast<unsigned>((vn->D + kVnCols - 1) / kVnCols);
    // the last workgroup is the returns'; an obs-only call has none
    const unsigned ret_blocks = (flags & CE_VECNORM_OBS_ONLY) ? 0 : 1;
    hipLaunchKernelGGL(vecnorm_step_kernel, dim3(col_blocks + ret_blocks), dim3(kVnBlock),
                       vn->lds_bytes, stream, a);
}

PolicyNoise vecnorm_noise(const ce_rollout_noise *noise) {
    return noise->kind == CE_NOISE_GENERATED
               ? PolicyNoise::rng(noise->seed, noise->t0, noise->row0)
               : PolicyNoise::block(noise->ptr, noise->stride);
}

int vecnorm_rollout_plain_ok(const char *who, bool engine_set, const ce_policy *p,
                             const ce_vecnorm *vn, int32_t k, const float *obs_norm,
                             int64_t obs_step, const float *reward_norm, int64_t reward_step,
                             uint32_t flags, const ce_rollout_noise *noise, const void *out,
                             const void *pout) {
    const std::string w(who);
    if (!engine_set) return fail(CE_EINVAL, w + ": null engine");
    if (!p) return fail(CE_EINVAL, w + ": null policy");
    if (!vn) return fail(CE_EINVAL, w + ": null normaliser");
    if (!obs_norm || !reward_norm)
        return fail(CE_EINVAL, w + ": null normalised obs or reward buffer");
    if (!noise) return fail(CE_EINVAL, w + ": null noise source");
    if (!out || !pout) return fail(CE_EINVAL, w + ": null outputs");
    if (k <= 0) return fail(CE_EINVAL, w + ": k must be positive, got " + std::to_string(k));
    if (noise->kind != CE_NOISE_BLOCK && noise->kind != CE_NOISE_GENERATED)
        return fail(CE_EINVAL, w + ": unknown noise kind " + std::to_string(noise->kind));
    if (flags & ~static_cast<uint32_t>(CE_VECNORM_TRAINING))
        return fail(CE_EINVAL, w + ": vn_flags takes CE_VECNORM_TRAINING only");
    if ((reinterpret_cast<uintptr_t>(obs_norm) & 15) != 0 || obs_step <= 0 || obs_step % 16 != 0)
        return fail(CE_EINVAL, w + ": obs_norm must be 16-byte aligned and obs_norm_step_bytes a "
                                   "positive multiple of 16");
    if ((reinterpret_cast<uintptr_t>(reward_norm) & 3) != 0 || reward_step <= 0 ||
        reward_step % 16 != 0)
        return fail(CE_EINVAL, w + ": reward_norm must be 4-byte aligned and "
                                   "reward_norm_step_bytes a positive multiple of 16");
    return CE_OK;
}

int vecnorm_rollout_shape_ok(const char *who, const VecnormRollout &v, int64_t rows, int obs_dim) {
    const std::string w(who);
    if (v.vn->rows != rows || v.vn->D != obs_dim)
        return fail(CE_EINVAL, w + ": the normaliser holds " + std::to_string(v.vn->rows) +
                                   " rows of " + std::to_string(v.vn->D) +
                                   " columns, the engine's rows are " + std::to_string(rows) +
                                   " of " + std::to_string(obs_dim));
    if (v.obs_step < rows * obs_dim * 4)
        return fail(CE_EINVAL, w + ": obs_norm_step_bytes must be at least rows * obs_dim * 4");
    if (v.reward_step < rows * 4)
        return fail(CE_EINVAL, w + ": reward_norm_step_bytes must be at least rows * 4");
    return CE_OK;
}

}  // namespace ce

extern "C" {

int ce_vecnorm_create(const ce_vecnorm_config *cfg, ce_vecnorm **out) {
    const char *who = "ce_vecnorm_create";
    const auto bad = [who](const std::string &what) { return fail(CE_EINVAL, who + what); };
    if (!cfg || !out) return bad(": null argument");
    *out = nullptr;
    if (cfg->abi_version != CE_ABI_VERSION) return bad(": ABI version mismatch");
    if (cfg->device < 0) return bad(": device must not be negative");
    if (cfg->rows < 1 || cfg->rows > (int64_t(1) << 24))
        return bad(": rows must be in [1, 2^24], got " + std::to_string(cfg->rows));
    if (cfg->obs_dim < 1 || cfg->obs_dim > (1 << 16))
        return bad(": obs_dim must be in [1, 2^16], got " + std::to_string(cfg->obs_dim));
    if (!(cfg->clip_obs > 0.0) || !(cfg->clip_reward > 0.0))
        return bad(": clip_obs and clip_reward must be positive");
    if (!std::isfinite(cfg->gamma)) return bad(": gamma must be finite");
    if (!(cfg->epsilon >= 0.0) || !std::isfinite(cfg->epsilon))
        return bad(": epsilon must be finite and not negative");
    ce_vecnorm *vn = new (std::nothrow) ce_vecnorm();
    if (!vn) return fail(CE_ENOMEM, std::string(who) + ": out of host memory");
    vn->cfg = *cfg;
    vn->rows = static_cast<int>(cfg->rows);
    vn->D = cfg->obs_dim;
    if (vn->rows <= ce::kVnStageRows)
        vn->lds_bytes = static_cast<size_t>(vn->rows) * ce::kVnCols * sizeof(float);
    const auto bail = [vn](int code) {
        ce_vecnorm_destroy(vn);
        return code;
    };
    CE_CLEAR_STALE_ERROR();
    CE_TRY(hipSetDevice(cfg->device));
    CE_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(ce::vecnorm_step_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize,
                               static_cast<int>(ce::kVnStageRows * ce::kVnCols * sizeof(float))));
    CE_TRY(hipMalloc(&vn->state, vn->state_doubles() * sizeof(double)));
    std::vector<double> init(vn->state_doubles(), 0.0);
    for (int c = 0; c < vn->D; ++c) {
        init[vn->D + c] = 1.0;
        init[2 * size_t(vn->D) + c] = 1e-4;
    }
    init[3 * size_t(vn->D) + 1] = 1.0;
    init[3 * size_t(vn->D) + 2] = 1e-4;
    CE_TRY(hipMemcpy(vn->state, init.data(), init.size() * sizeof(double), hipMemcpyHostToDevice));
    *out = vn;
    return CE_OK;
}

void ce_vecnorm_destroy(ce_vecnorm *vn) {
    if (!vn) return;
    if (vn->state) (void)hipFree(vn->state);
    delete vn;
}

int ce_vecnorm_step(ce_vecnorm *vn, const float *obs, const float *reward, const uint8_t *done,
                    float *obs_out, float *reward_out, uint32_t flags, void *hip_stream) {
    const char *who = "ce_vecnorm_step";
    const auto bad = [who](const std::string &what) { return fail(CE_EINVAL, who + what); };
    if (flags & ~kVnKnownFlags) return bad(": unknown flags");
    if ((flags & CE_VECNORM_OBS_ONLY) && (flags & (CE_VECNORM_TRAINING | CE_VECNORM_RESET)))
        return bad(": CE_VECNORM_OBS_ONLY goes with neither TRAINING nor RESET");
    if (!obs || !obs_out) return bad(": null obs or obs_out");
    if (!(flags & (CE_VECNORM_RESET | CE_VECNORM_OBS_ONLY)) && (!reward || !done || !reward_out))
        return bad(": null reward, done or reward_out (only RESET and OBS_ONLY take none)");
    if ((reinterpret_cast<uintptr_t>(obs) | reinterpret_cast<uintptr_t>(obs_out) |
         reinterpret_cast<uintptr_t>(reward) | reinterpret_cast<uintptr_t>(reward_out)) & 3)
        return bad(": obs, obs_out, reward and reward_out must be 4-byte aligned");
    if (!vn) return bad(": null normaliser");
    CE_CLEAR_STALE_ERROR();
    ce::vecnorm_launch(vn, obs, reward, done, obs_out, reward_out, flags,
                       static_cast<hipStream_t>(hip_stream));
    CE_HIP(hipGetLastError());
    return CE_OK;
}

static int vecnorm_state_copy(const char *who, ce_vecnorm *vn, double *obs_mean, double *obs_var,
                              double *obs_count, double *ret_mean, double *ret_var,
                              double *ret_count, double *ret, bool set, void *hip_stream) {
    const auto bad = [who](const std::string &what) { return fail(CE_EINVAL, who + what); };
    if (!obs_mean || !obs_var || !obs_count) return bad(": null observation moments");
    if (!ret_mean || !ret_var || !ret_count) return bad(": null return moments");
    if (!ret) return bad(": null ret");
    if (!vn) return bad(": null normaliser");
    CE_CLEAR_STALE_ERROR_AT(who);
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const size_t D = static_cast<size_t>(vn->D), n = vn->state_doubles();
    std::vector<double> host(n, 0.0);
    if (set) {
        for (size_t c = 0; c < D; ++c) {
            host[c] = obs_mean[c];
            host[D + c] = obs_var[c];
            host[2 * D + c] = *obs_count;
        }
        host[3 * D] = *ret_mean;
        host[3 * D + 1] = *ret_var;
        host[3 * D + 2] = *ret_count;
        for (int r = 0; r < vn->rows; ++r) host[3 * D + 4 + r] = ret[r];
        CE_HIP(hipMemcpyAsync(vn->state, host.data(), n * sizeof(double), hipMemcpyHostToDevice,
                              stream));
        CE_HIP(hipStreamSynchronize(stream));      // `host` is pageable
        return CE_OK;
    }
    CE_HIP(hipMemcpyAsync(host.data(), vn->state, n * sizeof(double), hipMemcpyDeviceToHost,
                          stream));
    CE_HIP(hipStreamSynchronize(stream));
    for (size_t c = 0; c < D; ++c) {
        obs_mean[c] = host[c];
        obs_var[c] = host[D + c];
    }
    *obs_count = host[2 * D];
    *ret_mean = host[3 * D];
    *ret_var = host[3 * D + 1];
    *ret_count = host[3 * D + 2];
    for (int r = 0; r < vn->rows; ++r) ret[r] = host[3 * D + 4 + r];
    return CE_OK;
}

int ce_vecnorm_get_state(ce_vecnorm *vn, double *obs_mean, double *obs_var, double *obs_count,
                         double *ret_mean, double *ret_var, double *ret_count, double *ret,
                         void *hip_stream) {
    return vecnorm_state_copy("ce_vecnorm_get_state", vn, obs_mean, obs_var, obs_count, ret_mean,
                              ret_var, ret_count, ret, false, hip_stream);
}

int ce_vecnorm_set_state(ce_vecnorm *vn, const double *obs_mean, const double *obs_var,
                         const double *obs_count, const double *ret_mean, const double *ret_var,
                         const double *ret_count, const double *ret, void *hip_stream) {
    return vecnorm_state_copy("ce_vecnorm_set_state", vn, const_cast<double *>(obs_mean),
                              const_cast<double *>(obs_var), const_cast<double *>(obs_count),
                              const_cast<double *>(ret_mean), const_cast<double *>(ret_var),
                              const_cast<double *>(ret_count), const_cast<double *>(ret), true,
                              hip_stream);
}

}  // extern "C"
