// The device-side VecNormalize (ce_vecnorm_* in include/custom_envs_amd.h) as
// the engines see it: ce_rollout_policy_vecnorm (engine.hip) and
// ce_multi_rollout_policy_vecnorm (multi_engine.hip) enqueue
// [policy, env step, normaliser] x K through these.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/custom_envs_amd.h"
#include "policy_engine.h"

namespace ce {

// What host_rollout_policy needs of a normalised rollout: the normaliser, the
// [k + 1] normalised observation slots (slot 0 the caller's) and the [k]
// normalised reward records.
struct VecnormRollout {
    ce_vecnorm *vn = nullptr;
    float *obs_norm = nullptr;
    int64_t obs_step = 0;        // bytes between slots
    float *reward_norm = nullptr;
    int64_t reward_step = 0;     // bytes between records
    uint32_t flags = 0;          // CE_VECNORM_TRAINING

    float *obs_slot(int s) const {
        return reinterpret_cast<float *>(reinterpret_cast<char *>(obs_norm) + s * obs_step);
    }
    float *reward_slot(int s) const {
        return reinterpret_cast<float *>(reinterpret_cast<char *>(reward_norm) + s * reward_step);
    }
};

// The checks of a normalised rollout that read no handle (null pointers, k,
// strides and alignment), in that order; `engine_set`: the engine handle is
// not null.  CE_OK or a failed status.
int vecnorm_rollout_plain_ok(const char *who, bool engine_set, const ce_policy *p,
                             const ce_vecnorm *vn, int32_t k, const float *obs_norm,
                             int64_t obs_step, const float *reward_norm, int64_t reward_step,
                             uint32_t flags, const ce_rollout_noise *noise, const void *out,
                             const void *pout);

// The normaliser's shape against the engine's rows, and the slot strides
// against that shape (no HIP call).
int vecnorm_rollout_shape_ok(const char *who, const VecnormRollout &v, int64_t rows, int obs_dim);

// The noise source of a rollout from its C form (checked by plain_ok).
PolicyNoise vecnorm_noise(const ce_rollout_noise *noise);

// Enqueue one vecnorm_step_kernel launch; arguments are NOT validated.
void vecnorm_launch(ce_vecnorm *vn, const float *obs, const float *reward, const uint8_t *done,
                    float *obs_out, float *reward_out, uint32_t flags, hipStream_t stream);

}  // namespace ce
