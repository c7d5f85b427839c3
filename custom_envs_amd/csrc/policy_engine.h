// The device-side MLP policy (ce_policy_* in include/custom_envs_amd.h) as the
// engines see it: ce_rollout_policy (engine.hip) and ce_multi_rollout_policy
// (multi_engine.hip) enqueue [policy, env step] x K through these.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/custom_envs_amd.h"

namespace ce {

// obs_dim / act_dim of a policy (no HIP call)
void policy_dims(const ce_policy *p, int *obs_dim, int *act_dim);

// Where a forward's N(0,1) noise comes from: the caller's block (`ptr`
// [rows][A], null for the deterministic policy; step s of a rollout reads
// ptr + s * stride), or, with `generated`, rng.h's stream under `seed` at
// draw t0 (+ s) for the global rows row0 .. row0 + rows - 1.
struct PolicyNoise {
    const float *ptr = nullptr;
    int64_t stride = 0;
    bool generated = false;
    uint64_t seed = 0;
    uint32_t t0 = 0, row0 = 0;

    static PolicyNoise block(const float *ptr, int64_t stride) {
        PolicyNoise n;
        n.ptr = ptr;
        n.stride = stride;
        return n;
    }
    static PolicyNoise rng(uint64_t seed, uint32_t t0, uint32_t row0) {
        PolicyNoise n;
        n.generated = true;
        n.seed = seed;
        n.t0 = t0;
        n.row0 = row0;
        return n;
    }
    // the source of step s of a rollout
    PolicyNoise at(int s) const {
        PolicyNoise n = *this;
        if (ptr) n.ptr = ptr + s * stride;
        n.t0 = t0 + static_cast<uint32_t>(s);
        return n;
    }
};

// Enqueue one policy_mlp_kernel launch -- policy_wide_kernel for a handle from
// ce_policy_create_wide, at every shape -- (the instance `noise` selects): every
// pointer a device pointer, all four outputs set, rows >= 1.  Arguments are
// NOT validated here.
void policy_launch(const ce_policy *p, const float *obs, const PolicyNoise &noise, int64_t rows,
                   const ce_policy_outputs &out, hipStream_t stream);

// The draws and rows of a generated-noise call (before any HIP call): draws
// t0 .. t0 + k - 1 and rows row0 .. row0 + rows - 1 must fit 32 bits.
int policy_rng_args_ok(const char *who, int64_t k, int64_t rows, uint32_t t0, uint32_t row0);

// The replay indices of draws t0 .. t0 + steps - 1 (rng_kernels.h:
// rng_replay_kernel), for ce_rng_replay and ce_ddpg_train.  rng_replay_args_ok
// is every check (no HIP call); rng_enqueue_replay is the one launch, its
// arguments NOT validated.
int rng_replay_args_ok(const char *who, int64_t steps, int64_t n, int64_t size, uint32_t t0);
void rng_enqueue_replay(int32_t *out, int64_t steps, int64_t n, int64_t size, uint64_t seed,
                        uint32_t t0, hipStream_t stream);

// The argument checks the two rollout entry points share (before any HIP
// call): null pointers, k, strides, alignment, the policy's shape against the
// engine's.  CE_OK or a failed status with ce_last_error set.
int policy_rollout_args_ok(const char *who, const ce_policy *p, int engine_obs_dim,
                           int engine_act_dim, int32_t k, const float *obs0, const float *noise,
                           int64_t noise_stride, int64_t rows, const void *env_obs,
                           int64_t out_step_bytes, const ce_policy_outputs *pout,
                           int64_t pout_step_bytes);

// What the learners (learner_host.h and its two users, ppo_grad_tile.h) need
// of a policy, as plain data: its shape, the offsets of its padded parameter image (every
// W zero-padded to [in_pad][out_pad], policy_engine.hip: plan), the segments
// that map the flat parameter vector into the image, and the image itself.
constexpr int kPlanLayers = 4;                  // hidden layers + the head
// the widest plan: a wide handle's limits (policy_wide_kernels.h) and the wide
// gradient kernel's (ppo_grad_wide_tile.h)
constexpr int kPlanWideMaxD = 1024, kPlanWideMaxA = 512;
constexpr int kPlanSegs = 4 * kPlanLayers + 1;  // (W, b) per layer per network + logstd
struct PolicyPlan {
    int D, A, n_hidden;
    int in_pad[kPlanLayers], out_pad[2][kPlanLayers];
    int off_w[2][kPlanLayers], off_b[2][kPlanLayers], off_logstd;
    int n_segs;                                 // logstd is the last segment
    int seg_dst[kPlanSegs], seg_src[kPlanSegs], seg_cols[kPlanSegs], seg_cols_pad[kPlanSegs];
    int n_params, img_floats, device;
    int wide;                                   // from ce_policy_create_wide: ce_<x>_create refuses it,
                                                // ce_<x>_create_wide requires it
    float *img;
};
PolicyPlan policy_plan(const ce_policy *p);

// Enqueue the repack of the device vector `flat` [n_params] into the image.
void policy_repack(const ce_policy *p, const float *flat, hipStream_t stream);

// the policy outputs of step t of a rollout
ce_policy_outputs policy_advance(const ce_policy_outputs &o, int64_t bytes);

}  // namespace ce
