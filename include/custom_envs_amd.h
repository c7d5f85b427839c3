/*
 * custom_envs_amd -- C ABI of the MI355X vectorised Optimize-v0 engine.
 *
 * The reference (adolfogonzalez3/custom_envs) is pure Python and has no FFI;
 * every entry point below replaces one Python-level interface on the hot
 * path, cited as file:line relative to the reference root:
 *
 *   ce_create      Optimize.__init__            custom_envs/envs/optimize.py:40-56
 *                  + ConcurrentVecEnv.__init__   custom_envs/vectorize/concurrentvecenv.py:77-95
 *   ce_seed        BaseEnvironment.seed          custom_envs/envs/baseenvironment.py:20-28
 *   ce_seed_draws / ce_seed_draws_mlp
 *                  Optimize.base_reset draws     custom_envs/envs/optimize.py:63-64
 *                  (model.reset then sequence.shuffle under use_random_state,
 *                   custom_envs/utils/utils_math.py:9-22)
 *   ce_reset       ConcurrentVecEnv.reset        custom_envs/vectorize/concurrentvecenv.py:109-113
 *                  -> BaseEnvironment.reset       custom_envs/envs/baseenvironment.py:43-49
 *   ce_step        VecEnv.step = step_async+step_wait
 *                                                custom_envs/vectorize/concurrentvecenv.py:97-107
 *                  -> _worker 'step' + auto-reset custom_envs/utils/utils_venv.py:24-56 (:31)
 *                  -> BaseEnvironment.step        custom_envs/envs/baseenvironment.py:30-41
 *                  -> Optimize.base_step          custom_envs/envs/optimize.py:69-100
 *   ce_step_async  ConcurrentVecEnv.step_async   custom_envs/vectorize/concurrentvecenv.py:97-100
 *   ce_wait        ConcurrentVecEnv.step_wait    custom_envs/vectorize/concurrentvecenv.py:102-107
 *   ce_step_many   K consecutive VecEnv.step calls with device-resident actions
 *                  (benchmark / GPU-resident agent mode; one hipGraph)
 *   ce_step_many_prepare
 *                  instantiate + upload that hipGraph without running it (graphs
 *                  are cached per (k, actions, stride, outputs, stream), so a
 *                  timed region never captures)
 *   ce_step_many_strided
 *                  K consecutive VecEnv.step calls in ONE persistent launch
 *                  (concurrentvecenv.py:94-107 x K over optimize.py:69-100 and
 *                  the utils_venv.py:31 auto-reset), step t's outputs into
 *                  record t of a [K] output slab (a device-resident rollout)
 *   ce_set_persistent / ce_step_many_kernel
 *                  choose / name the K-step launch form (no reference analogue)
 *   ce_get_state / ce_set_state
 *                  the per-env attributes model.weights, loss_hist, grad_hist,
 *                  current_step (optimize.py:45-50, baseenvironment.py:18)
 *   ce_destroy     ConcurrentVecEnv.close        custom_envs/vectorize/concurrentvecenv.py:115-125
 *
 * Multi-agent learning-rate path (MultiOptLRs-v0 under OptVecEnv):
 *   ce_multi_create  MultiOptLRs.__init__        custom_envs/envs/multioptlrs.py:39-61
 *                    + OptVecEnv.__init__         custom_envs/vectorize/optvecenv.py:57-68
 *                    + OptimizeFunction.__init__  custom_envs/problems/optimize_function.py:20-61
 *   ce_multi_reset   OptVecEnv.reset              custom_envs/vectorize/optvecenv.py:90-91
 *                    -> MultiOptLRs.base_reset    custom_envs/envs/multioptlrs.py:66-78
 *   ce_multi_step    OptVecEnv.step_async/wait    custom_envs/vectorize/optvecenv.py:70-88
 *                    -> OptEnvRunner.step         custom_envs/vectorize/optvecenv.py:38-46
 *                    -> MultiOptLRs.base_step     custom_envs/envs/multioptlrs.py:80-129
 *   ce_multi_step_async / ce_multi_wait / ce_multi_step_many(_prepare) / ce_multi_host_outputs /
 *   ce_multi_get_state / ce_multi_set_stream / ce_multi_destroy /
 *   ce_multi_step_many_strided / ce_multi_set_persistent / ce_multi_step_many_kernel:
 *                    as for Optimize-v0.
 *
 * MultiOptLRs-v0 over the neural-network problem (get_problem('nn')):
 *   ce_nn_create     MultiOptLRs.__init__(problem='nn')  multioptlrs.py:39-61
 *                    + OptimizeNN.__init__        custom_envs/problems/optimize_nn.py:22-64
 *                      (create_neural_net layers, custom_envs/utils/utils_tf.py:74-86)
 *                    + OptVecEnv.__init__         optvecenv.py:57-68
 *   ce_nn_seed       BaseEnvironment.seed         baseenvironment.py:20-28
 *   ce_nn_seed_draws the reset's kernel init + shuffle and the epoch-end shuffle
 *                    (optimize_nn.py:102-120 under use_random_state)
 *   ce_nn_reset      OptVecEnv.reset -> MultiOptLRs.base_reset  multioptlrs.py:66-78
 *   ce_nn_step       OptVecEnv.step -> MultiOptLRs.base_step    multioptlrs.py:80-129
 *                    (+ OptimizeNN.get_gradient/get/next, optimize_nn.py:102-159)
 *   ce_nn_step_async / ce_nn_wait / ce_nn_step_many(_prepare) / ce_nn_host_outputs /
 *   ce_nn_get_state / ce_nn_set_stream / ce_nn_destroy / ce_nn_n_params:
 *                    as for ce_multi_*.
 *
 * The agent's policy on the device (stable-baselines MlpPolicy as PPO2 / A2C run
 * it, run_multiagent_exp_single.py:37-49):
 *   ce_policy_create / _destroy / _n_params / _set_params / _set_bounds
 *                    the actor-critic network, its flat parameters and bounds
 *   ce_policy_create_wide / ce_policy_wide_n_params
 *                    the same handle for obs_dim <= 1024, act_dim <= 512 (the
 *                    reference's 981 -> 490 default shape); trained through
 *                    ce_ppo2_create_wide / ce_a2c_create_wide
 *   ce_policy_forward  one fused launch: action, env_action, neglogp, value
 *   ce_rollout_policy / ce_multi_rollout_policy
 *                    K x (policy forward, VecEnv.step) from one call, the
 *                    runner's inner loop with no host work between steps
 *
 * Conventions
 *   - Every function returns CE_OK (0) or a negative ce_status; nothing
 *     throws across the ABI.  ce_last_error() returns a thread-local message.
 *   - The engine owns all device memory (dataset, per-env state).  The caller
 *     owns the buffers it passes in.  With CE_PTR_DEVICE the caller's
 *     pointers are device pointers and the call is stream-ordered
 *     (asynchronous) on the engine stream (ce_set_stream); otherwise they are
 *     host pointers and the call synchronises before returning.
 *   - One engine per host thread; calls on one engine are not re-entrant.
 */
#ifndef CUSTOM_ENVS_AMD_H
#define CUSTOM_ENVS_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CE_ABI_VERSION 5

typedef struct ce_engine ce_engine;

typedef enum ce_status {
    CE_OK = 0,
    CE_EINVAL = -1,      /* bad argument or configuration                 */
    CE_EHIP = -2,        /* HIP runtime error                             */
    CE_ENOMEM = -3,      /* allocation failed                             */
    CE_ESTATE = -4,      /* e.g. step before the first reset              */
    CE_EUNSUPPORTED = -5 /* shape has no compiled kernel instance         */
} ce_status;

typedef enum ce_problem {
    /* softmax classifier without bias (the missing ModelNumpy) */
    CE_PROBLEM_SOFTMAX = 0,
    /* F -> hidden... (relu) -> K softmax network, float32 (OptimizeNN,
       custom_envs/problems/optimize_nn.py:22-64, create_neural_net
       utils_tf.py:74-86); flat parameters
       [W1 | b1 | W2 | b2 | ...] in trainable_variables order; CE_F32 only.
       One hidden layer of 64 with B = 32 runs the fused config-3 kernel;
       every other network (1-4 hidden layers, any widths, any B in 1..N,
       K <= 32) the layered path (net_engine.hip) */
    CE_PROBLEM_MLP = 1
} ce_problem;

typedef enum ce_precision {
    CE_F64 = 0, /* float64 state and arithmetic (the reference's numpy dtype) */
    CE_F32 = 1  /* float32 arithmetic, float64 loss recurrence                 */
} ce_precision;

enum {
    CE_PTR_DEVICE = 1u << 0 /* pointers passed to the call are device pointers */
};

typedef struct ce_config {
    int32_t abi_version; /* CE_ABI_VERSION                                  */
    int32_t problem;     /* ce_problem                                      */
    int32_t precision;   /* ce_precision                                    */
    int32_t device;      /* HIP device ordinal                              */
    int32_t num_envs;    /* E: envs owned by this engine (one rank's shard) */
    int32_t n_rows;      /* N: dataset rows                                 */
    int32_t n_features;  /* F                                               */
    int32_t n_classes;   /* K (targets are one-hot, to_onehot semantics)    */
    int32_t batch_size;  /* B rows per minibatch; B == N for batch_size=None */
    int32_t max_steps;   /* episode length, optimize.py:102-103 (40)        */
    int32_t auto_reset;  /* 1: VecEnv auto-reset on done (utils_venv.py:31);
                            0: single gym.Env (baseenvironment.py:30-41)   */
    int32_t n_hidden;    /* CE_PROBLEM_MLP hidden units of a one-layer
                            network (create_neural_net layers,
                            utils_tf.py:74-86); ignored otherwise          */
    int32_t n_layers;    /* CE_PROBLEM_MLP: 0 = one layer of n_hidden;
                            1..4 = that many hidden layers, widths below   */
    int32_t hidden[4];   /* the hidden widths when n_layers > 0            */
} ce_config;

/* Per-step outputs, one row per env.  obs is [E][2P+1] with P the problem's
   parameter count (F*K for the softmax classifier). */
typedef struct ce_outputs {
    float *obs;        /* concat(wght_hist[idx], loss_hist[idx], grad_hist[idx]) */
    float *reward;     /* -loss (minibatch, after the update)                */
    uint8_t *done;     /* current_step >= max_steps                          */
    float *objective;  /* info['objective']: full-dataset loss               */
    float *accuracy;   /* info['accuracy']                                   */
    int32_t *episode_len; /* info['episode']['l'] (current_step of the step) */
} ce_outputs;

/* Host-side copies of the per-env state (any pointer may be NULL). */
typedef struct ce_state {
    double *weights;      /* [E][P]  model.weights                         */
    double *grad_hist;    /* [E][P]  grad_hist[idx] of the last step       */
    double *loss_hist;    /* [E]     loss_hist[idx] of the last step       */
    int32_t *step;        /* [E]     current_step                          */
    double *init_weights; /* [E][P]  W0 every reset restores               */
    int32_t *order;       /* [E][N]  current row order (B < N only)        */
} ce_state;

int ce_abi_version(void);
const char *ce_last_error(void);
/* Sticky HIP errors an entry point found pending when it started (left by
 * another component, e.g. a caller's aborted stream capture) and cleared so
 * that they are not reported as its own failure: how many so far in this
 * process, and a note naming the last one ("" if none). */
int64_t ce_stale_error_count(void);
const char *ce_stale_error_note(void);

int ce_create(const ce_config *cfg, const double *features /* [N][F] */,
              const int32_t *labels /* [N] class index */, ce_engine **out);
void ce_destroy(ce_engine *eng);

int ce_set_stream(ce_engine *eng, void *hip_stream /* NULL: engine's own */);
/* Compact output form for the per-step all-gather (SURVEY 8e, config 4;
 * replaces nothing in the reference, whose VecEnv np.stacks full obs rows,
 * concurrentvecenv.py:99-104).  When on, every CE_PTR_DEVICE call and
 * ce_step_many writes obs as [E][P + 1] = (loss_hist[idx], grad_hist[idx])
 * only -- the wght_hist block of the observation is identically 0
 * (optimize.py:84-86) and is not stored -- and `done` may be NULL
 * (done == episode_len >= max_steps).  Host-mode calls keep the full form.
 * CE_EUNSUPPORTED unless the engine runs the two-class full-batch float64
 * kernel (ce_step_kernel "optimize_lr_mfma_kernel<...>"). */
int ce_set_compact_outputs(ce_engine *eng, int32_t on);
int ce_num_envs(const ce_engine *eng);
int ce_obs_dim(const ce_engine *eng);
int ce_act_dim(const ce_engine *eng);

/* seeds[i] seeds env i exactly as gym.utils.seeding.np_random(seeds[i]). */
int ce_seed(ce_engine *eng, const uint64_t *seeds, int32_t n);
/* Host-only: the (W0, perm) that every reset of a seed draws.  No GPU. */
int ce_seed_draws(uint64_t seed, int32_t n_features, int32_t n_classes,
                  int32_t n_rows, double *init_weights, int32_t *perm);
/* Host-only, CE_PROBLEM_MLP: glorot-uniform W1 then W2 (float32, zero
   biases, flat order) then the row permutation.  No GPU. */
int ce_seed_draws_mlp(uint64_t seed, int32_t n_features, int32_t n_hidden,
                      int32_t n_classes, int32_t n_rows, float *init_weights,
                      int32_t *perm);

int ce_reset(ce_engine *eng, const ce_outputs *out, uint32_t flags);
int ce_step(ce_engine *eng, const float *actions /* [E][P] */,
            const ce_outputs *out, uint32_t flags);
int ce_step_async(ce_engine *eng, const float *actions, const ce_outputs *out,
                  uint32_t flags);
int ce_wait(ce_engine *eng);
int ce_step_many(ce_engine *eng, int32_t k, const float *actions,
                 int64_t action_step_stride /* elements between steps */,
                 const ce_outputs *out /* device pointers */);
int ce_step_many_prepare(ce_engine *eng, int32_t k, const float *actions,
                         int64_t action_step_stride, const ce_outputs *out);
/* K steps whose outputs are kept: step t reads actions + t * action_step_stride
 * and writes every output of `out` (device pointers) advanced by
 * t * out_step_bytes -- a [K] array of output records, e.g. one buffer per
 * field of [K][E] rows (out_step_bytes = that field's E rows) or one packed
 * record per step.  out_step_bytes == 0 overwrites the same outputs every step
 * (ce_step_many).  Where the engine has a persistent kernel (two-class,
 * B == N, float64, n_rows <= 512: ce_step_many_kernel names it) the K steps
 * are ONE launch: the per-env state stays in registers across them and is
 * stored once; otherwise K step launches.  Stream-ordered, asynchronous.
 * obs must be 16-byte aligned and out_step_bytes a multiple of 16, else
 * CE_EINVAL. */
int ce_step_many_strided(ce_engine *eng, int32_t k, const float *actions,
                         int64_t action_step_stride, const ce_outputs *out,
                         int64_t out_step_bytes);
/* on = 1 (default; CE_PERSIST=0 in the environment at ce_create makes it 0):
 * ce_step_many and ce_step_many_strided use the persistent K-step kernel where
 * the engine has one; on = 0: one launch per step (the A/B form).  With the
 * persistent kernel selected, every K-step entry (ce_step_many, _prepare,
 * _strided) refuses an obs that is not 16-byte aligned with CE_EINVAL: the
 * kernel ce_step_many_kernel names is the one that runs, or none. */
int ce_set_persistent(ce_engine *eng, int32_t on);
/* The kernel ce_step_many runs: "optimize_lr_persist_kernel<NKF,TPW,PAD>" when
 * persistent, else ce_step_kernel's name. */
const char *ce_step_many_kernel(const ce_engine *eng);

/* Pinned host buffers holding the last host-mode outputs (zero-copy views). */
int ce_host_outputs(ce_engine *eng, ce_outputs *view);

/* Name of the step kernel the engine launches (introspection for profiles:
 * "optimize_pair_kernel<double,10,2>", "optimize_step_kernel<...>", ...).
 * Static storage, valid for the engine's lifetime; "" for a null engine. */
const char *ce_step_kernel(const ce_engine *eng);

int ce_get_state(ce_engine *eng, const ce_state *st);
int ce_set_state(ce_engine *eng, const ce_state *st);

/* ------------------------------------------------------------------------
 * MultiOptLRs-v0: one agent per problem parameter picks its learning rate.
 * Rows are (env, agent) in sorted agent-name order ('parameter-0',
 * 'parameter-1', 'parameter-10', ...), as OptVecEnv flattens them.
 */
typedef struct ce_multi_engine ce_multi_engine;

#define CE_MULTI_MAX_PARAMS 64

typedef enum ce_function {
    /* sum of Rosenbrock 100(y - x^2)^2 + (1 - x)^2 over coordinate pairs
       (utils_functions.py:4-6); 2 params = the reference's default problem */
    CE_FUNC_ROSENBROCK_PAIRS = 0
} ce_function;

/* info columns, multioptlrs.py:112-127 ('loss' is NaN when not terminal) */
typedef enum ce_multi_info {
    CE_INFO_LOSS = 0, CE_INFO_BATCH_LOSS, CE_INFO_WEIGHTS_MEAN, CE_INFO_WEIGHTS_SUM,
    CE_INFO_ACTIONS_MEAN, CE_INFO_ACTIONS_STD, CE_INFO_STATES_MEAN, CE_INFO_STATES_SUM,
    CE_INFO_GRADS_MEAN, CE_INFO_GRADS_SUM, CE_INFO_LOSS_MEAN, CE_INFO_ADJUSTED_LOSS,
    CE_INFO_ADJUSTED_GRAD, CE_INFO_GRAD_DIFF, CE_MULTI_INFO
} ce_multi_info;

typedef struct ce_multi_config {
    int32_t abi_version;
    int32_t device;
    int32_t num_envs;     /* E                                               */
    int32_t n_params;     /* P: agents per env = problem dimensions (even)   */
    int32_t function;     /* ce_function                                     */
    int32_t max_history;  /* H, adjusted-history length (multioptlrs.py:39)  */
    int32_t max_batches;  /* episode length (multioptlrs.py:39, default 400) */
    int32_t auto_reset;   /* 1: OptVecEnv auto-reset; 0: single env          */
    float initial_points[CE_MULTI_MAX_PARAMS];
} ce_multi_config;

typedef struct ce_multi_outputs {
    float *obs;           /* [E*P][3H] rows                                  */
    float *reward;        /* [E*P] (replicated per agent, optvecenv.py:43)   */
    uint8_t *done;        /* [E*P]                                           */
    float *info;          /* [E][CE_MULTI_INFO]                              */
    int32_t *episode_len; /* [E] info['episode']['l']                        */
} ce_multi_outputs;

int ce_multi_create(const ce_multi_config *cfg, ce_multi_engine **out);
void ce_multi_destroy(ce_multi_engine *eng);
int ce_multi_set_stream(ce_multi_engine *eng, void *hip_stream);
int ce_multi_reset(ce_multi_engine *eng, const ce_multi_outputs *out, uint32_t flags);
int ce_multi_step(ce_multi_engine *eng, const float *actions /* [E*P] rows */,
                  const ce_multi_outputs *out, uint32_t flags);
int ce_multi_step_async(ce_multi_engine *eng, const float *actions,
                        const ce_multi_outputs *out, uint32_t flags);
int ce_multi_wait(ce_multi_engine *eng);
int ce_multi_step_many(ce_multi_engine *eng, int32_t k, const float *actions,
                       int64_t action_step_stride, const ce_multi_outputs *out);
int ce_multi_step_many_prepare(ce_multi_engine *eng, int32_t k, const float *actions,
                               int64_t action_step_stride, const ce_multi_outputs *out);
/* As ce_step_many_strided: step t writes every output advanced by
 * t * out_step_bytes.  With max_history == 5 (the reference default,
 * multioptlrs.py:39) the K steps are ONE launch of multi_persist5_kernel (the
 * state in registers across them); otherwise K step launches. */
int ce_multi_step_many_strided(ce_multi_engine *eng, int32_t k, const float *actions,
                               int64_t action_step_stride, const ce_multi_outputs *out,
                               int64_t out_step_bytes);
/* As ce_set_persistent / ce_step_many_kernel. */
int ce_multi_set_persistent(ce_multi_engine *eng, int32_t on);
const char *ce_multi_step_many_kernel(const ce_multi_engine *eng);
int ce_multi_host_outputs(ce_multi_engine *eng, ce_multi_outputs *view);
/* theta [E][P] (problem parameters in agent order) and current_step [E] */
int ce_multi_get_state(ce_multi_engine *eng, float *theta, int32_t *step);

/* ------------------------------------------------------------------------
 * MultiOptLRs-v0 over OptimizeNN: one agent per network parameter.  The
 * network is F -> hidden[0] -> ... (relu) -> K (softmax), float32, flat
 * parameters in Keras trainable_variables order [W1 | b1 | W2 | b2 | ...].
 * Rows and outputs as for ce_multi_* (ce_multi_outputs).
 */
typedef struct ce_nn_engine ce_nn_engine;

#define CE_NN_MAX_HIDDEN 4

typedef struct ce_nn_config {
    int32_t abi_version;
    int32_t device;
    int32_t num_envs;      /* E                                                 */
    int32_t n_rows;        /* N dataset rows                                    */
    int32_t n_features;    /* F                                                 */
    int32_t n_classes;     /* K (<= 32)                                         */
    int32_t batch_size;    /* B rows per batch (load_data default 32; <= 32)    */
    int32_t n_hidden;      /* hidden layers, 1..CE_NN_MAX_HIDDEN                */
    int32_t hidden[CE_NN_MAX_HIDDEN]; /* units per hidden layer (multiples of 32,
                              <= 512); create_neural_net default (256, 256)    */
    int32_t max_history;   /* H (<= 16)                                         */
    int32_t max_batches;   /* episode length (default 400)                      */
    int32_t auto_reset;    /* 1: OptVecEnv auto-reset; 0: single env            */
} ce_nn_config;

int ce_nn_create(const ce_nn_config *cfg, const float *features /* [N][F] */,
                 const int32_t *labels /* [N] class index */, ce_nn_engine **out);
void ce_nn_destroy(ce_nn_engine *eng);
int ce_nn_set_stream(ce_nn_engine *eng, void *hip_stream);
/* P: parameters (= agents) per env */
int ce_nn_n_params(const ce_nn_engine *eng);
/* seeds[i] seeds env i as gym.utils.seeding.np_random(seeds[i]); must precede
   the first reset */
int ce_nn_seed(ce_nn_engine *eng, const uint64_t *seeds, int32_t n);
/* Host-only: the float32 initial parameters [P], the reset shuffle [N] and
   the epoch-end shuffle [N] of a seed (any output may be NULL).  No GPU. */
int ce_nn_seed_draws(uint64_t seed, int32_t n_dims, const int32_t *dims /* F, hidden..., K */,
                     int32_t n_rows, float *init_weights, int32_t *reset_perm,
                     int32_t *epoch_perm);
int ce_nn_reset(ce_nn_engine *eng, const ce_multi_outputs *out, uint32_t flags);
int ce_nn_step(ce_nn_engine *eng, const float *actions /* [E*P] rows */,
               const ce_multi_outputs *out, uint32_t flags);
int ce_nn_step_async(ce_nn_engine *eng, const float *actions, const ce_multi_outputs *out,
                     uint32_t flags);
int ce_nn_wait(ce_nn_engine *eng);
int ce_nn_step_many(ce_nn_engine *eng, int32_t k, const float *actions,
                    int64_t action_step_stride, const ce_multi_outputs *out);
int ce_nn_step_many_prepare(ce_nn_engine *eng, int32_t k, const float *actions,
                            int64_t action_step_stride, const ce_multi_outputs *out);
int ce_nn_host_outputs(ce_nn_engine *eng, ce_multi_outputs *view);
/* theta [E][P] (agent order), gprev [E][P] (newest raw-history gradient),
   step [E], cursor [E] (batch index in the epoch), order [E][N] (dataset row
   of each current row); any pointer may be NULL */
int ce_nn_get_state(ce_nn_engine *eng, float *theta, float *gprev, int32_t *step,
                    int32_t *cursor, int32_t *order);

/* ------------------------------------------------------------------------
 * The agent's policy on the device: stable-baselines' MlpPolicy as PPO2 / A2C
 * run it (run_multiagent_exp_single.py:37-49; net_arch = [dict(pi=[...],
 * vf=[...])], tanh), one fused launch per forward (policy_kernels.h):
 *   mean    = tanh-MLP_pi(obs) . Wmu + bmu            [A]
 *   value   = tanh-MLP_vf(obs) . Wv + bv              (a separate network of
 *                                                      the same hidden widths)
 *   action  = mean + exp(logstd) * noise              (noise: caller-supplied
 *             N(0,1) block, or NULL: action = mean; the *_rng entries form
 *             it in the kernel from the counter-based generator below)
 *   env_action = min(max(action, low), high)          (what the env step reads;
 *             action stays unclipped, as SB's runner stores it)
 *   neglogp = 0.5 sum noise^2 + sum logstd + 0.5 A log(2 pi)   (from the noise
 *             itself, not from (action - mean) / std; sum noise^2 = 0 for NULL)
 * Limits: 1..3 hidden layers, each width a multiple of 32 up to 128,
 * obs_dim <= 128, act_dim <= 64; anything else is CE_EUNSUPPORTED.  The
 * reference's default 7x7-image Optimize shape (obs_dim 981, act_dim 490) is
 * served on the act side by a wide handle, ce_policy_create_wide below
 * (obs_dim <= 1024, act_dim <= 512); ce_ppo2_create / ce_a2c_create refuse it,
 * ce_ppo2_create_wide / ce_a2c_create_wide train it.
 * Every argument check of every ce_policy_* / ce_*rollout_policy call happens
 * before its first HIP call.
 */
typedef struct ce_policy ce_policy;

typedef struct ce_policy_config {
    int32_t abi_version; /* CE_ABI_VERSION                                   */
    int32_t device;      /* HIP device ordinal                               */
    int32_t obs_dim;     /* D <= 128  (ce_policy_create_wide: <= 1024)       */
    int32_t act_dim;     /* A <= 64   (ce_policy_create_wide: <= 512)        */
    int32_t n_hidden;    /* hidden layers per network, 1..3                  */
    int32_t hidden[4];   /* their widths (multiples of 32, <= 128)           */
} ce_policy_config;

/* Device pointers; all four must be set. */
typedef struct ce_policy_outputs {
    float *action;     /* [rows][A] unclipped sample                        */
    float *env_action; /* [rows][A] clipped to the bounds                   */
    float *neglogp;    /* [rows]                                            */
    float *value;      /* [rows]                                            */
} ce_policy_outputs;

/* Host-only: the length of the flat float32 parameter vector
 *   pi network [W1[D][h1], b1, ..., Wmu[h][A], bmu],
 *   vf network [W1, b1, ..., Wv[h][1], bv], logstd[A]
 * (kernels row-major [in][out]), or a negative ce_status.  No GPU. */
int ce_policy_n_params(const ce_policy_config *cfg);
int ce_policy_create(const ce_policy_config *cfg, ce_policy **out);
/* The wide policy: the same config, parameter vector, semantics and handle
 * type with obs_dim <= 1024 and act_dim <= 512 (hidden layers as above), run
 * by policy_wide_kernel (policy_wide_kernels.h: the first layer in K-chunks
 * of 128 observation columns, the head in N-chunks of 128 actions).  A wide
 * handle always launches that kernel; at a shape ce_policy_create takes too
 * it writes the same bits.  Every entry that takes a ce_policy takes a wide
 * one -- set_params, set_bounds, forward, forward_rng, the rollouts and their
 * _rng / _vecnorm forms -- except the narrow learners: ce_ppo2_create and
 * ce_a2c_create answer CE_EUNSUPPORTED before any allocation (they take
 * obs_dim <= 128, act_dim <= 64); ce_ppo2_create_wide and ce_a2c_create_wide
 * take it. */
int ce_policy_wide_n_params(const ce_policy_config *cfg);
int ce_policy_create_wide(const ce_policy_config *cfg, ce_policy **out);
void ce_policy_destroy(ce_policy *p);
/* n must equal ce_policy_n_params.  Host pointer: synchronises before
 * returning.  CE_PTR_DEVICE: `flat` is a device pointer and the refresh is
 * stream-ordered on hip_stream (one repacking launch, no host round trip);
 * forwards that must see it run on the same stream or after a sync. */
int ce_policy_set_params(ce_policy *p, const float *flat, int64_t n, uint32_t flags,
                         void *hip_stream);
/* Host pointers low[A], high[A] (NULL: unbounded on that side; the default).
 * Synchronous. */
int ce_policy_set_bounds(ce_policy *p, const float *low, const float *high);
/* One stream-ordered launch over `rows` observation rows [rows][D] (device
 * pointers; noise [rows][A] or NULL); any rows >= 1, any engine's obs. */
int ce_policy_forward(const ce_policy *p, const float *obs, const float *noise, int64_t rows,
                      const ce_policy_outputs *out, void *hip_stream);
/* A K-step closed-loop rollout as one call: for t = 0..k-1, on the engine's
 * stream, (1) the policy reads obs0 (t = 0) or env record t-1's obs and
 * writes policy record t (pout advanced by t * pout_step_bytes; noise block
 * t at noise + t * noise_stride elements, noise may be NULL); (2) the env
 * steps with record t's env_action -- the same per-step kernel ce_step_async
 * launches, bit-equal to the unfused sequence -- and writes env record t
 * (out advanced by t * out_step_bytes; obs is the observation after the step,
 * on done the auto-reset observation).  No host work between steps.
 * CE_ESTATE before the first reset; CE_EINVAL with compact outputs on, for a
 * policy whose obs_dim / act_dim are not the engine's (ce_obs_dim /
 * ce_act_dim; 3 * max_history / 1 for the multi engine), for an obs that is
 * not 16-byte aligned or step bytes that are not non-negative multiples of 16. */
int ce_rollout_policy(ce_engine *eng, const ce_policy *p, int32_t k, const float *obs0,
                      const float *noise, int64_t noise_stride, const ce_outputs *out,
                      int64_t out_step_bytes, const ce_policy_outputs *pout,
                      int64_t pout_step_bytes);
int ce_multi_rollout_policy(ce_multi_engine *eng, const ce_policy *p, int32_t k,
                            const float *obs0, const float *noise, int64_t noise_stride,
                            const ce_multi_outputs *out, int64_t out_step_bytes,
                            const ce_policy_outputs *pout, int64_t pout_step_bytes);

/* The counter-based generator (csrc/rng.h; custom_envs_amd/rng.py states it in
 * NumPy): Philox4x32-10 under the key (seed & 0xffffffff, seed >> 32) at the
 * counter (row, t, block, purpose) -- the global row, the draw index, the
 * group of four values inside the row, and a tag (0 policy noise, 1
 * permutation keys, 2 predict, 3 DDPG action noise, 4 replay indices).  Column a of a row's N(0,1) noise is element
 * a % 4 of block a / 4 (Box-Muller on u(x) = ((x >> 8) + 0.5) 2^-24, so
 * |z| <= 5.89).  Each entry below is one plain launch on hip_stream, and every
 * argument is checked before any HIP call.
 *
 * ce_rng_normal: out[s][r][a], s < k, r < rows, a < act_dim (record s at
 * out + s * record_stride_bytes; device pointer) = the policy noise (purpose
 * 0) of global row row0 + r at draw t0 + s.  rows in [1, 2^24], act_dim in
 * [1, 64], t0 + k <= 2^32, row0 + rows <= 2^32.
 * ce_rng_u32: out[i], i < n <= 2^31, = word i % 4 of the block at the counter
 * (0, t, i / 4, purpose). */
int ce_rng_normal(float *out, int32_t k, int64_t rows, int32_t act_dim,
                  int64_t record_stride_bytes, uint64_t seed, uint32_t t0, uint32_t row0,
                  void *hip_stream);
int ce_rng_u32(uint32_t *out, int64_t n, uint64_t seed, uint32_t purpose, uint32_t t,
               void *hip_stream);
/* ce_rng_normal for a wide policy's noise: act_dim in [1, 512]. */
int ce_rng_normal_wide(float *out, int32_t k, int64_t rows, int32_t act_dim,
                       int64_t record_stride_bytes, uint64_t seed, uint32_t t0, uint32_t row0,
                       void *hip_stream);
/* ce_rng_normal under the caller's purpose tag (3: DDPG's action noise). */
int ce_rng_normal_purpose(float *out, int32_t k, int64_t rows, int32_t act_dim,
                          int64_t record_stride_bytes, uint64_t seed, uint32_t purpose, uint32_t t0,
                          uint32_t row0, void *hip_stream);
/* Replay indices (purpose 4): out[s][i], s < steps, i < n (int32, contiguous,
 * device pointer) = (w * size) >> 32 of the word w = ce_rng_u32(seed, 4,
 * t0 + s)[i], an index in [0, size) drawn with replacement; one launch for all
 * steps.  n and size in [1, 2^24], t0 + steps <= 2^32.  Index j is drawn with
 * probability within size / 2^32 (relative) of 1 / size. */
int ce_rng_replay(int32_t *out, int64_t steps, int64_t n, int64_t size, uint64_t seed, uint32_t t0,
                  void *hip_stream);
/* ce_policy_forward / ce_rollout_policy / ce_multi_rollout_policy with the
 * noise formed inside the policy kernel instead of read from a block: row r
 * of the call uses global row row0 + r, and step s of a rollout uses draw
 * t0 + s.  Bit-equal to the block forms fed the output of ce_rng_normal.
 * CE_EINVAL when t0 + k > 2^32 or row0 + rows > 2^32. */
int ce_policy_forward_rng(const ce_policy *p, const float *obs, uint64_t seed, uint32_t t,
                          uint32_t row0, int64_t rows, const ce_policy_outputs *out,
                          void *hip_stream);
int ce_rollout_policy_rng(ce_engine *eng, const ce_policy *p, int32_t k, const float *obs0,
                          uint64_t seed, uint32_t t0, uint32_t row0, const ce_outputs *out,
                          int64_t out_step_bytes, const ce_policy_outputs *pout,
                          int64_t pout_step_bytes);
int ce_multi_rollout_policy_rng(ce_multi_engine *eng, const ce_policy *p, int32_t k,
                                const float *obs0, uint64_t seed, uint32_t t0, uint32_t row0,
                                const ce_multi_outputs *out, int64_t out_step_bytes,
                                const ce_policy_outputs *pout, int64_t pout_step_bytes);

/* ------------------------------------------------------------------------
 * The PPO2 learner on the device (stable-baselines 2.x PPO2 over the policy
 * above; custom_envs_amd/ppo2.py states the semantics in NumPy): GAE, the
 * loss gradient, a global-norm clip, TF-style Adam and the repack of the
 * policy's image (ppo2_kernels.h; the host side both learners share is
 * csrc/learner_host.h).  The learner owns the master flat
 * parameters, Adam's m and v, the step count and the partial slab on the
 * policy's device.  ce_ppo2_gae / _grad / _step are stream-ordered on the
 * caller's stream and never synchronise; results are bit-identical run after
 * run for the same inputs and grid_limit (no floating-point atomics).
 * Every argument check precedes the first HIP call, and the checks of the
 * plain arguments precede the check of the handle.
 */
typedef struct ce_ppo2 ce_ppo2;

typedef struct ce_ppo2_config {
    float gamma;           /* in [0, 1]                                      */
    float lam;             /* in [0, 1]                                      */
    float cliprange;       /* > 0                                            */
    float cliprange_vf;    /* value clip range; negative: no value clipping  */
    float ent_coef;
    float vf_coef;
    float max_grad_norm;   /* global-norm clip; <= 0: none                   */
    float lr;              /* > 0                                            */
    float beta1;           /* in [0, 1)                                      */
    float beta2;           /* in [0, 1)                                      */
    float eps;             /* > 0                                            */
    int32_t normalize_adv; /* normalise advantages over the rows of a call   */
    int32_t grid_limit;    /* workgroups per network; 0: one per CU          */
} ce_ppo2_config;

/* The policy must outlive the learner.  The master parameters start as zeros. */
int ce_ppo2_create(ce_policy *policy, const ce_ppo2_config *cfg, ce_ppo2 **out);
/* The same handle for a policy from ce_policy_create_wide (obs_dim <= 1024,
 * act_dim <= 512, 1..3 hidden layers of 32..128 units): the gradient runs on
 * the chunked kernel of csrc/ppo_grad_wide_tile.h, every other ce_ppo2_* entry
 * takes the handle as it is.  At a shape ce_ppo2_create takes too the gradient
 * (but dlogstd's last place) and statistics are the same bits at the same
 * grid_limit.  A narrow policy handle is CE_EINVAL; grid_limit 0 means 64
 * workgroups per network (at most one per CU).  The config struct is
 * ce_ppo2_create's. */
int ce_ppo2_create_wide(ce_policy *policy, const ce_ppo2_config *cfg, ce_ppo2 **out);
void ce_ppo2_destroy(ce_ppo2 *l);
/* The master parameters (n = ce_policy_n_params; host pointer: synchronises;
 * CE_PTR_DEVICE: stream-ordered).  Both also write through to the policy's
 * image.  Adam's moments and the step count are kept. */
int ce_ppo2_set_params(ce_ppo2 *l, const float *flat, int64_t n, uint32_t flags,
                       void *hip_stream);
int ce_ppo2_get_params(ce_ppo2 *l, float *flat, int64_t n, uint32_t flags, void *hip_stream);
/* The optimiser's state, so that training can be resumed elsewhere: Adam's m
 * and v ([n] float32 each, n = ce_policy_n_params; host pointers: synchronises;
 * CE_PTR_DEVICE: device pointers, stream-ordered) and the count of Adam steps
 * taken (`step` is always a host value).  With the parameters this is all a
 * learner carries from one step to the next. */
int ce_ppo2_get_opt_state(ce_ppo2 *l, float *m, float *v, int64_t n, int64_t *step,
                          uint32_t flags, void *hip_stream);
int ce_ppo2_set_opt_state(ce_ppo2 *l, const float *m, const float *v, int64_t n, int64_t step,
                          uint32_t flags, void *hip_stream);
/* adv, ret [k][rows] contiguous float32 from rewards (float32), dones (uint8)
 * and values (float32) read in place in rollout records: record t of each at
 * base + t * stride bytes (reward / value strides multiples of 4), last_values
 * [rows].  Device pointers. */
int ce_ppo2_gae(const ce_ppo2 *l, int32_t k, int64_t rows, const float *rewards,
                int64_t reward_stride_bytes, const uint8_t *dones, int64_t done_stride_bytes,
                const float *values, int64_t value_stride_bytes, const float *last_values,
                float *adv, float *ret, void *hip_stream);
/* The loss gradient of n rows: rows idx[0..n) (int32, clamped to [0, m)) of
 * the m-row arrays obs [m][D], actions [m][A], advantages, returns,
 * old_neglogp, old_values [m], or rows 0..n-1 when idx is NULL (n <= m).
 * cliprange < 0: the learner's.  Writes grad [n_params] and stats [8]: loss,
 * pg_loss, vf_loss, entropy, approxkl, clipfrac, |grad|^2, 0.  No update. */
int ce_ppo2_grad(ce_ppo2 *l, int64_t n, int64_t m, const int32_t *idx, const float *obs,
                 const float *actions, const float *advantages, const float *returns,
                 const float *old_neglogp, const float *old_values, float cliprange,
                 float *grad, float *stats, void *hip_stream);
/* ce_ppo2_grad, then the clip, Adam and the policy image's repack, one call.
 * lr < 0 / cliprange < 0: the learner's. */
int ce_ppo2_step(ce_ppo2 *l, int64_t n, int64_t m, const int32_t *idx, const float *obs,
                 const float *actions, const float *advantages, const float *returns,
                 const float *old_neglogp, const float *old_values, float lr, float cliprange,
                 float *stats, void *hip_stream);

/* ------------------------------------------------------------------------
 * The A2C learner on the device (stable-baselines 2.x A2C over the policy
 * above; custom_envs_amd/a2c.py states the semantics in NumPy): the n-step
 * returns of discount_with_dones, the loss gradient
 *   loss = mean(adv neglogp) - ent_coef entropy + vf_coef mean((v - ret)^2),
 *   adv = ret - old_value (a constant of the rollout, not normalised),
 * a global-norm clip, TF's RMSProp (epsilon inside the root) and the repack of
 * the policy's image (a2c_kernels.h).  One learner per policy: the learner
 * owns the master flat parameters, RMSProp's ms (starts at ones) and mom
 * (zeros), the partial slab and the returns buffer on the policy's device,
 * and a second learner of either kind on the same policy would overwrite the
 * image from its own master copy.  Every ce_a2c_* call but create / destroy
 * is stream-ordered on the caller's stream and never synchronises (host
 * pointers of _set_params / _get_params aside); results are bit-identical run
 * after run for the same inputs and grid_limit (no floating-point atomics).
 * Every argument check precedes the first HIP call, and the checks of the
 * plain arguments precede the check of the handle.
 * Not here: DDPG, MlpLstmPolicy, explained_variance, a learning-rate
 * scheduler (pass lr per call).  The gradient exchange across GPUs is the
 * last section of this header.
 */
typedef struct ce_a2c ce_a2c;

typedef struct ce_a2c_config {
    float gamma;           /* in [0, 1]                                      */
    float ent_coef;
    float vf_coef;
    float max_grad_norm;   /* global-norm clip; <= 0: none                   */
    float lr;              /* > 0                                            */
    float alpha;           /* RMSProp decay, in [0, 1)                       */
    float eps;             /* > 0, inside the root                           */
    float momentum;        /* in [0, 1)                                      */
    int32_t grid_limit;    /* workgroups per network; 0: one per CU          */
} ce_a2c_config;

/* The policy must outlive the learner.  The master parameters start as zeros. */
int ce_a2c_create(ce_policy *policy, const ce_a2c_config *cfg, ce_a2c **out);
/* As ce_ppo2_create_wide: the A2C learner of a policy from ce_policy_create_wide. */
int ce_a2c_create_wide(ce_policy *policy, const ce_a2c_config *cfg, ce_a2c **out);
void ce_a2c_destroy(ce_a2c *l);
/* As ce_ppo2_set_params / _get_params (one body, csrc/learner_host.h); ms and
 * mom are kept. */
int ce_a2c_set_params(ce_a2c *l, const float *flat, int64_t n, uint32_t flags, void *hip_stream);
int ce_a2c_get_params(ce_a2c *l, float *flat, int64_t n, uint32_t flags, void *hip_stream);
/* The optimiser's state, as ce_ppo2_get_opt_state: RMSProp's mean square ms
 * and its momentum buffer mom ([n] float32 each).  RMSProp keeps no counter:
 * `step` comes back 0 and must be 0 when set. */
int ce_a2c_get_opt_state(ce_a2c *l, float *ms, float *mom, int64_t n, int64_t *step,
                         uint32_t flags, void *hip_stream);
int ce_a2c_set_opt_state(ce_a2c *l, const float *ms, const float *mom, int64_t n, int64_t step,
                         uint32_t flags, void *hip_stream);
/* ret [k][rows] contiguous float32 from rewards (float32) and dones (uint8)
 * read in place in rollout records (record t at base + t * stride bytes; the
 * reward stride a multiple of 4) and last_values [rows]:
 *   carry = last_values; t = k-1 .. 0: carry = r_t + gamma carry (1 - done_t).
 * k * rows <= 2^24.  Device pointers. */
int ce_a2c_returns(const ce_a2c *l, int32_t k, int64_t rows, const float *rewards,
                   int64_t reward_stride_bytes, const uint8_t *dones, int64_t done_stride_bytes,
                   const float *last_values, float *ret, void *hip_stream);
/* The loss gradient of n rows: rows idx[0..n) (int32, clamped to [0, m)) of
 * the flat m-row arrays obs [m][D], actions [m][A], returns, old_values [m],
 * or rows 0..n-1 when idx is NULL (n <= m).  Writes grad [n_params] and
 * stats [8]: loss, pg_loss, vf_loss, entropy, 0, 0, |grad|^2, 0.  No update. */
int ce_a2c_grad(ce_a2c *l, int64_t n, int64_t m, const int32_t *idx, const float *obs,
                const float *actions, const float *returns, const float *old_values, float *grad,
                float *stats, void *hip_stream);
/* ce_a2c_grad, then the clip, RMSProp and the policy image's repack, one
 * call.  lr < 0: the learner's. */
int ce_a2c_step(ce_a2c *l, int64_t n, int64_t m, const int32_t *idx, const float *obs,
                const float *actions, const float *returns, const float *old_values, float lr,
                float *stats, void *hip_stream);
/* The whole update of a k-step rollout of `rows` rows on its records in
 * place: obs [k][rows][D] contiguous; actions / values / rewards / dones in
 * their strided records (record t at base + t * stride bytes; every stride at
 * least one record long, the float32 ones multiples of 4).  Enqueues six
 * launches -- the returns scan into a learner-owned buffer (allocated when k *
 * rows first exceeds it), the gradient over all k * rows rows, reduce, finish,
 * RMSProp, repack -- with no copy and, in the steady state, no allocation. */
int ce_a2c_update(ce_a2c *l, int32_t k, int64_t rows, const float *obs, const float *actions,
                  int64_t action_stride_bytes, const float *values, int64_t value_stride_bytes,
                  const float *rewards, int64_t reward_stride_bytes, const uint8_t *dones,
                  int64_t done_stride_bytes, const float *last_values, float lr, float *stats,
                  void *hip_stream);

/* ------------------------------------------------------------------------
 * Data-parallel learners: the gradient exchange across GPUs.  W ranks, rank r
 * holding n_r rows, take the single learner's step on all n_total = sum n_r
 * rows (the mean is 1 / n_total; PPO2 normalises advantages over all of them).
 * A _partial call ends with this rank's record ready to gather; an _apply call
 * starts from the W gathered records.  The collective in between is the
 * caller's (custom_envs_amd/distributed.py: GradientExchange).
 *
 * A record is ce_learner_record_bytes(policy) bytes of float64, a multiple of
 * 256: [n_params sums over this rank's rows, in flat parameter order, before
 * any rounding and without the entropy term | 8 statistic sums | n_r].
 * `records` is [world][record], rank r's record in slot r.  Every rank adds
 * the records in rank order in float64, so every rank computes the same bits,
 * and at world 1 _partial + _apply leave the bits of _step.  Records and
 * moments are device pointers, 8-byte aligned.  Stream-ordered, no
 * synchronisation, no allocation (ce_a2c_update_partial's returns buffer
 * aside, as ce_a2c_update's).
 */
int64_t ce_learner_record_bytes(const ce_policy *policy);   /* -1: null policy */
/* out3 = (n, mean, sum (a - mean)^2) of the n gathered advantages, float64. */
int ce_ppo2_adv_moments(const ce_ppo2 *l, int64_t n, int64_t m, const int32_t *idx,
                        const float *advantages, double *out3, void *hip_stream);
/* ce_ppo2_grad's rows with the row weight 1 / n_total (n_total >= n), into
 * `record`.  moments: [world][3], every rank's ce_ppo2_adv_moments triple,
 * merged in rank order (Chan) into the normalisation; NULL only when the
 * learner does not normalise advantages. */
int ce_ppo2_partial(ce_ppo2 *l, int64_t n, int64_t n_total, int64_t m, const int32_t *idx,
                    const float *obs, const float *actions, const float *advantages,
                    const float *returns, const float *old_neglogp, const float *old_values,
                    float cliprange, int32_t world, const double *moments, double *record,
                    void *hip_stream);
/* grad [n_params] and stats [8] of all n_total rows from the records; no update. */
int ce_ppo2_combine(ce_ppo2 *l, int32_t world, const double *records, int64_t n_total,
                    float *grad, float *stats, void *hip_stream);
/* ce_ppo2_combine, then the clip, Adam (one step) and the repack. */
int ce_ppo2_apply(ce_ppo2 *l, int32_t world, const double *records, int64_t n_total, float lr,
                  float *stats, void *hip_stream);
/* ce_a2c_grad's rows with the row weight 1 / n_total, into `record`. */
int ce_a2c_partial(ce_a2c *l, int64_t n, int64_t n_total, int64_t m, const int32_t *idx,
                   const float *obs, const float *actions, const float *returns,
                   const float *old_values, double *record, void *hip_stream);
/* ce_a2c_update's returns scan and gradient on the rollout records in place,
 * with the row weight 1 / n_total (n_total >= k * rows), into `record`. */
int ce_a2c_update_partial(ce_a2c *l, int32_t k, int64_t rows, int64_t n_total, const float *obs,
                          const float *actions, int64_t action_stride_bytes, const float *values,
                          int64_t value_stride_bytes, const float *rewards,
                          int64_t reward_stride_bytes, const uint8_t *dones,
                          int64_t done_stride_bytes, const float *last_values, double *record,
                          void *hip_stream);
int ce_a2c_combine(ce_a2c *l, int32_t world, const double *records, int64_t n_total, float *grad,
                   float *stats, void *hip_stream);
/* ce_a2c_combine, then the clip, RMSProp and the repack. */
int ce_a2c_apply(ce_a2c *l, int32_t world, const double *records, int64_t n_total, float lr,
                 float *stats, void *hip_stream);

/* ------------------------------------------------------------------------
 * The DDPG learner on the device (custom_envs_amd/ddpg.py states the
 * semantics in NumPy): stable-baselines 2.x DDPG over ddpg.MlpPolicy at its
 * defaults.  With o = min(max(obs, obs_lo), obs_hi):
 *   actor   a = tanh(relu-MLP(o) . W_out + b_out)              in [-1, 1]^A
 *   critic  h = relu(o W_0 + b_0); h = concat(h, action); further relu layers;
 *           Q = h . W_out + b_out
 *   y       = reward + gamma (1 - done1) critic'(obs1, actor'(obs1))   (targets)
 *   critic_loss = mean((critic(obs0, action) - y)^2)    -> d / d critic
 *   actor_loss  = -mean(critic(obs0, actor(obs0)))      -> d / d actor only
 *   Adam (eps outside the root, no clip) on each block with its own lr and a
 *   shared step count, then target = (1 - tau) target + tau params.
 * The flat float32 vector is [actor | critic]:
 *   actor  [W0[D][h0], b0, ..., W_out[h_last][A], b_out],
 *   critic [W0[D][h0], b0, W1[h0 + A][h1], b1, ..., W_out[.][1], b_out]
 * (row-major [in][out]; the + A rows sit on the layer after the first hidden
 * one, W_out with a single hidden layer).  The targets use the same layout.
 * Limits: 1..2 hidden layers, each 32 or 64 wide, obs_dim <= 128, act_dim <=
 * 64; anything else is CE_EUNSUPPORTED.  Every argument check precedes the
 * first HIP call; calls are stream-ordered on hip_stream, no synchronisation
 * (host-pointer parameter copies aside) and no allocation.
 */
typedef struct ce_ddpg ce_ddpg;

typedef struct ce_ddpg_config {
    int32_t abi_version; /* CE_ABI_VERSION                                   */
    int32_t device;      /* HIP device ordinal                               */
    int32_t obs_dim;     /* D <= 128                                         */
    int32_t act_dim;     /* A <= 64                                          */
    int32_t n_hidden;    /* hidden layers per network, 1..2                  */
    int32_t hidden[4];   /* their widths (32 or 64)                          */
    int32_t grid_limit;  /* workgroups per branch of the gradient; 0: CUs    */
    double gamma;        /* discount                                         */
    double tau;          /* soft-update rate                                 */
    double actor_lr;     /* Adam step size of the actor's block              */
    double critic_lr;    /* Adam step size of the critic's block             */
    double beta1;
    double beta2;
    double eps;
    double obs_lo;       /* observation_range                                */
    double obs_hi;
    float scale[64];     /* env_action = action * scale, [A]                 */
} ce_ddpg_config;

#define CE_DDPG_TARGET 2u /* ce_ddpg_{set,get}_params: the target networks  */

/* Host-only: the length of the flat parameter vector, or a negative
 * ce_status.  No GPU. */
int ce_ddpg_n_params(const ce_ddpg_config *cfg);
int ce_ddpg_create(const ce_ddpg_config *cfg, ce_ddpg **out);
void ce_ddpg_destroy(ce_ddpg *l);
/* The online parameters, copied into the targets too (SB's initialisation);
 * Adam's moments and step count are kept.  Flags as ce_policy_set_params;
 * with CE_DDPG_TARGET the targets alone (a saved model's, after the online
 * ones). */
int ce_ddpg_set_params(ce_ddpg *l, const float *flat, int64_t n, uint32_t flags, void *hip_stream);
/* flags: CE_PTR_DEVICE | CE_DDPG_TARGET. */
int ce_ddpg_get_params(ce_ddpg *l, float *flat, int64_t n, uint32_t flags, void *hip_stream);
/* One launch over obs [rows][D] (noise [rows][A] or NULL): action = a, or
 * min(max(a + noise, -1), 1); env_action = action * scale.  Device pointers. */
int ce_ddpg_act(const ce_ddpg *l, const float *obs, const float *noise, int64_t rows,
                float *action, float *env_action, void *hip_stream);
/* y [n] of the rows idx[0..n) (NULL: the first n) of an m-row batch. */
int ce_ddpg_target(ce_ddpg *l, int64_t n, int64_t m, const int32_t *idx, const float *obs1,
                   const float *rewards, const uint8_t *dones, float *y, void *hip_stream);
/* grad [n_params] and stats [8] = critic_loss, actor_loss, mean Q, mean y, 0, 0,
 * |critic grad|^2, |actor grad|^2; no update.  Four launches.  y [n]: the
 * caller's device buffer the targets of these rows are left in. */
int ce_ddpg_grad(ce_ddpg *l, int64_t n, int64_t m, const int32_t *idx, const float *obs0,
                 const float *actions, const float *rewards, const float *obs1,
                 const uint8_t *dones, float *y, float *grad, float *stats, void *hip_stream);
/* ce_ddpg_grad, then Adam on both blocks, the soft update and the images'
 * repack as one more launch: five.  actor_lr / critic_lr below zero: the
 * config's; zero: that block's parameters stay where they are. */
int ce_ddpg_step(ce_ddpg *l, int64_t n, int64_t m, const int32_t *idx, const float *obs0,
                 const float *actions, const float *rewards, const float *obs1,
                 const uint8_t *dones, float *y, double actor_lr, double critic_lr,
                 float *stats, void *hip_stream);

/* The action noise ce_ddpg_act_rng forms from the generator (purpose 3):
 * z = the N(0,1) value of (global row row0 + r, draw t, column c), then per
 * column c, in float32 with every operation rounded on its own,
 *   CE_DDPG_NOISE_NORMAL  n  = mean + sigma * z
 *   CE_DDPG_NOISE_OU      x' = (x + (theta * (mean - x)) * dt) + s * z,  n = x',
 *                         s = float32(sigma * sqrt(dt)) formed in double
 * (stable-baselines' NormalActionNoise / OrnsteinUhlenbeckActionNoise). */
#define CE_DDPG_NOISE_NORMAL 0
#define CE_DDPG_NOISE_OU 1
typedef struct ce_ddpg_noise {
    int32_t kind;        /* CE_DDPG_NOISE_*                                  */
    double theta;        /* OU: the pull towards the mean                    */
    double dt;           /* OU: > 0                                          */
    float mean[64];      /* [A]                                              */
    float sigma[64];     /* [A], >= 0                                        */
} ce_ddpg_noise;
/* ce_ddpg_act with the noise formed inside the kernel: action = min(max(a + n,
 * -1), 1).  OU reads and writes ou_state [rows][A] (float32, device; the
 * caller zeroes it to start) and reads x as 0 at the rows where reset [rows]
 * (uint8, device, or NULL) is non-zero: the previous step's dones.  Bit-equal
 * to ce_ddpg_act fed the same n.  CE_EINVAL: OU without ou_state, row0 + rows
 * > 2^32.  One launch, no allocation, no synchronisation. */
int ce_ddpg_act_rng(const ce_ddpg *l, const float *obs, int64_t rows, uint64_t seed, uint32_t t,
                    uint32_t row0, const ce_ddpg_noise *noise, float *ou_state,
                    const uint8_t *reset, float *action, float *env_action, void *hip_stream);
/* `steps` train steps in one call: ONE launch draws idx_scratch [steps][n]
 * (ce_rng_replay at draws t0 .. t0 + steps - 1 over [0, size)), then step s is
 * ce_ddpg_step over rows idx_scratch[s] of the size-row batch with stats
 * [steps][8] row s; y [n] is reused by every step.  Bit-equal to the same
 * ce_ddpg_step calls issued one by one.  Adam's count advances by steps. */
int ce_ddpg_train(ce_ddpg *l, int32_t steps, int64_t n, int64_t size, uint64_t seed, uint32_t t0,
                  const float *obs0, const float *actions, const float *rewards,
                  const float *obs1, const uint8_t *dones, int32_t *idx_scratch, float *y,
                  double actor_lr, double critic_lr, float *stats, void *hip_stream);
/* Adam's m and v ([n] float32 each, n = ce_ddpg_n_params, the flat layout) and
 * the shared step count, as ce_ppo2_get_opt_state / ce_ppo2_set_opt_state:
 * host pointers synchronise, CE_PTR_DEVICE is stream-ordered. */
int ce_ddpg_get_opt_state(ce_ddpg *l, float *m, float *v, int64_t n, int64_t *step,
                          uint32_t flags, void *hip_stream);
int ce_ddpg_set_opt_state(ce_ddpg *l, const float *m, const float *v, int64_t n, int64_t step,
                          uint32_t flags, void *hip_stream);

/* DDPG's side of the gradient exchange (as ce_ppo2_partial / _combine /
 * _apply above): W ranks, rank r holding n_r sampled rows, take the single
 * agent's train step on the concatenation, N = sum n_r.  A record is
 * ce_ddpg_record_bytes(l) bytes of float64, a multiple of 256:
 *   [n_params sums over this rank's rows in flat parameter order, before any
 *    rounding | 8 statistic sums | n_r | zeros].
 * `records` is [world][record], rank r's record in slot r; every rank adds
 * them in rank order in float64 and rounds once, so every rank computes the
 * same bits, and at world 1 _partial + _apply leave the bits of ce_ddpg_step.
 * Device pointers, 8-byte aligned; stream-ordered, no synchronisation, no
 * allocation. */
int64_t ce_ddpg_record_bytes(const ce_ddpg *l);              /* -1: null learner */
/* ce_ddpg_grad's target and gradient of these n rows with the row weight 1 /
 * n_total (n <= n_total <= 2^30), into `record`.  Three launches. */
int ce_ddpg_partial(ce_ddpg *l, int64_t n, int64_t n_total, int64_t m, const int32_t *idx,
                    const float *obs0, const float *actions, const float *rewards,
                    const float *obs1, const uint8_t *dones, float *y, double *record,
                    void *hip_stream);
/* grad [n_params] and stats [8] of all n_total rows from the records; no update. */
int ce_ddpg_combine(ce_ddpg *l, int32_t world, const double *records, int64_t n_total,
                    float *grad, float *stats, void *hip_stream);
/* ce_ddpg_combine into the agent's gradient, then ce_ddpg_step's update (Adam
 * on both blocks, one step; the soft update; both images). */
int ce_ddpg_apply(ce_ddpg *l, int32_t world, const double *records, int64_t n_total,
                  double actor_lr, double critic_lr, float *stats, void *hip_stream);

/* The wide DDPG agent: the same learner at obs_dim <= 1024, act_dim <= 512
 * (1..2 hidden layers of 32 or 64 units), on tile kernels that walk the wide
 * layers in chunks (csrc/ddpg_wide_kernels.h); the reference's Optimize-v0
 * spec is 981 -> 490.  ce_ddpg_create_wide returns a ce_ddpg marked wide, and
 * every other ce_ddpg_* entry takes it as it is; ce_ddpg_act_rng reads 64
 * columns of noise, so a handle with act_dim > 64 takes its generated noise
 * through ce_ddpg_act_rng_wide (which serves any handle).  grid_limit 0: at
 * most 64 workgroups per branch.  CE_EUNSUPPORTED past the limits, before any
 * HIP call.  ce_ddpg_create keeps its own limits (128, 64). */
#define CE_DDPG_WIDE_MAX_OBS 1024
#define CE_DDPG_WIDE_MAX_ACT 512
typedef struct ce_ddpg_wide_config {
    int32_t abi_version; /* CE_ABI_VERSION                                   */
    int32_t device;      /* HIP device ordinal                               */
    int32_t obs_dim;     /* D <= 1024                                        */
    int32_t act_dim;     /* A <= 512                                         */
    int32_t n_hidden;    /* hidden layers per network, 1..2                  */
    int32_t hidden[4];   /* their widths (32 or 64)                          */
    int32_t grid_limit;  /* workgroups per branch of the gradient; 0: <= 64  */
    double gamma;
    double tau;
    double actor_lr;
    double critic_lr;
    double beta1;
    double beta2;
    double eps;
    double obs_lo;
    double obs_hi;
    float scale[CE_DDPG_WIDE_MAX_ACT]; /* env_action = action * scale, [A]   */
} ce_ddpg_wide_config;
typedef struct ce_ddpg_wide_noise {
    int32_t kind;        /* CE_DDPG_NOISE_*                                  */
    double theta;
    double dt;
    float mean[CE_DDPG_WIDE_MAX_ACT];  /* [A]                                */
    float sigma[CE_DDPG_WIDE_MAX_ACT]; /* [A], >= 0                          */
} ce_ddpg_wide_noise;
/* Host-only, as ce_ddpg_n_params. */
int ce_ddpg_n_params_wide(const ce_ddpg_wide_config *cfg);
int ce_ddpg_create_wide(const ce_ddpg_wide_config *cfg, ce_ddpg **out);
/* ce_ddpg_act_rng with up to 512 columns of noise.  The columns' mean and
 * sigma are kept in the handle's device memory: a call whose values differ
 * from the previous call's uploads them and synchronises the stream once. */
int ce_ddpg_act_rng_wide(ce_ddpg *l, const float *obs, int64_t rows, uint64_t seed, uint32_t t,
                         uint32_t row0, const ce_ddpg_wide_noise *noise, float *ou_state,
                         const uint8_t *reset, float *action, float *env_action, void *hip_stream);

/* The episode monitor on the device: utils_logging.VecMonitor's bookkeeping
 * (custom_envs/utils/utils_logging.py:98-116 per env) over K-step rollout
 * records where the rollout left them.  The carry -- per env ep_reward
 * (float64), ep_len (int32), episode (int64), total_steps (int64) -- lives on
 * the device between calls.  Records are read in place: an env's reward and
 * done at step t are row num_envs-index * row_stride of record t (base + t *
 * stride bytes), so a multi-agent env is seen through its first agent row. */
typedef struct ce_monitor ce_monitor;
#define CE_MONITOR_MAX_INFO 16
/* One info column: element (t, env) is
 * ((const float *)((const char *)base + t * stride_bytes))[env * row_floats + col]. */
typedef struct ce_monitor_column {
    const void *base;      /* device, 4-byte aligned                          */
    int64_t stride_bytes;  /* multiple of 4, >= num_envs * row_floats * 4     */
    int32_t row_floats;    /* floats per env in one record, >= 1              */
    int32_t col;           /* in [0, row_floats)                              */
} ce_monitor_column;
/* Bytes of one episode record with n_info columns (-1: n_info out of range):
 *   {int32 env, int32 t, float64 r, int32 l, float32 current_reward,
 *    int64 episode, float32 info[n_info]}  padded to a multiple of 8
 * r is the float64 sum of the episode's float32 rewards in step order (the
 * bits of VecMonitor's np.float64 sum), unrounded. */
int64_t ce_monitor_record_bytes(int32_t n_info);
/* A monitor of num_envs envs on `device`, the carry zeroed. */
int ce_monitor_create(int32_t device, int32_t num_envs, ce_monitor **out);
void ce_monitor_destroy(ce_monitor *m);
/* VecMonitor.reset: ep_reward and ep_len cleared and episode advanced by one,
 * of every env (indices NULL) or of the n envs listed in the host array
 * indices (duplicates count once).  CE_EINVAL: an index outside the envs. */
int ce_monitor_reset(ce_monitor *m, const int32_t *indices, int32_t n, void *hip_stream);
/* K steps of VecMonitor.step as four launches, stream-ordered, no host read:
 * the forward scan per env (ep_reward += (double)reward, ep_len += 1; at a done
 * (r, l, current_reward, episode) is staged at [t][env], the sums are cleared
 * and episode advanced), the finished episodes' count per 256 flags of the
 * flattened [k][num_envs] dones, the one-workgroup scan of the counts, and the
 * write of one record per finished episode into out [capacity] in (t, env)
 * order.  The count of finished episodes goes to total[0] (device, 8-byte
 * aligned) whatever the capacity; nothing is written at or past out +
 * capacity * ce_monitor_record_bytes(n_info).  The rollout records and
 * `columns`' targets must stay as they are until the last ce_monitor_write of
 * this scan.  Allocates only when k * num_envs exceeds every earlier call's. */
int ce_monitor_scan(ce_monitor *m, int32_t k, int32_t num_envs, int32_t row_stride,
                    const float *rewards, int64_t reward_stride_bytes, const uint8_t *dones,
                    int64_t done_stride_bytes, const ce_monitor_column *columns, int32_t n_info,
                    void *out, int64_t capacity, int64_t *total, void *hip_stream);
/* The last scan's records again, into another (larger) buffer: the write
 * launch only, the carry is untouched.  CE_ESTATE before the first scan. */
int ce_monitor_write(ce_monitor *m, void *out, int64_t capacity, void *hip_stream);
/* The carry to / from host arrays of num_envs entries each; synchronises. */
int ce_monitor_get_state(ce_monitor *m, double *ep_reward, int32_t *ep_len, int64_t *episode,
                         int64_t *total_steps, void *hip_stream);
int ce_monitor_set_state(ce_monitor *m, const double *ep_reward, const int32_t *ep_len,
                         const int64_t *episode, const int64_t *total_steps, void *hip_stream);
/* stable-baselines' explained_variance of a rollout: 1 - Var[returns - values]
 * / Var[returns] over k * rows entries (population variances; NaN when
 * Var[returns] == 0) into out[0] (float64, device).  values is read strided in
 * the policy records, returns is the learner's flat [k * rows] array.  Two
 * passes in float64 in a fixed order by one workgroup: the same inputs give the
 * same bits.  One launch on the current device, no synchronisation. */
int ce_explained_variance(int32_t k, int64_t rows, const float *values, int64_t value_stride_bytes,
                          const float *returns, double *out, void *hip_stream);

/* stable-baselines' VecNormalize on the device (custom_envs_amd/vectorize/
 * vecnormalize.py states it in NumPy as vecnormalize_numpy).  The state -- the
 * float64 running mean, variance and count of every observation column and of
 * the discounted returns, and the per-row return `ret` -- lives on the device
 * between calls.  One step is ONE launch (csrc/vecnorm_kernels.h): the moments
 * are merged with the batch first, then obs and reward are scaled with the
 * updated moments, clipped and stored as float32.  Every sum runs in a fixed
 * order without atomics: the same inputs give the same bits.  Rows are the
 * engine's rows (envs x agents); the moments run per column over all rows. */
typedef struct ce_vecnorm ce_vecnorm;

typedef struct ce_vecnorm_config {
    int32_t abi_version; /* CE_ABI_VERSION                                   */
    int32_t device;      /* HIP device ordinal                               */
    int64_t rows;        /* in [1, 2^24]                                     */
    int32_t obs_dim;     /* in [1, 2^16]                                     */
    int32_t norm_obs;    /* 0: obs_out is obs unchanged                      */
    int32_t norm_reward; /* 0: reward_out is reward unchanged                */
    int32_t reserved;    /* 0                                                */
    double clip_obs;     /* > 0 (SB: 10)                                     */
    double clip_reward;  /* > 0 (SB: 10)                                     */
    double gamma;        /* finite (SB: 0.99)                                */
    double epsilon;      /* >= 0 (SB: 1e-8)                                  */
} ce_vecnorm_config;

enum ce_vecnorm_flags {
    CE_VECNORM_TRAINING = 1u << 0, /* merge this batch into the moments      */
    CE_VECNORM_RESET = 1u << 1,    /* VecNormalize.reset: ret = 0, the obs moments
                                      updated, no reward; reward, done and
                                      reward_out may be NULL                 */
    CE_VECNORM_OBS_ONLY = 1u << 2  /* obs_out only, with the moments as they are:
                                      nothing of the state changes (not with
                                      TRAINING or RESET); reward, done and
                                      reward_out may be NULL                 */
};

/* The state starts at mean 0, variance 1, count 1e-4, ret 0.  The checks of
 * cfg precede the first HIP call. */
int ce_vecnorm_create(const ce_vecnorm_config *cfg, ce_vecnorm **out);
void ce_vecnorm_destroy(ce_vecnorm *vn);
/* One stream-ordered launch (device pointers; obs and obs_out [rows][obs_dim]
 * float32, reward and reward_out [rows] float32, done [rows] bytes):
 *   if TRAINING and norm_obs:    obs moments = update(obs moments, obs)
 *   obs_out = clip((obs - mean) / sqrt(var + epsilon), +-clip_obs)
 *   ret = ret * gamma + reward
 *   if TRAINING and norm_reward: ret moments = update(ret moments, ret)
 *   reward_out = clip(reward / sqrt(ret var + epsilon), +-clip_reward)
 *   ret[done] = 0
 * The quotients are formed as products with 1 / sqrt(.), one rounding away
 * from the statement's in float64.  The checks of the pointers and flags
 * precede the check of the handle; all precede the first HIP call. */
int ce_vecnorm_step(ce_vecnorm *vn, const float *obs, const float *reward, const uint8_t *done,
                    float *obs_out, float *reward_out, uint32_t flags, void *hip_stream);
/* The state to / from host arrays: obs_mean, obs_var [obs_dim], ret [rows],
 * the others one double each; synchronises. */
int ce_vecnorm_get_state(ce_vecnorm *vn, double *obs_mean, double *obs_var, double *obs_count,
                         double *ret_mean, double *ret_var, double *ret_count, double *ret,
                         void *hip_stream);
int ce_vecnorm_set_state(ce_vecnorm *vn, const double *obs_mean, const double *obs_var,
                         const double *obs_count, const double *ret_mean, const double *ret_var,
                         const double *ret_count, const double *ret, void *hip_stream);

/* Where a rollout's N(0,1) noise comes from. */
enum ce_noise_kind {
    CE_NOISE_BLOCK = 0,    /* ptr [k][rows][A], `stride` elements apart; NULL:
                              the deterministic policy                       */
    CE_NOISE_GENERATED = 1 /* formed in the policy kernel: seed, draw t0 + s,
                              global rows row0 ..                            */
};
typedef struct ce_rollout_noise {
    int32_t kind;     /* ce_noise_kind                                       */
    int32_t reserved; /* 0                                                   */
    const float *ptr;
    int64_t stride;
    uint64_t seed;
    uint32_t t0, row0;
} ce_rollout_noise;

/* ce_rollout_policy / ce_multi_rollout_policy with a third launch per step:
 * for s = 0..k-1, on the engine's stream, (1) the policy reads normalised slot
 * s of obs_norm ([k + 1] slots of [rows][D], obs_norm_step_bytes apart; slot 0
 * is the caller's, already normalised) and writes policy record s; (2) the env
 * steps into raw record s of `out`; (3) the normaliser (ce_vecnorm_step with
 * vn_flags, TRAINING or 0) reads that record's obs, reward and done and writes
 * normalised slot s + 1 and normalised reward record s ([k] records of [rows],
 * reward_norm_step_bytes apart).  The raw records stay intact.  Bit-equal to
 * the same three calls issued one by one.  Checks, in this order and all before
 * the first HIP call: null pointers (the engine's first); k, the noise kind,
 * vn_flags, alignment (obs_norm and both step bytes multiples of 16); then what
 * ce_rollout_policy checks; then the normaliser's rows and obs_dim against the
 * engine's and the step bytes against rows * D * 4 and rows * 4. */
int ce_rollout_policy_vecnorm(ce_engine *eng, const ce_policy *p, ce_vecnorm *vn, int32_t k,
                              float *obs_norm, int64_t obs_norm_step_bytes, float *reward_norm,
                              int64_t reward_norm_step_bytes, uint32_t vn_flags,
                              const ce_rollout_noise *noise, const ce_outputs *out,
                              int64_t out_step_bytes, const ce_policy_outputs *pout,
                              int64_t pout_step_bytes);
int ce_multi_rollout_policy_vecnorm(ce_multi_engine *eng, const ce_policy *p, ce_vecnorm *vn,
                                    int32_t k, float *obs_norm, int64_t obs_norm_step_bytes,
                                    float *reward_norm, int64_t reward_norm_step_bytes,
                                    uint32_t vn_flags, const ce_rollout_noise *noise,
                                    const ce_multi_outputs *out, int64_t out_step_bytes,
                                    const ce_policy_outputs *pout, int64_t pout_step_bytes);

#ifdef __cplusplus
}
#endif

#endif /* CUSTOM_ENVS_AMD_H */
