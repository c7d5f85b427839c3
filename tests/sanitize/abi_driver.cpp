// Host-code sanitizer driver (ASan + UBSan, CPU only; no GPU call succeeds
// here): every host-only C-ABI entry point with realistic and edge shapes,
// every entry point's argument validation with bad arguments, and ce_create's
// plan with the host-side dataset image builders (the library's test hooks).  The
// draws are printed (one line per array, hex float bits / ints) so the
// pytest wrapper (tests/test_sanitize.py) compares them with the numpy
// oracle; any sanitizer report aborts the process with a non-zero status.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "custom_envs_amd.h"

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::fprintf(stderr, "EXPECT failed: %s (line %d)\n", #cond, __LINE__); \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

template <typename T> static void dump(const char *tag, const std::vector<T> &v) {
    std::printf("%s", tag);
    for (const T &x : v) {
        uint64_t bits = 0;
        std::memcpy(&bits, &x, sizeof(T));
        std::printf(" %llx", static_cast<unsigned long long>(bits));
    }
    std::printf("\n");
}

// The argument checks of ce_ppo2_* and ce_a2c_* with a NULL handle: one defect
// per call (the lists of tests/test_ppo2_host.py and tests/test_a2c_host.py),
// each refused with a message that names it, and the all-valid call refused
// for the handle alone, last.
#define REFUSED(call, word)                                                   \
    EXPECT((call) == CE_EINVAL && std::strstr(ce_last_error(), word) != nullptr)

static void learner_checks() {
    std::vector<float> buf(64, 0.0f);
    float *a = buf.data();
    const uint8_t *d = reinterpret_cast<const uint8_t *>(a);
    const int32_t *ix = reinterpret_cast<const int32_t *>(a);
    const float *odd = reinterpret_cast<const float *>(reinterpret_cast<const char *>(a) + 2);
    const int64_t big = int64_t(1) << 24;

    // ---- create / destroy / parameters
    ce_ppo2_config pc{0.99f, 0.95f, 0.2f, 0.2f, 0.01f, 0.5f, 0.5f, 2.5e-4f, 0.9f, 0.999f, 1e-5f, 1, 0};
    ce_ppo2 *pl = nullptr;
    REFUSED(ce_ppo2_create(nullptr, &pc, &pl), "null policy");
    REFUSED(ce_ppo2_create(nullptr, nullptr, &pl), "null config");
    REFUSED(ce_ppo2_create(nullptr, &pc, nullptr), "null output");
    ce_ppo2_config pbad = pc;
    pbad.gamma = 1.5f;
    REFUSED(ce_ppo2_create(nullptr, &pbad, &pl), "gamma");
    pbad = pc;
    pbad.beta1 = 1.0f;
    REFUSED(ce_ppo2_create(nullptr, &pbad, &pl), "beta1");
    pbad = pc;
    pbad.grid_limit = -1;
    REFUSED(ce_ppo2_create(nullptr, &pbad, &pl), "grid_limit");
    EXPECT(pl == nullptr);
    ce_ppo2_destroy(nullptr);
    ce_a2c_config ac{0.99f, 0.01f, 0.25f, 0.5f, 7e-4f, 0.99f, 1e-5f, 0.0f, 0};
    ce_a2c *al = nullptr;
    REFUSED(ce_a2c_create(nullptr, &ac, &al), "null policy");
    REFUSED(ce_a2c_create(nullptr, nullptr, &al), "null config");
    REFUSED(ce_a2c_create(nullptr, &ac, nullptr), "null output");
    ce_a2c_config abad = ac;
    abad.alpha = 1.0f;
    REFUSED(ce_a2c_create(nullptr, &abad, &al), "alpha");
    abad = ac;
    abad.momentum = -0.5f;
    REFUSED(ce_a2c_create(nullptr, &abad, &al), "momentum");
    EXPECT(al == nullptr);
    ce_a2c_destroy(nullptr);
    REFUSED(ce_ppo2_set_params(nullptr, nullptr, 8, 0, nullptr), "null parameter vector");
    REFUSED(ce_ppo2_set_params(nullptr, a, 8, 0, nullptr), "null learner");
    REFUSED(ce_ppo2_get_params(nullptr, nullptr, 8, 0, nullptr), "null parameter vector");
    REFUSED(ce_ppo2_get_params(nullptr, a, 8, 0, nullptr), "null learner");
    REFUSED(ce_a2c_set_params(nullptr, nullptr, 8, 0, nullptr), "null parameter vector");
    REFUSED(ce_a2c_set_params(nullptr, a, 8, 0, nullptr), "null learner");
    REFUSED(ce_a2c_get_params(nullptr, nullptr, 8, 0, nullptr), "null parameter vector");
    REFUSED(ce_a2c_get_params(nullptr, a, 8, 0, nullptr), "null learner");

    // ---- ce_ppo2_gae(l, k, rows, rewards, rs, dones, ds, values, vs, last, adv, ret, stream)
    REFUSED(ce_ppo2_gae(nullptr, 0, 4, a, 16, d, 4, a, 16, a, a, a, nullptr), "k must");
    REFUSED(ce_ppo2_gae(nullptr, 2, 0, a, 16, d, 4, a, 16, a, a, a, nullptr), "rows must");
    REFUSED(ce_ppo2_gae(nullptr, 2, 4, nullptr, 16, d, 4, a, 16, a, a, a, nullptr), "null rewards");
    REFUSED(ce_ppo2_gae(nullptr, 2, 4, a, 16, nullptr, 4, a, 16, a, a, a, nullptr), "null dones");
    REFUSED(ce_ppo2_gae(nullptr, 2, 4, a, 16, d, 4, nullptr, 16, a, a, a, nullptr), "null values");
    REFUSED(ce_ppo2_gae(nullptr, 2, 4, a, 16, d, 4, a, 16, nullptr, a, a, nullptr), "null last_values");
    REFUSED(ce_ppo2_gae(nullptr, 2, 4, a, 16, d, 4, a, 16, a, nullptr, a, nullptr), "null adv");
    REFUSED(ce_ppo2_gae(nullptr, 2, 4, a, 16, d, 4, a, 16, a, a, nullptr, nullptr), "null adv or ret");
    REFUSED(ce_ppo2_gae(nullptr, 2, 4, a, 18, d, 4, a, 16, a, a, a, nullptr), "reward_stride_bytes");
    REFUSED(ce_ppo2_gae(nullptr, 2, 4, a, 8, d, 4, a, 16, a, a, a, nullptr), "reward_stride_bytes");
    REFUSED(ce_ppo2_gae(nullptr, 2, 4, a, 16, d, 4, a, 17, a, a, a, nullptr), "value_stride_bytes");
    REFUSED(ce_ppo2_gae(nullptr, 2, 4, a, 16, d, 3, a, 16, a, a, a, nullptr), "done_stride_bytes");
    REFUSED(ce_ppo2_gae(nullptr, 2, 4, odd, 16, d, 4, a, 16, a, a, a, nullptr), "4-byte aligned");
    REFUSED(ce_ppo2_gae(nullptr, 2, 4, a, 16, d, 4, odd, 16, a, a, a, nullptr), "4-byte aligned");
    REFUSED(ce_ppo2_gae(nullptr, 2, 4, a, 16, d, 4, a, 16, a, a, a, nullptr), "null learner");
    // k * rows past 2^24 is A2C's bound only
    REFUSED(ce_ppo2_gae(nullptr, 2, big, a, 4 * big, d, big, a, 4 * big, a, a, a, nullptr), "null learner");

    // ---- ce_ppo2_grad / _step(l, n, m, idx, obs, actions, adv, ret, old_neglogp, old_values, ...)
    REFUSED(ce_ppo2_grad(nullptr, 0, 4, nullptr, a, a, a, a, a, a, -1.0f, a, a, nullptr), "n must");
    REFUSED(ce_ppo2_grad(nullptr, 4, 0, nullptr, a, a, a, a, a, a, -1.0f, a, a, nullptr), "m must");
    REFUSED(ce_ppo2_grad(nullptr, 4, big + 1, nullptr, a, a, a, a, a, a, -1.0f, a, a, nullptr), "m must");
    REFUSED(ce_ppo2_grad(nullptr, big + 1, 4, ix, a, a, a, a, a, a, -1.0f, a, a, nullptr), "n must");
    REFUSED(ce_ppo2_grad(nullptr, 5, 4, nullptr, a, a, a, a, a, a, -1.0f, a, a, nullptr), "no idx");
    REFUSED(ce_ppo2_grad(nullptr, 4, 4, nullptr, nullptr, a, a, a, a, a, -1.0f, a, a, nullptr), "null obs");
    REFUSED(ce_ppo2_grad(nullptr, 4, 4, nullptr, a, nullptr, a, a, a, a, -1.0f, a, a, nullptr), "null actions");
    REFUSED(ce_ppo2_grad(nullptr, 4, 4, nullptr, a, a, nullptr, a, a, a, -1.0f, a, a, nullptr), "null advantages");
    REFUSED(ce_ppo2_grad(nullptr, 4, 4, nullptr, a, a, a, nullptr, a, a, -1.0f, a, a, nullptr), "null returns");
    REFUSED(ce_ppo2_grad(nullptr, 4, 4, nullptr, a, a, a, a, nullptr, a, -1.0f, a, a, nullptr), "null old_neglogp");
    REFUSED(ce_ppo2_grad(nullptr, 4, 4, nullptr, a, a, a, a, a, nullptr, -1.0f, a, a, nullptr), "null old_values");
    REFUSED(ce_ppo2_grad(nullptr, 4, 4, nullptr, a, a, a, a, a, a, -1.0f, a, nullptr, nullptr), "null stats");
    REFUSED(ce_ppo2_grad(nullptr, 4, 4, nullptr, a, a, a, a, a, a, -1.0f, nullptr, a, nullptr), "null grad");
    REFUSED(ce_ppo2_grad(nullptr, 4, 4, nullptr, a, a, a, a, a, a, -1.0f, a, a, nullptr), "null learner");
    REFUSED(ce_ppo2_grad(nullptr, 8, 4, ix, a, a, a, a, a, a, -1.0f, a, a, nullptr), "null learner");
    REFUSED(ce_ppo2_step(nullptr, 0, 4, nullptr, a, a, a, a, a, a, -1.0f, -1.0f, a, nullptr), "n must");
    REFUSED(ce_ppo2_step(nullptr, 5, 4, nullptr, a, a, a, a, a, a, -1.0f, -1.0f, a, nullptr), "no idx");
    REFUSED(ce_ppo2_step(nullptr, 4, 4, nullptr, a, a, a, a, nullptr, a, -1.0f, -1.0f, a, nullptr), "null old_neglogp");
    REFUSED(ce_ppo2_step(nullptr, 4, 4, nullptr, a, a, a, a, a, a, -1.0f, -1.0f, nullptr, nullptr), "null stats");
    REFUSED(ce_ppo2_step(nullptr, 4, 4, nullptr, a, a, a, a, a, a, -1.0f, -1.0f, a, nullptr), "null learner");

    // ---- ce_a2c_returns(l, k, rows, rewards, rs, dones, ds, last, ret, stream)
    REFUSED(ce_a2c_returns(nullptr, 0, 4, a, 16, d, 4, a, a, nullptr), "k must");
    REFUSED(ce_a2c_returns(nullptr, 2, 0, a, 16, d, 4, a, a, nullptr), "rows must");
    REFUSED(ce_a2c_returns(nullptr, 2, big, a, 4 * big, d, big, a, a, nullptr), "k * rows");
    REFUSED(ce_a2c_returns(nullptr, 2, 4, nullptr, 16, d, 4, a, a, nullptr), "null rewards");
    REFUSED(ce_a2c_returns(nullptr, 2, 4, a, 16, nullptr, 4, a, a, nullptr), "null dones");
    REFUSED(ce_a2c_returns(nullptr, 2, 4, a, 16, d, 4, nullptr, a, nullptr), "null last_values");
    REFUSED(ce_a2c_returns(nullptr, 2, 4, a, 16, d, 4, a, nullptr, nullptr), "null ret");
    REFUSED(ce_a2c_returns(nullptr, 2, 4, a, 18, d, 4, a, a, nullptr), "reward_stride_bytes");
    REFUSED(ce_a2c_returns(nullptr, 2, 4, a, 8, d, 4, a, a, nullptr), "reward_stride_bytes");
    REFUSED(ce_a2c_returns(nullptr, 2, 4, a, 16, d, 3, a, a, nullptr), "done_stride_bytes");
    REFUSED(ce_a2c_returns(nullptr, 2, 4, odd, 16, d, 4, a, a, nullptr), "4-byte aligned");
    REFUSED(ce_a2c_returns(nullptr, 2, 4, a, 16, d, 4, a, a, nullptr), "null learner");

    // ---- ce_a2c_grad / _step(l, n, m, idx, obs, actions, returns, old_values, ...)
    REFUSED(ce_a2c_grad(nullptr, 0, 4, nullptr, a, a, a, a, a, a, nullptr), "n must");
    REFUSED(ce_a2c_grad(nullptr, 4, 0, nullptr, a, a, a, a, a, a, nullptr), "m must");
    REFUSED(ce_a2c_grad(nullptr, 4, big + 1, nullptr, a, a, a, a, a, a, nullptr), "m must");
    REFUSED(ce_a2c_grad(nullptr, 5, 4, nullptr, a, a, a, a, a, a, nullptr), "no idx");
    REFUSED(ce_a2c_grad(nullptr, 4, 4, nullptr, nullptr, a, a, a, a, a, nullptr), "null obs");
    REFUSED(ce_a2c_grad(nullptr, 4, 4, nullptr, a, nullptr, a, a, a, a, nullptr), "null actions");
    REFUSED(ce_a2c_grad(nullptr, 4, 4, nullptr, a, a, nullptr, a, a, a, nullptr), "null returns");
    REFUSED(ce_a2c_grad(nullptr, 4, 4, nullptr, a, a, a, nullptr, a, a, nullptr), "null old_values");
    REFUSED(ce_a2c_grad(nullptr, 4, 4, nullptr, a, a, a, a, a, nullptr, nullptr), "null stats");
    REFUSED(ce_a2c_grad(nullptr, 4, 4, nullptr, a, a, a, a, nullptr, a, nullptr), "null grad");
    REFUSED(ce_a2c_grad(nullptr, 4, 4, nullptr, a, a, a, a, a, a, nullptr), "null learner");
    REFUSED(ce_a2c_grad(nullptr, 8, 4, ix, a, a, a, a, a, a, nullptr), "null learner");
    REFUSED(ce_a2c_step(nullptr, 0, 4, nullptr, a, a, a, a, -1.0f, a, nullptr), "n must");
    REFUSED(ce_a2c_step(nullptr, 5, 4, nullptr, a, a, a, a, -1.0f, a, nullptr), "no idx");
    REFUSED(ce_a2c_step(nullptr, 4, 4, nullptr, a, a, nullptr, a, -1.0f, a, nullptr), "null returns");
    REFUSED(ce_a2c_step(nullptr, 4, 4, nullptr, a, a, a, a, -1.0f, nullptr, nullptr), "null stats");
    REFUSED(ce_a2c_step(nullptr, 4, 4, nullptr, a, a, a, a, -1.0f, a, nullptr), "null learner");

    // ---- ce_a2c_update(l, k, rows, obs, actions, as, values, vs, rewards, rs, dones, ds, last, lr, stats, stream)
    REFUSED(ce_a2c_update(nullptr, 0, 4, a, a, 32, a, 16, a, 16, d, 4, a, -1.0f, a, nullptr), "k must");
    REFUSED(ce_a2c_update(nullptr, 2, 0, a, a, 32, a, 16, a, 16, d, 4, a, -1.0f, a, nullptr), "rows must");
    REFUSED(ce_a2c_update(nullptr, 2, 4, nullptr, a, 32, a, 16, a, 16, d, 4, a, -1.0f, a, nullptr), "null obs");
    REFUSED(ce_a2c_update(nullptr, 2, 4, a, nullptr, 32, a, 16, a, 16, d, 4, a, -1.0f, a, nullptr), "null actions");
    REFUSED(ce_a2c_update(nullptr, 2, 4, a, a, 32, nullptr, 16, a, 16, d, 4, a, -1.0f, a, nullptr), "null values");
    REFUSED(ce_a2c_update(nullptr, 2, 4, a, a, 32, a, 16, nullptr, 16, d, 4, a, -1.0f, a, nullptr), "null rewards");
    REFUSED(ce_a2c_update(nullptr, 2, 4, a, a, 32, a, 16, a, 16, nullptr, 4, a, -1.0f, a, nullptr), "null dones");
    REFUSED(ce_a2c_update(nullptr, 2, 4, a, a, 32, a, 16, a, 16, d, 4, nullptr, -1.0f, a, nullptr), "null last_values");
    REFUSED(ce_a2c_update(nullptr, 2, 4, a, a, 32, a, 16, a, 16, d, 4, a, -1.0f, nullptr, nullptr), "null stats");
    REFUSED(ce_a2c_update(nullptr, 2, 4, a, a, 32, a, 16, a, 8, d, 4, a, -1.0f, a, nullptr), "reward_stride_bytes");
    REFUSED(ce_a2c_update(nullptr, 2, 4, a, a, 32, a, 16, a, 18, d, 4, a, -1.0f, a, nullptr), "reward_stride_bytes");
    REFUSED(ce_a2c_update(nullptr, 2, 4, a, a, 32, a, 12, a, 16, d, 4, a, -1.0f, a, nullptr), "value_stride_bytes");
    REFUSED(ce_a2c_update(nullptr, 2, 4, a, a, 32, a, 17, a, 16, d, 4, a, -1.0f, a, nullptr), "value_stride_bytes");
    REFUSED(ce_a2c_update(nullptr, 2, 4, a, a, 8, a, 16, a, 16, d, 4, a, -1.0f, a, nullptr), "action_stride_bytes");
    REFUSED(ce_a2c_update(nullptr, 2, 4, a, a, 34, a, 16, a, 16, d, 4, a, -1.0f, a, nullptr), "action_stride_bytes");
    REFUSED(ce_a2c_update(nullptr, 2, 4, a, a, 32, a, 16, a, 16, d, 3, a, -1.0f, a, nullptr), "done_stride_bytes");
    REFUSED(ce_a2c_update(nullptr, 2, 4, a, a, 32, odd, 16, a, 16, d, 4, a, -1.0f, a, nullptr), "4-byte aligned");
    REFUSED(ce_a2c_update(nullptr, 2, 4, a, a, 32, a, 16, a, 16, d, 4, a, -1.0f, a, nullptr), "null learner");
}

// The refusals of ce_ddpg_* that run through the checks it shares with the two
// learners above (csrc/learner_checks.h), with a NULL handle: the same words,
// and the all-valid call refused for the handle alone.
static void ddpg_checks() {
    std::vector<double> rec(64, 0.0);
    double *r = rec.data();
    double *off = reinterpret_cast<double *>(reinterpret_cast<char *>(r) + 4);
    float *a = reinterpret_cast<float *>(r);
    const uint8_t *d = reinterpret_cast<const uint8_t *>(r);
    const int32_t *ix = reinterpret_cast<const int32_t *>(r);
    const int64_t big = int64_t(1) << 24, total = int64_t(1) << 30;
    int64_t step = 0;

    REFUSED(ce_ddpg_set_params(nullptr, nullptr, 8, 0, nullptr), "null parameter vector");
    REFUSED(ce_ddpg_set_params(nullptr, a, 8, 0, nullptr), "null learner");
    REFUSED(ce_ddpg_get_params(nullptr, nullptr, 8, 0, nullptr), "null parameter vector");
    REFUSED(ce_ddpg_get_params(nullptr, a, 8, 0, nullptr), "null learner");
    REFUSED(ce_ddpg_get_opt_state(nullptr, a, a, 8, nullptr, 0, nullptr), "null step");
    REFUSED(ce_ddpg_get_opt_state(nullptr, nullptr, a, 8, &step, 0, nullptr), "null m");
    REFUSED(ce_ddpg_get_opt_state(nullptr, a, nullptr, 8, &step, 0, nullptr), "null v");
    REFUSED(ce_ddpg_get_opt_state(nullptr, a, a, 8, &step, 0, nullptr), "null learner");
    REFUSED(ce_ddpg_set_opt_state(nullptr, a, a, 8, -1, 0, nullptr), "step must not be negative");
    REFUSED(ce_ddpg_set_opt_state(nullptr, nullptr, a, 8, 0, 0, nullptr), "null m");
    REFUSED(ce_ddpg_set_opt_state(nullptr, a, nullptr, 8, 0, 0, nullptr), "null v");
    REFUSED(ce_ddpg_set_opt_state(nullptr, a, a, 8, 0, 0, nullptr), "null learner");

    // ---- ce_ddpg_target(l, n, m, idx, obs1, rewards, dones, y, stream)
    REFUSED(ce_ddpg_target(nullptr, 0, 4, nullptr, a, a, d, a, nullptr), "n must");
    REFUSED(ce_ddpg_target(nullptr, 4, big + 1, nullptr, a, a, d, a, nullptr), "m must");
    REFUSED(ce_ddpg_target(nullptr, big + 1, 4, ix, a, a, d, a, nullptr), "n must");
    REFUSED(ce_ddpg_target(nullptr, 5, 4, nullptr, a, a, d, a, nullptr), "n exceeds m");
    REFUSED(ce_ddpg_target(nullptr, 4, 4, nullptr, a, a, d, a, nullptr), "null learner");
    REFUSED(ce_ddpg_target(nullptr, 8, 4, ix, a, a, d, a, nullptr), "null learner");

    // ---- ce_ddpg_grad(l, n, m, idx, obs0, actions, rewards, obs1, dones, y, grad, stats, stream)
    REFUSED(ce_ddpg_grad(nullptr, 0, 4, nullptr, a, a, a, a, d, a, a, a, nullptr), "n must");
    REFUSED(ce_ddpg_grad(nullptr, 5, 4, nullptr, a, a, a, a, d, a, a, a, nullptr), "n exceeds m");
    REFUSED(ce_ddpg_grad(nullptr, 4, 4, nullptr, a, a, a, a, d, a, nullptr, a, nullptr), "null grad");
    REFUSED(ce_ddpg_grad(nullptr, 4, 4, nullptr, a, a, a, a, d, a, a, a, nullptr), "null learner");

    // ---- ce_ddpg_partial(l, n, n_total, m, idx, obs0, actions, rewards, obs1, dones, y, record, stream)
    REFUSED(ce_ddpg_partial(nullptr, 0, 4, 4, nullptr, a, a, a, a, d, a, r, nullptr), "n must");
    REFUSED(ce_ddpg_partial(nullptr, 5, 5, 4, nullptr, a, a, a, a, d, a, r, nullptr), "n exceeds m");
    REFUSED(ce_ddpg_partial(nullptr, 4, 3, 4, nullptr, a, a, a, a, d, a, r, nullptr), "n_total must");
    REFUSED(ce_ddpg_partial(nullptr, 4, total + 1, 4, nullptr, a, a, a, a, d, a, r, nullptr), "n_total must");
    REFUSED(ce_ddpg_partial(nullptr, 4, 4, 4, nullptr, a, a, a, a, d, a, nullptr, nullptr), "null record");
    REFUSED(ce_ddpg_partial(nullptr, 4, 4, 4, nullptr, a, a, a, a, d, a, off, nullptr), "8-byte aligned");
    REFUSED(ce_ddpg_partial(nullptr, 4, 4, 4, nullptr, a, a, a, a, d, nullptr, r, nullptr), "null y buffer");
    REFUSED(ce_ddpg_partial(nullptr, 4, total, 4, nullptr, a, a, a, a, d, a, r, nullptr), "null learner");

    // ---- ce_ddpg_combine(l, world, records, n_total, grad, stats, stream): grad comes first
    REFUSED(ce_ddpg_combine(nullptr, 0, r, 8, nullptr, a, nullptr), "null grad");
    REFUSED(ce_ddpg_combine(nullptr, 0, r, 8, a, a, nullptr), "world must");
    REFUSED(ce_ddpg_combine(nullptr, (1 << 16) + 1, r, 8, a, a, nullptr), "world must");
    REFUSED(ce_ddpg_combine(nullptr, 2, r, 0, a, a, nullptr), "n_total must");
    REFUSED(ce_ddpg_combine(nullptr, 2, r, total + 1, a, a, nullptr), "n_total must");
    REFUSED(ce_ddpg_combine(nullptr, 2, nullptr, 8, a, a, nullptr), "null records");
    REFUSED(ce_ddpg_combine(nullptr, 2, off, 8, a, a, nullptr), "8-byte aligned");
    REFUSED(ce_ddpg_combine(nullptr, 2, r, 8, a, nullptr, nullptr), "null stats");
    REFUSED(ce_ddpg_combine(nullptr, 2, r, 8, a, a, nullptr), "null learner");

    // ---- ce_ddpg_apply(l, world, records, n_total, actor_lr, critic_lr, stats, stream)
    REFUSED(ce_ddpg_apply(nullptr, 0, r, 8, -1.0, -1.0, a, nullptr), "world must");
    REFUSED(ce_ddpg_apply(nullptr, 2, r, 0, -1.0, -1.0, a, nullptr), "n_total must");
    REFUSED(ce_ddpg_apply(nullptr, 2, nullptr, 8, -1.0, -1.0, a, nullptr), "null records");
    REFUSED(ce_ddpg_apply(nullptr, 2, off, 8, -1.0, -1.0, a, nullptr), "8-byte aligned");
    REFUSED(ce_ddpg_apply(nullptr, 2, r, 8, -1.0, -1.0, nullptr, nullptr), "null stats");
    REFUSED(ce_ddpg_apply(nullptr, 2, r, 8, -1.0, -1.0, a, nullptr), "null learner");
}

// The library's test hooks (csrc/engine.hip; not part of the public header).
extern "C" int ce_test_plan(const ce_config *cfg, const int32_t *labels, char *step_name,
                            char *many_name, int32_t cap);
extern "C" int64_t ce_test_dataset_image(const ce_config *cfg, const double *features,
                                         const int32_t *labels, void *out, int64_t cap);

static ce_config plan_config(int problem, int precision, int N, int F, int K, int B) {
    ce_config c{};
    c.abi_version = CE_ABI_VERSION;
    c.problem = problem;
    c.precision = precision;
    c.num_envs = 4;
    c.n_rows = N;
    c.n_features = F;
    c.n_classes = K;
    c.batch_size = B;
    c.max_steps = 40;
    c.auto_reset = 1;
    c.n_hidden = 64;
    return c;
}

// Plan the config and build its dataset image into an exactly sized heap
// buffer (ASan guards both ends); the kernel name must start with `kernel`.
static void plan_and_image(const ce_config &c, const char *kernel) {
    std::vector<double> X(static_cast<size_t>(c.n_rows) * c.n_features);
    std::vector<int32_t> y(c.n_rows);
    for (size_t i = 0; i < X.size(); ++i) X[i] = 0.25 * static_cast<double>(i % 7) - 0.5;
    for (int r = 0; r < c.n_rows; ++r) y[r] = r % c.n_classes;
    char step[128], many[128];
    EXPECT(ce_test_plan(&c, y.data(), step, many, sizeof(step)) == CE_OK);
    EXPECT(std::strncmp(step, kernel, std::strlen(kernel)) == 0);
    const int64_t bytes = ce_test_dataset_image(&c, X.data(), y.data(), nullptr, 0);
    EXPECT(bytes > 0);
    if (bytes <= 0) return;
    std::vector<unsigned char> img(bytes);
    EXPECT(ce_test_dataset_image(&c, X.data(), y.data(), img.data(), bytes) == bytes);
    EXPECT(ce_test_dataset_image(&c, X.data(), y.data(), img.data(), bytes - 1) == bytes);
}

// ce_create's plan and its host-side image builders (no device needed): the
// smallest shapes that exercise each pad, per path.
static void plan_checks() {
    plan_and_image(plan_config(CE_PROBLEM_SOFTMAX, CE_F64, 5, 3, 3, 5), "optimize_step_kernel<double,3,3");
    plan_and_image(plan_config(CE_PROBLEM_SOFTMAX, CE_F32, 5, 3, 3, 5), "optimize_step_kernel<float,3,3");
    plan_and_image(plan_config(CE_PROBLEM_SOFTMAX, CE_F64, 5, 2, 2, 3), "optimize_pair_kernel<double,2");
    plan_and_image(plan_config(CE_PROBLEM_SOFTMAX, CE_F64, 1, 17, 5, 1), "optimize_mfma_kernel<5>");
    plan_and_image(plan_config(CE_PROBLEM_SOFTMAX, CE_F64, 65, 17, 5, 65), "optimize_mfma_kernel<5>");
    plan_and_image(plan_config(CE_PROBLEM_SOFTMAX, CE_F64, 1, 1, 2, 1), "optimize_lr_mfma_kernel<1,");
    plan_and_image(plan_config(CE_PROBLEM_SOFTMAX, CE_F64, 256, 10, 2, 256), "optimize_lr_mfma_kernel<3,");
    plan_and_image(plan_config(CE_PROBLEM_SOFTMAX, CE_F64, 300, 13, 2, 300), "optimize_lr_mfma_kernel<4,");
    plan_and_image(plan_config(CE_PROBLEM_MLP, CE_F32, 64, 8, 10, 32), "mlp_step_kernel");
    plan_and_image(plan_config(CE_PROBLEM_MLP, CE_F32, 128, 16, 10, 32), "mlp_step_kernel");
    ce_config net = plan_config(CE_PROBLEM_MLP, CE_F32, 100, 12, 7, 20);
    net.n_layers = 4;
    net.hidden[0] = 96;
    net.hidden[1] = 33;
    net.hidden[2] = 7;
    net.hidden[3] = 48;
    plan_and_image(net, "net<12,96,33,7,48,7>:mfma");
    net.hidden[1] = 300;
    plan_and_image(net, "net<12,96,300,7,48,7>:wide");
    char name[8];
    ce_config lr = plan_config(CE_PROBLEM_SOFTMAX, CE_F64, 256, 10, 2, 256);
    std::vector<int32_t> y(256, 1);
    EXPECT(ce_test_plan(&lr, y.data(), name, nullptr, sizeof(name)) == CE_OK);   // a short buffer
    EXPECT(std::strcmp(name, "optimiz") == 0);
    y[255] = 2;
    EXPECT(ce_test_plan(&lr, y.data(), name, name, sizeof(name)) == CE_EINVAL);
    EXPECT(ce_test_plan(nullptr, nullptr, nullptr, nullptr, 0) == CE_EINVAL);
    EXPECT(ce_test_dataset_image(&lr, nullptr, y.data(), nullptr, 0) == CE_EINVAL);
}

int main() {
    EXPECT(ce_abi_version() == CE_ABI_VERSION);
    // ---- host-only draws: edge seeds and shapes
    const uint64_t seeds[] = {0ull, 3ull, 2147483647ull, 8589934592ull, 18446744073709551615ull};
    for (uint64_t s : seeds) {
        std::vector<double> w(10 * 2);
        std::vector<int32_t> p(256);
        EXPECT(ce_seed_draws(s, 10, 2, 256, w.data(), p.data()) == CE_OK);
        std::printf("seed %llu\n", static_cast<unsigned long long>(s));
        dump("lr_w", w);
        dump("lr_p", p);
        const int F = 24, H = 64, K = 10, N = 200;
        std::vector<float> wm(F * H + H + H * K + K);
        std::vector<int32_t> pm(N);
        EXPECT(ce_seed_draws_mlp(s, F, H, K, N, wm.data(), pm.data()) == CE_OK);
        dump("mlp_w", wm);
        dump("mlp_p", pm);
        const int32_t dims[] = {4, 32, 3};
        const int P = 4 * 32 + 32 + 32 * 3 + 3;
        std::vector<float> wn(P);
        std::vector<int32_t> rp(150), ep(150);
        EXPECT(ce_nn_seed_draws(s, 3, dims, 150, wn.data(), rp.data(), ep.data()) == CE_OK);
        dump("nn_w", wn);
        dump("nn_rp", rp);
        dump("nn_ep", ep);
        EXPECT(ce_nn_seed_draws(s, 3, dims, 150, nullptr, nullptr, ep.data()) == CE_OK);
    }
    {   // one row, a large permutation
        std::vector<double> w(3 * 3);
        std::vector<int32_t> p(1);
        EXPECT(ce_seed_draws(7, 3, 3, 1, w.data(), p.data()) == CE_OK && p[0] == 0);
        std::vector<int32_t> big(1 << 20);
        std::vector<double> w2(64 * 16);
        EXPECT(ce_seed_draws(9, 64, 16, 1 << 20, w2.data(), big.data()) == CE_OK);
        std::vector<char> seen(big.size(), 0);
        for (int32_t r : big) EXPECT(r >= 0 && r < (1 << 20) && !seen[r]++);
    }
    // ---- argument validation: every entry point rejects what it must,
    // with a message, and never dereferences a null engine
    EXPECT(ce_seed_draws(1, 0, 2, 10, nullptr, nullptr) == CE_EINVAL);
    EXPECT(ce_seed_draws_mlp(1, 4, 0, 3, 10, nullptr, nullptr) == CE_EINVAL);
    EXPECT(ce_create(nullptr, nullptr, nullptr, nullptr) == CE_EINVAL);
    EXPECT(std::strlen(ce_last_error()) > 0);
    std::vector<double> X(16 * 128, 0.5);
    std::vector<int32_t> y(128, 1);
    ce_engine *eng = nullptr;
    ce_config cfg{};
    cfg.abi_version = CE_ABI_VERSION + 1;
    EXPECT(ce_create(&cfg, X.data(), y.data(), &eng) == CE_EINVAL && eng == nullptr);
    cfg.abi_version = CE_ABI_VERSION;
    cfg.num_envs = 2;
    cfg.n_rows = 128;
    cfg.n_features = 16;
    cfg.n_classes = 10;
    cfg.batch_size = 129;                       // > n_rows
    cfg.max_steps = 40;
    cfg.precision = CE_F64;
    EXPECT(ce_create(&cfg, X.data(), y.data(), &eng) == CE_EINVAL);
    cfg.batch_size = 32;
    cfg.max_steps = 0;
    EXPECT(ce_create(&cfg, X.data(), y.data(), &eng) == CE_EINVAL);
    cfg.max_steps = 40;
    y[5] = 10;                                  // label out of range
    EXPECT(ce_create(&cfg, X.data(), y.data(), &eng) == CE_EINVAL);
    y[5] = 1;
    cfg.n_features = 65;                        // past the f64 MFMA kernel's F <= 64
    std::vector<double> X65(65 * 128, 0.5);
    EXPECT(ce_create(&cfg, X65.data(), y.data(), &eng) == CE_EUNSUPPORTED);
    // the network path's geometry checks (net_geometry) run before any HIP call
    cfg.n_features = 16;
    cfg.problem = CE_PROBLEM_MLP;
    cfg.precision = CE_F32;
    cfg.n_layers = 2;
    cfg.hidden[0] = 9000;                       // past the wide-layer path's 8192 units
    cfg.hidden[1] = 64;
    EXPECT(ce_create(&cfg, X.data(), y.data(), &eng) == CE_EUNSUPPORTED);
    cfg.hidden[0] = 0;
    EXPECT(ce_create(&cfg, X.data(), y.data(), &eng) == CE_EINVAL);
    cfg.hidden[0] = 64;
    cfg.n_classes = 33;
    EXPECT(ce_create(&cfg, X.data(), y.data(), &eng) == CE_EUNSUPPORTED);
    cfg.n_classes = 10;
    cfg.n_layers = 5;
    EXPECT(ce_create(&cfg, X.data(), y.data(), &eng) == CE_EUNSUPPORTED);
    // null engines everywhere
    EXPECT(ce_num_envs(nullptr) == CE_EINVAL);
    EXPECT(ce_set_stream(nullptr, nullptr) == CE_EINVAL);
    EXPECT(ce_set_compact_outputs(nullptr, 1) == CE_EINVAL);
    EXPECT(ce_seed(nullptr, nullptr, 0) == CE_EINVAL);
    EXPECT(ce_reset(nullptr, nullptr, 0) == CE_EINVAL);
    EXPECT(ce_step(nullptr, nullptr, nullptr, 0) == CE_EINVAL);
    EXPECT(ce_step_many(nullptr, 4, nullptr, 0, nullptr) == CE_EINVAL);
    EXPECT(ce_get_state(nullptr, nullptr) == CE_EINVAL);
    EXPECT(ce_set_state(nullptr, nullptr) == CE_EINVAL);
    EXPECT(ce_host_outputs(nullptr, nullptr) == CE_EINVAL);
    EXPECT(std::strcmp(ce_step_kernel(nullptr), "") == 0);
    ce_destroy(nullptr);
    EXPECT(ce_multi_create(nullptr, nullptr) == CE_EINVAL);
    ce_multi_destroy(nullptr);
    EXPECT(ce_nn_create(nullptr, nullptr, nullptr, nullptr) == CE_EINVAL);
    ce_nn_destroy(nullptr);
    learner_checks();
    ddpg_checks();
    plan_checks();
    std::printf("failures %d\n", failures);
    return failures ? 1 : 0;
}
