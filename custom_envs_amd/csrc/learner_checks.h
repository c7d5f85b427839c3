// The argument checks every learner shares (ppo2_engine.hip and a2c_engine.hip
// through learner_host.h, ddpg_engine.hip directly): they need no PolicyPlan
// and no kernel, only the plain arguments, so each refusal has one text.  None
// of them checks the handle: an entry point does that last among its argument
// checks, so the others run without a device.
#pragma once

#include <cstdint>
#include <string>

#include "common.h"

namespace ce {

constexpr int64_t kLearnerMaxRows = int64_t(1) << 24;
constexpr int64_t kLearnerMaxTotalRows = int64_t(1) << 30;
constexpr int kLearnerMaxWorld = 1 << 16;

// `flat` and its length of a set_params / get_params call; `n_params` < 0: a
// null learner.  `noun`: what has the parameters ("policy", "agent").
inline int learner_params_ok(const char *who, int n_params, const char *noun, const void *flat,
                             int64_t n, const char *got) {
    if (!flat) return fail(CE_EINVAL, std::string(who) + ": null parameter vector");
    if (n_params < 0) return fail(CE_EINVAL, std::string(who) + ": null learner");
    if (n != n_params)
        return fail(CE_EINVAL, std::string(who) + got + std::to_string(n) + " parameters, the " +
                                   noun + " has " + std::to_string(n_params));
    return CE_OK;
}

// The optimiser's state in and out.  A learner names its two [n_params]
// float32 blocks once (Adam's m and v; A2C: RMSProp's ms and mom); this copies
// them to (`set` false) or from (`set` true) the caller's `a` and `b`: host
// pointers (synchronises) or, under CE_PTR_DEVICE, device pointers
// (stream-ordered).  `n_params` < 0: a null learner, and dev_a / dev_b unread.
inline int learner_opt_state(const char *who, int n_params, const char *noun, float *dev_a,
                             float *dev_b, const char *name_a, const char *name_b, void *a, void *b,
                             int64_t n, bool set, uint32_t flags, void *hip_stream) {
    const auto bad = [who](const std::string &what) { return fail(CE_EINVAL, who + what); };
    if (!a) return bad(std::string(": null ") + name_a);
    if (!b) return bad(std::string(": null ") + name_b);
    if (n_params < 0) return bad(": null learner");
    if (n != n_params)
        return bad(": got " + std::to_string(n) + " entries per block, the " + noun + " has " +
                   std::to_string(n_params) + " parameters");
    CE_CLEAR_STALE_ERROR_AT(who);
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const bool dev = (flags & CE_PTR_DEVICE) != 0;
    const size_t bytes = static_cast<size_t>(n) * sizeof(float);
    const hipMemcpyKind kind = dev ? hipMemcpyDeviceToDevice
                                   : (set ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost);
    if (set) {
        CE_HIP(hipMemcpyAsync(dev_a, a, bytes, kind, stream));
        CE_HIP(hipMemcpyAsync(dev_b, b, bytes, kind, stream));
    } else {
        CE_HIP(hipMemcpyAsync(a, dev_a, bytes, kind, stream));
        CE_HIP(hipMemcpyAsync(b, dev_b, bytes, kind, stream));
    }
    if (!dev) CE_HIP(hipStreamSynchronize(stream));   // the host blocks may be pageable
    return CE_OK;
}

// n rows gathered by idx (null: the first n) out of an m-row batch
inline int learner_rows_ok(const char *who, int64_t n, int64_t m, const int32_t *idx) {
    const auto bad = [who](const std::string &what) { return fail(CE_EINVAL, who + what); };
    if (n < 1) return bad(": n must be at least 1, got " + std::to_string(n));
    if (m < 1 || m > kLearnerMaxRows)
        return bad(": m must be in [1, 2^24], got " + std::to_string(m));
    if (n > kLearnerMaxRows) return bad(": n must be at most 2^24");
    if (!idx && n > m) return bad(": n exceeds m and there is no idx to gather by");
    return CE_OK;
}

// n_total and the record of a partial call (after learner_rows_ok)
inline int learner_partial_ok(const char *who, int64_t n, int64_t n_total, const void *record) {
    const auto bad = [who](const std::string &what) { return fail(CE_EINVAL, who + what); };
    if (n_total < n || n_total > kLearnerMaxTotalRows)
        return bad(": n_total must be in [n, 2^30], got " + std::to_string(n_total) + " for n = " +
                   std::to_string(n));
    if (!record) return bad(": null record");
    if (reinterpret_cast<uintptr_t>(record) & 7) return bad(": the record must be 8-byte aligned");
    return CE_OK;
}

// world, the gathered records, n_total and stats of an apply / combine call
inline int learner_apply_ok(const char *who, int32_t world, const void *records, int64_t n_total,
                            const void *stats) {
    const auto bad = [who](const std::string &what) { return fail(CE_EINVAL, who + what); };
    if (world < 1 || world > kLearnerMaxWorld)
        return bad(": world must be in [1, 2^16], got " + std::to_string(world));
    if (n_total < 1 || n_total > kLearnerMaxTotalRows)
        return bad(": n_total must be in [1, 2^30], got " + std::to_string(n_total));
    if (!records) return bad(": null records");
    if (reinterpret_cast<uintptr_t>(records) & 7) return bad(": the records must be 8-byte aligned");
    if (!stats) return bad(": null stats");
    return CE_OK;
}

}  // namespace ce
