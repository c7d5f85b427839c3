// The host shell the three engines share (engine.hip, multi_engine.hip,
// multinn_engine.hip): the output-struct description, the stream / staging
// buffers / K-step bookkeeping every engine holds (ce::Host), and the bodies
// of the entry points that differ between engines only in what they launch.
//
// An engine keeps its config checks, its device state and, in an `Ops`
// struct of static functions, how it launches:
//   int Ops::step(E *e, const float *act, const Outputs &o, bool device_form)
//   int Ops::reset(E *e, const Outputs &o, bool device_form)
//   int Ops::persist(E *e, int k, const float *act, int64_t stride,
//                    const Outputs &o, int64_t out_step)        (K-step engines)
//   void Ops::policy_shape(const E *e, int *obs_dim, int *act_dim, int64_t *rows)
//                                                               (rollout-policy)
// each enqueues on e->host.stream and returns CE_OK or a failed status.
// `device_form` is true when `o` was given in a CE_PTR_DEVICE-style call (the
// caller's buffers, in the compact form when that is on) and false for the
// host-staged forms (the engine's own region, always the full form).
// Dispatch is static (templates on Ops); nothing here allocates on a call path.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "common.h"
#include "policy_engine.h"
#include "vecnorm_engine.h"

namespace ce {

// The members of an output struct in region order: each(f) calls
// f(index, member pointer, optional), `optional` marking the members the
// compact form leaves out (ce_set_compact_outputs: no done, it is
// episode_len >= max_steps, and no reward, it is -objective when B = N).
template <typename O>
struct OutputMembers;

template <>
struct OutputMembers<ce_outputs> {
    static constexpr int kCount = 6;
    template <typename F>
    static void each(F &&f) {
        f(0, &ce_outputs::obs, false);
        f(1, &ce_outputs::reward, true);
        f(2, &ce_outputs::objective, false);
        f(3, &ce_outputs::accuracy, false);
        f(4, &ce_outputs::episode_len, false);
        f(5, &ce_outputs::done, true);
    }
};

template <>
struct OutputMembers<ce_multi_outputs> {
    static constexpr int kCount = 5;
    template <typename F>
    static void each(F &&f) {
        f(0, &ce_multi_outputs::obs, false);
        f(1, &ce_multi_outputs::reward, false);
        f(2, &ce_multi_outputs::info, false);
        f(3, &ce_multi_outputs::episode_len, false);
        f(4, &ce_multi_outputs::done, false);
    }
};

// every output pointer set (the compact form may leave the optional ones null)
template <typename O>
bool complete(const O *o, bool compact = false) {
    bool ok = o != nullptr;
    if (ok) OutputMembers<O>::each([&](int, auto m, bool optional) {
        if (!(o->*m) && !(optional && compact)) ok = false;
    });
    return ok;
}

// The outputs of step s of a strided run: every pointer `bytes` further on.
template <typename O>
O advance(const O &o, int64_t bytes) {
    O r = o;
    OutputMembers<O>::each([&](int, auto m, bool) {
        using P = std::remove_reference_t<decltype(r.*m)>;
        if (r.*m) r.*m = reinterpret_cast<P>(reinterpret_cast<char *>(r.*m) + bytes);
    });
    return r;
}

inline bool aligned(const void *p, size_t n) { return reinterpret_cast<uintptr_t>(p) % n == 0; }

// OptEnvRunner's rows: the agent names "parameter-i" sorted as strings
// (optvecenv.py:10-14,22-23).  row_agent[r] is the agent on output row r,
// agent_row its inverse.
inline void sorted_agent_rows(size_t P, std::vector<int32_t> *row_agent,
                              std::vector<int32_t> *agent_row) {
    std::vector<std::string> names(P);
    for (size_t i = 0; i < P; ++i) names[i] = "parameter-" + std::to_string(i);
    row_agent->resize(P);
    agent_row->resize(P);
    for (size_t i = 0; i < P; ++i) (*row_agent)[i] = static_cast<int32_t>(i);
    std::sort(row_agent->begin(), row_agent->end(),
              [&](int32_t x, int32_t y) { return names[x] < names[y]; });
    for (size_t r = 0; r < P; ++r) (*agent_row)[(*row_agent)[r]] = static_cast<int32_t>(r);
}

// fn(i) for every i < n on up to 16 host threads, thread t taking i = t,
// t + threads, ...: the per-env seed draws (a thread past n would draw nothing)
template <typename Fn>
void for_each_strided(size_t n, Fn &&fn) {
    const size_t hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
    const size_t nt = std::min(hw, n);
    std::vector<std::thread> pool;
    for (size_t t = 0; t < nt; ++t)
        pool.emplace_back([&fn, n, nt, t] {
            for (size_t i = t; i < n; i += nt) fn(i);
        });
    for (auto &th : pool) th.join();
}

// What every engine holds besides its own device state.
template <typename O>
struct Host {
    static constexpr int kMembers = OutputMembers<O>::kCount;
    hipStream_t own_stream = nullptr, stream = nullptr;
    // host-staged calls: actions and outputs go through pinned mirrors
    size_t act_bytes = 0;
    float *d_act = nullptr, *h_act = nullptr;
    // outputs: one region on the device, a pinned mirror on the host; member
    // i takes bytes[i] per step at off[i] (16-byte aligned)
    size_t bytes[kMembers] = {0}, off[kMembers] = {0};
    size_t out_bytes = 0;
    char *d_out = nullptr, *h_out = nullptr;
    bool was_reset = false;
    GraphCache graphs;        // step_many: k captured one-step launches
    // step_many: k <= many_direct steps are plain launches, longer runs a
    // cached hipGraph (0: always the graph)
    int many_direct = 0;
    // the K-step kernel: available for the shape, and chosen
    // (ce_*_set_persistent; CE_PERSIST=0 at create turns it off)
    bool persist = false, persist_on = true;
    // what the K-step kernel and the strided form need of the caller's obs
    // (16 where the observation block is stored as 16-byte units)
    size_t obs_align = 1;
    // device-form calls write the compact form (ce_set_compact_outputs)
    bool compact = false;

    bool persistent() const { return persist && persist_on; }

    O region(char *base) const {
        O o;
        OutputMembers<O>::each([&](int i, auto m, bool) {
            o.*m = reinterpret_cast<std::remove_reference_t<decltype(o.*m)>>(base + off[i]);
        });
        return o;
    }

    void copy_out(const O &src, const O *dst) const {
        if (!dst) return;
        OutputMembers<O>::each([&](int i, auto m, bool) {
            if (dst->*m) std::memcpy(dst->*m, src.*m, bytes[i]);
        });
    }

    // The device, the stream, the action staging buffers and the zeroed
    // output region with its mirror.  On failure the caller destroys.
    int create(int device, size_t action_bytes, const size_t (&member_bytes)[kMembers]) {
        CE_HIP(hipSetDevice(device));
        CE_HIP(hipStreamCreateWithFlags(&own_stream, hipStreamNonBlocking));
        stream = own_stream;
        act_bytes = action_bytes;
        CE_HIP(hipMalloc(&d_act, act_bytes));
        CE_HIP(hipHostMalloc(reinterpret_cast<void **>(&h_act), act_bytes));
        out_bytes = 0;
        for (int i = 0; i < kMembers; ++i) {
            bytes[i] = member_bytes[i];
            off[i] = out_bytes;
            out_bytes = align16(out_bytes + bytes[i]);
        }
        CE_HIP(hipMalloc(&d_out, out_bytes));
        CE_HIP(hipHostMalloc(reinterpret_cast<void **>(&h_out), out_bytes));
        CE_HIP(hipMemset(d_out, 0, out_bytes));
        std::memset(h_out, 0, out_bytes);
        if (const char *pe = std::getenv("CE_PERSIST")) persist_on = pe[0] != '0';
        return CE_OK;
    }

    // wait for the stream and drop the captured graphs (before an engine
    // frees what they reference)
    void drain() {
        if (stream) (void)hipStreamSynchronize(stream);
        graphs.release();
    }

    // drain, then free the engine's device allocations `dev` with the shell's
    void destroy(std::initializer_list<void *> dev) {
        drain();
        for (void *p : dev)
            if (p) (void)hipFree(p);
        if (d_act) (void)hipFree(d_act);
        if (d_out) (void)hipFree(d_out);
        if (h_out) (void)hipHostFree(h_out);
        if (h_act) (void)hipHostFree(h_act);
        if (own_stream) (void)hipStreamDestroy(own_stream);
    }
};

// ---- entry-point bodies ----------------------------------------------------

// a device-form call's `out` (null: the engine's own region)
template <typename O>
int caller_outputs_ok(const Host<O> &h, const O *out) {
    if (h.compact && !out) return fail(CE_EINVAL, "compact outputs need caller buffers");
    if (out && !complete(out, h.compact)) return fail(CE_EINVAL, "device outputs must all be set");
    return CE_OK;
}

template <class Ops, class E, class O>
int host_step(E *e, const float *actions, const O *out, uint32_t flags, bool sync) {
    if (!e) return fail(CE_EINVAL, "null engine");
    CE_CLEAR_STALE_ERROR();
    Host<O> &h = e->host;
    if (!h.was_reset) return fail(CE_ESTATE, "step() before the first reset()");
    if (!actions) return fail(CE_EINVAL, "null actions");
    int rc;
    if (flags & CE_PTR_DEVICE) {
        if ((rc = caller_outputs_ok(h, out)) != CE_OK) return rc;
        if ((rc = Ops::step(e, actions, out ? *out : h.region(h.d_out), true)) != CE_OK) return rc;
        CE_HIP(hipGetLastError());
        if (sync) CE_HIP(hipStreamSynchronize(h.stream));
        return CE_OK;
    }
    std::memcpy(h.h_act, actions, h.act_bytes);
    CE_HIP(hipMemcpyAsync(h.d_act, h.h_act, h.act_bytes, hipMemcpyHostToDevice, h.stream));
    if ((rc = Ops::step(e, h.d_act, h.region(h.d_out), false)) != CE_OK) return rc;
    CE_HIP(hipGetLastError());
    CE_HIP(hipMemcpyAsync(h.h_out, h.d_out, h.out_bytes, hipMemcpyDeviceToHost, h.stream));
    if (sync) {
        CE_HIP(hipStreamSynchronize(h.stream));
        h.copy_out(h.region(h.h_out), out);
    }
    return CE_OK;
}

template <class Ops, class E, class O>
int host_reset(E *e, const O *out, uint32_t flags) {
    if (!e) return fail(CE_EINVAL, "null engine");
    CE_CLEAR_STALE_ERROR();
    Host<O> &h = e->host;
    int rc;
    if (flags & CE_PTR_DEVICE) {
        if ((rc = caller_outputs_ok(h, out)) != CE_OK) return rc;
        if ((rc = Ops::reset(e, out ? *out : h.region(h.d_out), true)) != CE_OK) return rc;
        CE_HIP(hipGetLastError());
        h.was_reset = true;
        return CE_OK;
    }
    if ((rc = Ops::reset(e, h.region(h.d_out), false)) != CE_OK) return rc;
    CE_HIP(hipGetLastError());
    CE_HIP(hipMemcpyAsync(h.h_out, h.d_out, h.out_bytes, hipMemcpyDeviceToHost, h.stream));
    CE_HIP(hipStreamSynchronize(h.stream));
    h.was_reset = true;
    if (out && out->obs) std::memcpy(out->obs, h.region(h.h_out).obs, h.bytes[0]);
    return CE_OK;
}

template <class E>
int host_wait(E *e) {
    if (!e) return fail(CE_EINVAL, "null engine");
    CE_HIP(hipStreamSynchronize(e->host.stream));
    return CE_OK;
}

template <class E>
int host_set_stream(E *e, void *stream) {
    if (!e) return fail(CE_EINVAL, "null engine");
    e->host.stream = stream ? static_cast<hipStream_t>(stream) : e->host.own_stream;
    return CE_OK;
}

template <class E, class O>
int host_outputs(E *e, O *view) {
    if (!e || !view) return fail(CE_EINVAL, "null argument");
    *view = e->host.region(e->host.h_out);
    return CE_OK;
}

template <class E>
int host_set_persistent(E *e, int32_t on) {
    if (!e) return fail(CE_EINVAL, "null engine");
    e->host.persist_on = on != 0;
    return CE_OK;
}

// the arguments every K-step form checks
template <class E, class O>
int many_args_ok(const E *e, int32_t k, const float *actions, int64_t stride, const O *out) {
    if (!e) return fail(CE_EINVAL, "null engine");
    if (!e->host.was_reset) return fail(CE_ESTATE, "step_many() before the first reset()");
    if (k <= 0 || !actions || stride < 0) return fail(CE_EINVAL, "step_many: bad arguments");
    return caller_outputs_ok(e->host, out);
}

// k steps of every env, actions s * stride apart, outputs s * out_step bytes
// apart (one Ops::step per step).
template <class Ops, class E, class O>
int launch_steps(E *e, int k, const float *actions, int64_t stride, const O &o, int64_t out_step) {
    for (int s = 0; s < k; ++s) {
        const int rc = Ops::step(e, actions + s * stride, advance(o, s * out_step), true);
        if (rc != CE_OK) return rc;
    }
    return CE_OK;
}

// step_many (`launch`) and step_many_prepare (!`launch`): the K-step kernel
// where the engine has one and it is on, else plain launches up to
// many_direct steps, else a cached graph of the k launches.
template <class Ops, class E, class O>
int host_step_many(E *e, int32_t k, const float *actions, int64_t stride, const O *out,
                   bool launch) {
    int rc = many_args_ok(e, k, actions, stride, out);
    if (rc != CE_OK) return rc;
    Host<O> &h = e->host;
    const O o = out ? *out : h.region(h.d_out);
    if (h.persistent()) {
        // refused, never served by another form while ce_*_step_many_kernel()
        // names the K-step kernel
        if (!aligned(o.obs, h.obs_align))
            return fail(CE_EINVAL, "the persistent K-step kernel needs a 16-byte aligned obs "
                                   "(ce_set_persistent(e, 0) selects the per-step launches)");
        if (!launch) return CE_OK;   // one launch: nothing to instantiate
        CE_CLEAR_STALE_ERROR();
        if ((rc = Ops::persist(e, k, actions, stride, o, 0)) != CE_OK) return rc;
        CE_HIP(hipGetLastError());
        return CE_OK;
    }
    if (launch && k <= h.many_direct) {
        CE_CLEAR_STALE_ERROR();
        if ((rc = launch_steps<Ops>(e, k, actions, stride, o, 0)) != CE_OK) return rc;
        CE_HIP(hipGetLastError());
        return CE_OK;
    }
    hipGraphExec_t exec;
    rc = h.graphs.get(graph_key(k, 0, actions, stride, h.stream, o),
                      [&] { (void)launch_steps<Ops>(e, k, actions, stride, o, 0); }, &exec);
    if (rc != CE_OK) return rc;
    if (launch) CE_HIP(hipGraphLaunch(exec, h.stream));
    return CE_OK;
}

template <class Ops, class E, class O>
int host_step_many_strided(E *e, int32_t k, const float *actions, int64_t stride, const O *out,
                           int64_t out_step) {
    int rc = many_args_ok(e, k, actions, stride, out);
    if (rc != CE_OK) return rc;
    if (!out) return fail(CE_EINVAL, "step_many_strided: needs caller output buffers");
    if (out_step < 0 || out_step % 16 != 0)
        return fail(CE_EINVAL, "step_many_strided: out_step_bytes must be a non-negative "
                               "multiple of 16");
    Host<O> &h = e->host;
    if (!aligned(out->obs, h.obs_align))
        return fail(CE_EINVAL, "step_many_strided: obs must be 16-byte aligned");
    CE_CLEAR_STALE_ERROR();
    rc = h.persistent() ? Ops::persist(e, k, actions, stride, *out, out_step)
                        : launch_steps<Ops>(e, k, actions, stride, *out, out_step);
    if (rc != CE_OK) return rc;
    CE_HIP(hipGetLastError());
    return CE_OK;
}

// [policy, env step] x k: step s reads the observation step s - 1 wrote
// (obs0 first) and writes record s of `out` and `pout`; its noise is
// `noise.at(s)`: the caller's block s, or draw t0 + s of the generator.  The
// arguments are checked before was_reset.  With `vn` a third launch per step
// normalises record s's obs and reward into vn's slot s + 1 and record s, and
// the policy reads the normalised slots (obs0 is slot 0); the raw records stay.
template <class Ops, class E, class O>
int host_rollout_policy(const char *who, E *e, const ce_policy *p, int32_t k, const float *obs0,
                        const PolicyNoise &noise, const O *out, int64_t out_step,
                        const ce_policy_outputs *pout, int64_t pout_step,
                        const VecnormRollout *vn = nullptr) {
    const auto bad = [who](int code, const char *what) { return fail(code, std::string(who) + what); };
    if (noise.generated) {      // needs no engine: checked first
        const int rc = policy_rng_args_ok(who, k, 0, noise.t0, noise.row0);
        if (rc != CE_OK) return rc;
    }
    if (!e) return bad(CE_EINVAL, ": null engine");
    if (!complete(out)) return bad(CE_EINVAL, ": device outputs must all be set");
    Host<O> &h = e->host;
    if (h.compact)
        return bad(CE_EINVAL, ": needs the full output form (compact outputs are on)");
    int obs_dim, act_dim;
    int64_t rows;
    Ops::policy_shape(e, &obs_dim, &act_dim, &rows);
    int rc = policy_rollout_args_ok(who, p, obs_dim, act_dim, k, obs0, noise.ptr, noise.stride,
                                    rows, out->obs, out_step, pout, pout_step);
    if (rc != CE_OK) return rc;
    if (noise.generated && (rc = policy_rng_args_ok(who, k, rows, noise.t0, noise.row0)) != CE_OK)
        return rc;
    if (vn && (rc = vecnorm_rollout_shape_ok(who, *vn, rows, obs_dim)) != CE_OK) return rc;
    if (!h.was_reset) return bad(CE_ESTATE, " before the first reset()");
    CE_CLEAR_STALE_ERROR();
    const float *obs = obs0;
    for (int s = 0; s < k; ++s) {
        const ce_policy_outputs po = policy_advance(*pout, s * pout_step);
        const O eo = advance(*out, s * out_step);
        policy_launch(p, obs, noise.at(s), rows, po, h.stream);
        if ((rc = Ops::step(e, po.env_action, eo, true)) != CE_OK) return rc;
        obs = eo.obs;
        if (vn) {
            vecnorm_launch(vn->vn, eo.obs, eo.reward, eo.done, vn->obs_slot(s + 1),
                           vn->reward_slot(s), vn->flags, h.stream);
            obs = vn->obs_slot(s + 1);
        }
    }
    CE_HIP(hipGetLastError());
    return CE_OK;
}

}  // namespace ce
