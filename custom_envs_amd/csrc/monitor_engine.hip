// C-ABI implementation of the device-side episode monitor (ce_monitor_* and
// ce_explained_variance in include/custom_envs_amd.h): the carry of
// utils_logging.VecMonitor on the device, the staging area of the last scan and
// the launches [scan, count, block scan, write] on the caller's stream.  Every
// argument check precedes the first HIP call, and the checks of the plain
// arguments precede the check of the handle, so they run without a device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "common.h"
#include "monitor_kernels.h"

static_assert(ce::kMonMaxInfo == CE_MONITOR_MAX_INFO, "the header's column limit");

struct ce_monitor {
    int device = 0, envs = 0;
    ce::MonitorCarry carry{};
    ce::MonitorStage stage{};
    int64_t stage_cap = 0;               // elements of each staging array
    int *block_count = nullptr, *block_off = nullptr;
    int64_t block_cap = 0;
    long long *total = nullptr;          // of the last scan
    unsigned char *mask = nullptr;       // [envs], ce_monitor_reset's
    std::vector<unsigned char> host_mask;
    ce::MonitorRecords last{};           // what ce_monitor_write reads again
    bool scanned = false;
};

namespace {

using ce::fail;

constexpr int64_t kMonMaxFlags = int64_t(1) << 30;

void free_stage(ce_monitor *m) {
    for (void *q : {static_cast<void *>(m->stage.r), static_cast<void *>(m->stage.l),
                    static_cast<void *>(m->stage.cur), static_cast<void *>(m->stage.episode)})
        if (q) (void)hipFree(q);
    m->stage = ce::MonitorStage{};
    m->stage_cap = 0;
}

void free_blocks(ce_monitor *m) {
    if (m->block_count) (void)hipFree(m->block_count);
    if (m->block_off) (void)hipFree(m->block_off);
    m->block_count = m->block_off = nullptr;
    m->block_cap = 0;
}

// the staging area for `flags` = k * envs flags: grows as needed; the steady
// state allocates nothing
int reserve(ce_monitor *m, int64_t flags) {
    if (flags > m->stage_cap) {
        free_stage(m);                   // hipFree waits for the launches that read it
        const size_t n = static_cast<size_t>(flags);
        CE_HIP(hipMalloc(&m->stage.r, n * sizeof(double)));
        CE_HIP(hipMalloc(&m->stage.l, n * sizeof(int)));
        CE_HIP(hipMalloc(&m->stage.cur, n * sizeof(float)));
        CE_HIP(hipMalloc(&m->stage.episode, n * sizeof(long long)));
        m->stage_cap = flags;
    }
    const int64_t nb = (flags + ce::kMonBlock - 1) / ce::kMonBlock;
    if (nb > m->block_cap) {
        free_blocks(m);
        CE_HIP(hipMalloc(&m->block_count, static_cast<size_t>(nb) * sizeof(int)));
        CE_HIP(hipMalloc(&m->block_off, static_cast<size_t>(nb) * sizeof(int)));
        m->block_cap = nb;
    }
    return CE_OK;
}

int out_ok(const char *who, const void *out, int64_t capacity) {
    const auto bad = [who](const std::string &what) { return fail(CE_EINVAL, who + what); };
    if (capacity < 0) return bad(": capacity must not be negative");
    if (capacity > 0 && !out) return bad(": null output buffer");
    if (reinterpret_cast<uintptr_t>(out) & 7) return bad(": the output buffer must be 8-byte aligned");
    return CE_OK;
}

void enqueue_write(const ce_monitor *m, void *out, int64_t capacity, hipStream_t stream) {
    const ce::MonitorRecords &q = m->last;
    const unsigned nb = static_cast<unsigned>((int64_t(q.k) * q.envs + ce::kMonBlock - 1) / ce::kMonBlock);
    hipLaunchKernelGGL(ce::monitor_write_kernel, dim3(nb), dim3(ce::kMonBlock), 0, stream, q,
                       m->stage, m->block_off, static_cast<char *>(out),
                       static_cast<long long>(capacity),
                       static_cast<int>(ce_monitor_record_bytes(q.n_info)));
}

}  // namespace

extern "C" {

int64_t ce_monitor_record_bytes(int32_t n_info) {
    if (n_info < 0 || n_info > CE_MONITOR_MAX_INFO) return -1;
    return ce::kMonRecordHead + 8 * ((n_info + 1) / 2);
}

int ce_monitor_create(int32_t device, int32_t num_envs, ce_monitor **out) {
    if (!out) return fail(CE_EINVAL, "ce_monitor_create: null output handle");
    *out = nullptr;
    if (device < 0) return fail(CE_EINVAL, "ce_monitor_create: device must not be negative");
    if (num_envs < 1 || num_envs > (1 << 24))
        return fail(CE_EINVAL, "ce_monitor_create: num_envs must be in [1, 2^24], got " +
                                   std::to_string(num_envs));
    ce_monitor *m = new (std::nothrow) ce_monitor();
    if (!m) return fail(CE_ENOMEM, "ce_monitor_create: out of host memory");
    m->device = device;
    m->envs = num_envs;
    const auto bail = [m](int code) {
        ce_monitor_destroy(m);
        return code;
    };
    CE_CLEAR_STALE_ERROR();
    const size_t n = static_cast<size_t>(num_envs);
    CE_TRY(hipSetDevice(device));
    CE_TRY(hipMalloc(&m->carry.ep_reward, n * sizeof(double)));
    CE_TRY(hipMalloc(&m->carry.ep_len, n * sizeof(int)));
    CE_TRY(hipMalloc(&m->carry.episode, n * sizeof(long long)));
    CE_TRY(hipMalloc(&m->carry.total_steps, n * sizeof(long long)));
    CE_TRY(hipMalloc(&m->total, sizeof(long long)));
    CE_TRY(hipMalloc(&m->mask, n));
    CE_TRY(hipMemset(m->carry.ep_reward, 0, n * sizeof(double)));
    CE_TRY(hipMemset(m->carry.ep_len, 0, n * sizeof(int)));
    CE_TRY(hipMemset(m->carry.episode, 0, n * sizeof(long long)));
    CE_TRY(hipMemset(m->carry.total_steps, 0, n * sizeof(long long)));
    CE_TRY(hipMemset(m->total, 0, sizeof(long long)));
    CE_TRY(hipDeviceSynchronize());
    m->host_mask.resize(n);
    *out = m;
    return CE_OK;
}

void ce_monitor_destroy(ce_monitor *m) {
    if (!m) return;
    free_stage(m);
    free_blocks(m);
    for (void *q : {static_cast<void *>(m->carry.ep_reward), static_cast<void *>(m->carry.ep_len),
                    static_cast<void *>(m->carry.episode), static_cast<void *>(m->carry.total_steps),
                    static_cast<void *>(m->total), static_cast<void *>(m->mask)})
        if (q) (void)hipFree(q);
    delete m;
}

int ce_monitor_reset(ce_monitor *m, const int32_t *indices, int32_t n, void *hip_stream) {
    const char *who = "ce_monitor_reset";
    const auto bad = [who](const std::string &what) { return fail(CE_EINVAL, who + what); };
    if (indices && n < 0) return bad(": n must not be negative");
    if (!m) return bad(": null monitor");
    if (indices)
        for (int32_t i = 0; i < n; ++i)
            if (indices[i] < 0 || indices[i] >= m->envs)
                return bad(": index " + std::to_string(indices[i]) + " is outside [0, " +
                           std::to_string(m->envs) + ")");
    CE_CLEAR_STALE_ERROR();
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const unsigned char *mask = nullptr;
    if (indices) {
        if (n == 0) return CE_OK;
        std::fill(m->host_mask.begin(), m->host_mask.end(), 0);
        for (int32_t i = 0; i < n; ++i) m->host_mask[indices[i]] = 1;
        CE_HIP(hipMemcpyAsync(m->mask, m->host_mask.data(), m->host_mask.size(),
                              hipMemcpyHostToDevice, stream));
        CE_HIP(hipStreamSynchronize(stream));      // host_mask is pageable and reused
        mask = m->mask;
    }
    hipLaunchKernelGGL(ce::monitor_reset_kernel,
                       dim3(static_cast<unsigned>((m->envs + ce::kMonBlock - 1) / ce::kMonBlock)),
                       dim3(ce::kMonBlock), 0, stream, m->envs, mask, m->carry);
    CE_HIP(hipGetLastError());
    return CE_OK;
}

int ce_monitor_scan(ce_monitor *m, int32_t k, int32_t num_envs, int32_t row_stride,
                    const float *rewards, int64_t reward_stride_bytes, const uint8_t *dones,
                    int64_t done_stride_bytes, const ce_monitor_column *columns, int32_t n_info,
                    void *out, int64_t capacity, int64_t *total, void *hip_stream) {
    const char *who = "ce_monitor_scan";
    const auto bad = [who](const std::string &what) { return fail(CE_EINVAL, who + what); };
    if (k < 1) return bad(": k must be at least 1, got " + std::to_string(k));
    if (num_envs < 1 || num_envs > (1 << 24))
        return bad(": num_envs must be in [1, 2^24], got " + std::to_string(num_envs));
    if (int64_t(k) * num_envs > kMonMaxFlags)
        return bad(": k * num_envs must be at most 2^30, got " + std::to_string(int64_t(k) * num_envs));
    if (row_stride < 1 || row_stride > (1 << 16))
        return bad(": row_stride must be in [1, 2^16], got " + std::to_string(row_stride));
    const int64_t rows = int64_t(num_envs) * row_stride;
    if (!rewards) return bad(": null rewards");
    if (!dones) return bad(": null dones");
    if (reinterpret_cast<uintptr_t>(rewards) & 3) return bad(": rewards must be 4-byte aligned");
    if (reward_stride_bytes < rows * 4 || reward_stride_bytes % 4 != 0)
        return bad(": reward_stride_bytes must be a multiple of 4 of at least num_envs * row_stride * 4");
    if (done_stride_bytes < rows) return bad(": done_stride_bytes must be at least num_envs * row_stride");
    if (n_info < 0 || n_info > CE_MONITOR_MAX_INFO)
        return bad(": n_info must be in [0, " + std::to_string(CE_MONITOR_MAX_INFO) + "], got " +
                   std::to_string(n_info));
    if (n_info > 0 && !columns) return bad(": null columns");
    for (int32_t c = 0; c < n_info; ++c) {
        const ce_monitor_column &col = columns[c];
        const std::string name = ": column " + std::to_string(c);
        if (!col.base) return bad(name + " has a null base");
        if (reinterpret_cast<uintptr_t>(col.base) & 3) return bad(name + " must be 4-byte aligned");
        if (col.row_floats < 1 || col.row_floats > (1 << 16))
            return bad(name + ": row_floats must be in [1, 2^16]");
        if (col.col < 0 || col.col >= col.row_floats)
            return bad(name + ": col must be in [0, row_floats)");
        if (col.stride_bytes % 4 != 0 || col.stride_bytes < int64_t(num_envs) * col.row_floats * 4)
            return bad(name + ": stride_bytes must be a multiple of 4 of at least num_envs * "
                              "row_floats * 4");
    }
    int rc = out_ok(who, out, capacity);
    if (rc != CE_OK) return rc;
    if (!total) return bad(": null total");
    if (reinterpret_cast<uintptr_t>(total) & 7) return bad(": total must be 8-byte aligned");
    if (!m) return bad(": null monitor");
    if (num_envs != m->envs)
        return bad(": the monitor holds " + std::to_string(m->envs) + " envs, got " +
                   std::to_string(num_envs));
    CE_CLEAR_STALE_ERROR();
    const int64_t flags = int64_t(k) * num_envs;
    if ((rc = reserve(m, flags)) != CE_OK) return rc;
    ce::MonitorRecords q{};
    q.k = k;
    q.envs = num_envs;
    q.row_stride = row_stride;
    q.n_info = n_info;
    q.reward = reinterpret_cast<const char *>(rewards);
    q.reward_stride = reward_stride_bytes;
    q.done = dones;
    q.done_stride = done_stride_bytes;
    for (int32_t c = 0; c < n_info; ++c)
        q.info[c] = ce::MonitorColumn{static_cast<const char *>(columns[c].base),
                                      static_cast<long long>(columns[c].stride_bytes),
                                      columns[c].row_floats, columns[c].col};
    m->last = q;
    m->scanned = true;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const unsigned nb = static_cast<unsigned>((flags + ce::kMonBlock - 1) / ce::kMonBlock);
    hipLaunchKernelGGL(ce::monitor_scan_kernel,
                       dim3(static_cast<unsigned>((num_envs + ce::kMonBlock - 1) / ce::kMonBlock)),
                       dim3(ce::kMonBlock), 0, stream, q, m->carry, m->stage);
    hipLaunchKernelGGL(ce::monitor_count_kernel, dim3(nb), dim3(ce::kMonBlock), 0, stream, q,
                       m->block_count);
    hipLaunchKernelGGL(ce::monitor_blockscan_kernel, dim3(1), dim3(ce::kMonBlock), 0, stream,
                       static_cast<int>(nb), m->block_count, m->block_off, m->total,
                       reinterpret_cast<long long *>(total));
    enqueue_write(m, out, capacity, stream);
    CE_HIP(hipGetLastError());
    return CE_OK;
}

int ce_monitor_write(ce_monitor *m, void *out, int64_t capacity, void *hip_stream) {
    const char *who = "ce_monitor_write";
    const int rc = out_ok(who, out, capacity);
    if (rc != CE_OK) return rc;
    if (!m) return fail(CE_EINVAL, std::string(who) + ": null monitor");
    if (!m->scanned) return fail(CE_ESTATE, std::string(who) + ": no scan to write the records of");
    CE_CLEAR_STALE_ERROR();
    enqueue_write(m, out, capacity, static_cast<hipStream_t>(hip_stream));
    CE_HIP(hipGetLastError());
    return CE_OK;
}

static int state_copy(const char *who, ce_monitor *m, void *ep_reward, void *ep_len, void *episode,
                      void *total_steps, bool set, void *hip_stream) {
    const auto bad = [who](const std::string &what) { return fail(CE_EINVAL, who + what); };
    if (!ep_reward) return bad(": null ep_reward");
    if (!ep_len) return bad(": null ep_len");
    if (!episode) return bad(": null episode");
    if (!total_steps) return bad(": null total_steps");
    if (!m) return bad(": null monitor");
    CE_CLEAR_STALE_ERROR_AT(who);
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    const size_t n = static_cast<size_t>(m->envs);
    struct Block { void *dev, *host; size_t bytes; };
    const Block blocks[] = {{m->carry.ep_reward, ep_reward, n * sizeof(double)},
                            {m->carry.ep_len, ep_len, n * sizeof(int)},
                            {m->carry.episode, episode, n * sizeof(long long)},
                            {m->carry.total_steps, total_steps, n * sizeof(long long)}};
    for (const Block &b : blocks) {
        if (set)
            CE_HIP(hipMemcpyAsync(b.dev, b.host, b.bytes, hipMemcpyHostToDevice, stream));
        else
            CE_HIP(hipMemcpyAsync(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost, stream));
    }
    CE_HIP(hipStreamSynchronize(stream));     // the host blocks may be pageable
    return CE_OK;
}

int ce_monitor_get_state(ce_monitor *m, double *ep_reward, int32_t *ep_len, int64_t *episode,
                         int64_t *total_steps, void *hip_stream) {
    return state_copy("ce_monitor_get_state", m, ep_reward, ep_len, episode, total_steps, false,
                      hip_stream);
}

int ce_monitor_set_state(ce_monitor *m, const double *ep_reward, const int32_t *ep_len,
                         const int64_t *episode, const int64_t *total_steps, void *hip_stream) {
    return state_copy("ce_monitor_set_state", m, const_cast<double *>(ep_reward),
                      const_cast<int32_t *>(ep_len), const_cast<int64_t *>(episode),
                      const_cast<int64_t *>(total_steps), true, hip_stream);
}

int ce_explained_variance(int32_t k, int64_t rows, const float *values, int64_t value_stride_bytes,
                          const float *returns, double *out, void *hip_stream) {
    const char *who = "ce_explained_variance";
    const auto bad = [who](const std::string &what) { return fail(CE_EINVAL, who + what); };
    if (k < 1) return bad(": k must be at least 1, got " + std::to_string(k));
    if (rows < 1 || rows > (int64_t(1) << 24))
        return bad(": rows must be in [1, 2^24], got " + std::to_string(rows));
    if (int64_t(k) * rows > kMonMaxFlags)
        return bad(": k * rows must be at most 2^30, got " + std::to_string(int64_t(k) * rows));
    if (!values) return bad(": null values");
    if (!returns) return bad(": null returns");
    if (!out) return bad(": null output");
    if ((reinterpret_cast<uintptr_t>(values) | reinterpret_cast<uintptr_t>(returns)) & 3)
        return bad(": values and returns must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(out) & 7) return bad(": the output must be 8-byte aligned");
    if (value_stride_bytes < rows * 4 || value_stride_bytes % 4 != 0)
        return bad(": value_stride_bytes must be a multiple of 4 of at least rows * 4");
    CE_CLEAR_STALE_ERROR();
    hipLaunchKernelGGL(ce::monitor_ev_kernel, dim3(1), dim3(ce::kMonBlock), 0,
                       static_cast<hipStream_t>(hip_stream), k, static_cast<int>(rows),
                       reinterpret_cast<const char *>(values),
                       static_cast<long long>(value_stride_bytes), returns, out);
    CE_HIP(hipGetLastError());
    return CE_OK;
}

}  // extern "C"
