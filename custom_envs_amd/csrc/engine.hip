// C-ABI implementation of the MI355X Optimize-v0 engine (include/custom_envs_amd.h).
//
// ce_create is plan -> allocate -> upload -> seed.  The plan (engine_plan.h)
// is everything decided from the config and the CE_* switches before any
// device call: which of the five kernel families runs (ce::Path), with which
// instance, sizes and names; every later entry point switches on plan.path.
// The rest is the host's part: own the device copy of the dataset (one image
// per path, built on the host by the *_build_image functions) and the per-env
// state (struct-of-arrays, one contiguous [E][P] slab per quantity so a
// wave's P values are one coalesced segment), stage host actions/outputs
// through pinned buffers (engine_host.h, shared with the other engines), and
// launch one fused step kernel per VecEnv.step.  The env RNG is native
// (seeding.cpp): W0 and the reset permutation are drawn once per seed and
// uploaded, because use_random_state never advances the env RNG
// (custom_envs/utils/utils_math.py:9-22), so every reset replays the same
// draws.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "engine_host.h"
#include "engine_plan.h"   // and through it the kernel headers of every path but the pair kernel's
#include "optimize_pair_kernel.h"
#include "seeding.h"

namespace {

using ce::fail;
using ce::KernelEntry;
using ce::Path;
using ce::StepFn;

template <typename T, int F, int K, bool STAGED>
void launch_step(const void *args, int grid, size_t lds, hipStream_t stream) {
    hipLaunchKernelGGL((ce::optimize_step_kernel<T, F, K, STAGED>), dim3(grid),
                       dim3(ce::kBlock), STAGED ? lds : 0, stream,
                       *static_cast<const ce::StepArgs<T> *>(args));
}

// Two envs per wave (optimize_pair_kernel.h): grid = ceil(E / 16) blocks.
template <typename T, int F, int K, int U>
void launch_pair(const void *args, int, size_t lds, hipStream_t stream) {
    if constexpr (ce::pair_shape(F, K)) {
        const auto &a = *static_cast<const ce::StepArgs<T> *>(args);
        const int grid = (a.E + ce::kPairEnvsPerBlock - 1) / ce::kPairEnvsPerBlock;
        hipLaunchKernelGGL((ce::optimize_pair_kernel<T, F, U>), dim3(grid), dim3(ce::kPairBlock),
                           lds + ce::pair_scratch_bytes<T>(F), stream, a);
    }
}

template <typename T, int F, int K>
void launch_reset(const void *args, int grid, size_t, hipStream_t stream) {
    hipLaunchKernelGGL((ce::optimize_reset_kernel<T, F, K>), dim3(grid), dim3(ce::kBlock), 0,
                       stream, *static_cast<const ce::StepArgs<T> *>(args));
}

// Shapes with a compiled register-path instance.
#define CE_SHAPES(X) \
    X(2, 2) X(4, 2) X(4, 3) X(5, 2) X(8, 2) X(10, 2) X(16, 2) X(20, 2) X(10, 3) X(10, 4) X(3, 3)

#define CE_PAIRS(T, F, K)                                                                   \
    {ce::pair_shape(F, K) ? launch_pair<T, F, K, 1> : nullptr,                              \
     ce::pair_shape(F, K) ? launch_pair<T, F, K, 2> : nullptr}
#define CE_ENTRY(F, K)                                                                \
    {CE_F64, F, K, launch_step<double, F, K, true>, launch_step<double, F, K, false>, \
     launch_reset<double, F, K>, CE_PAIRS(double, F, K)},                             \
    {CE_F32, F, K, launch_step<float, F, K, true>, launch_step<float, F, K, false>,   \
     launch_reset<float, F, K>, CE_PAIRS(float, F, K)},

const KernelEntry kKernels[] = {CE_SHAPES(CE_ENTRY)};

}  // namespace

const KernelEntry *ce::find_kernel(int precision, int F, int K) {
    for (const auto &k : kKernels)
        if (k.precision == precision && k.F == F && k.K == K) return &k;
    return nullptr;
}

struct ce_engine {
    ce_config cfg{};
    ce::EnginePlan plan;          // what ce_create decided (engine_plan.h)
    // stream, staging buffers, step_many bookkeeping; host.compact:
    // ce_set_compact_outputs; host.persist: the persistent K-step kernel
    // (optimize_lr_persist.h) is available for the shape
    ce::Host<ce_outputs> host;
    ce::NetPlan *net = nullptr;   // Path::Net: the layered path's work buffers (net_engine.hip)
    // device state
    void *X = nullptr;            // the path's dataset image
    float *Xs = nullptr;          // MlpFused: the dataset in MFMA operand order (mlp_kernels.h)
    int32_t *label = nullptr;     // MlpFused, Net
    void *W = nullptr, *G = nullptr, *W0 = nullptr;
    double *L = nullptr;
    int32_t *step = nullptr;
    int32_t *perm = nullptr, *order = nullptr, *order_sel = nullptr;
    unsigned long long *diag = nullptr;   // CE_DIAG builds: per-wave phase stamps
};

namespace {

// The register kernels' image, [rows | labels]: row-major rows padded to
// ce::row_stride elements (zeros in the pad), then the int32 labels at the
// next 16-byte boundary, in one buffer staged with one copy.  Two-class
// shapes store s_y x with s_y = +1 (y = 0) / -1 (y = 1) (ce::signed_rows,
// optimize_kernels.h): exact, and it folds the label into the row's dot
// product.
std::vector<unsigned char> register_build_image(int F, int K, int N, size_t tsize,
                                                const double *x, const int32_t *y) {
    const size_t RS = ce::row_stride(F, static_cast<int>(tsize));
    const size_t xbytes = ce::align16(N * RS * tsize);
    const bool sign_fold = ce::signed_rows(F, K);
    std::vector<unsigned char> blob(ce::align16(xbytes + 4 * static_cast<size_t>(N)), 0);
    for (size_t r = 0; r < static_cast<size_t>(N); ++r)
        for (size_t f = 0; f < static_cast<size_t>(F); ++f) {
            const double v = (sign_fold && y[r] != 0) ? -x[r * F + f] : x[r * F + f];
            const float v32 = static_cast<float>(v);
            if (tsize == sizeof(double)) std::memcpy(&blob[(r * RS + f) * 8], &v, 8);
            else std::memcpy(&blob[(r * RS + f) * 4], &v32, 4);
        }
    std::memcpy(&blob[xbytes], y, 4 * static_cast<size_t>(N));
    return blob;
}

// The MLP problem's image: the [N][F] float32 rows, then (the fused kernel
// only) the same rows in MFMA operand order, MlpArgs::Xs (mlp_kernels.h).
std::vector<unsigned char> mlp_build_image(size_t F, size_t N, const double *x, bool operand_copy) {
    std::vector<unsigned char> bytes((operand_copy ? 2 : 1) * N * F * sizeof(float));
    float *x32 = reinterpret_cast<float *>(bytes.data()), *xs = x32 + N * F;
    for (size_t i = 0; i < N * F; ++i) x32[i] = static_cast<float>(x[i]);
    const size_t chunks = F / 8;
    for (size_t t = 0; operand_copy && t < N / 32; ++t)
        for (size_t c = 0; c < chunks; ++c)
            for (size_t l = 0; l < 64; ++l)
                for (size_t j = 0; j < 4; ++j)
                    xs[((t * chunks + c) * 64 + l) * 4 + j] =
                        x32[(32 * t + (l & 31)) * F + 8 * c + 4 * (l >> 5) + j];
    return bytes;
}

// The dataset image of the plan's path, as ce_create uploads it.
std::vector<unsigned char> dataset_image(const ce_config &c, const ce::EnginePlan &p,
                                         const double *x, const int32_t *y) {
    switch (p.path) {
    case Path::Register:
        return register_build_image(c.n_features, c.n_classes, c.n_rows, p.tsize, x, y);
    case Path::Gen:
        return ce::gen_build_image(c.n_features, c.n_rows, x, y);
    case Path::LrMfma: {
        std::vector<unsigned char> bytes(ce::lr_image_doubles(c.n_features, c.n_rows) * sizeof(double));
        ce::lr_build_image(c.n_features, c.n_rows, x, y, reinterpret_cast<double *>(bytes.data()));
        return bytes;
    }
    case Path::MlpFused:
    case Path::Net:
        return mlp_build_image(c.n_features, c.n_rows, x, p.path == Path::MlpFused);
    }
    return {};
}

// The fields StepArgs, MlpArgs and NetArgs share.
template <typename A>
void fill_shared_args(A &a, const ce_engine *e, const float *act, const ce_outputs &o) {
    a.E = e->cfg.num_envs;
    a.N = e->cfg.n_rows;
    a.F = e->cfg.n_features;
    a.K = e->cfg.n_classes;
    a.max_steps = e->cfg.max_steps;
    a.auto_reset = e->cfg.auto_reset;
    a.W = static_cast<decltype(a.W)>(e->W);
    a.G = static_cast<decltype(a.G)>(e->G);
    a.W0 = static_cast<decltype(a.W0)>(e->W0);
    a.L = e->L;
    a.step = e->step;
    a.perm = e->perm;
    a.order = e->order;
    a.order_sel = e->order_sel;
    a.act = act;
    a.obs = o.obs;
    a.reward = o.reward;
    a.done = o.done;
    a.objective = o.objective;
    a.accuracy = o.accuracy;
    a.episode_len = o.episode_len;
}

// compact: the caller's device outputs are in the compact form
// (ce_set_compact_outputs; only the two-class MFMA path writes it)
template <typename T>
ce::StepArgs<T> make_args(const ce_engine *e, const float *act, const ce_outputs &o,
                          bool compact = false) {
    ce::StepArgs<T> a;
    fill_shared_args(a, e, act, o);
    const ce::Switches &sw = e->plan.sw;
    const int P = e->plan.P;
    a.B = e->cfg.batch_size;
    a.data = static_cast<const unsigned char *>(e->X);
    a.diag = e->diag;
    a.inv_B = 1.0 / static_cast<double>(e->cfg.batch_size);
    a.p_mul = (65536 + P - 1) / P;
    a.lr_waves = sw.lr_waves;
    a.gen_tail = sw.gen_tail;
    a.gen_cat = sw.gen_cat;
    a.lr_mode_cap = sw.lr_mode_cap;
    a.obs_stride = compact ? P + 1 : 2 * P + 1;
    a.obs_lo = compact ? P : 0;
    return a;
}

ce::MlpArgs make_mlp_args(const ce_engine *e, const float *act, const ce_outputs &o) {
    ce::MlpArgs a;
    fill_shared_args(a, e, act, o);
    a.P = e->plan.P;
    a.X = static_cast<const float *>(e->X);
    a.Xs = e->Xs;
    a.label = e->label;
    a.diag = e->diag;
    return a;
}

ce::NetArgs make_net_args(const ce_engine *e, const float *act, const ce_outputs &o) {
    ce::NetArgs a{};
    fill_shared_args(a, e, act, o);
    const std::vector<int> &dims = e->plan.dims;
    a.B = e->cfg.batch_size;
    a.P = e->plan.P;
    a.n_hidden = static_cast<int>(dims.size()) - 2;
    for (int l = 0; l < a.n_hidden; ++l) a.hidden[l] = dims[l + 1];
    a.X = static_cast<const float *>(e->X);
    a.label = e->label;
    return a;
}

// One workgroup per env; `even` / `odd`: the kernel's <true> / <false>
// instance (P even: pair accesses aligned in every env).
using MlpKernel = void (*)(ce::MlpArgs);
void launch_mlp(MlpKernel even, MlpKernel odd, const ce::MlpArgs &a, hipStream_t stream) {
    const MlpKernel kernel = (a.P & 1) == 0 ? even : odd;
    hipLaunchKernelGGL(kernel, dim3(a.E), dim3(ce::kMlpBlock), 0, stream, a);
}

int launch(const ce_engine *e, bool reset, const float *act, const ce_outputs &o,
           hipStream_t stream, bool compact = false) {
    const ce::EnginePlan &p = e->plan;
    switch (p.path) {
    case Path::Net: {
        const ce::NetArgs a = make_net_args(e, act, o);
        return reset ? ce::net_reset(e->net, a, stream) : ce::net_step(e->net, a, stream);
    }
    case Path::MlpFused: {
        const ce::MlpArgs a = make_mlp_args(e, act, o);
        if (reset) {
            launch_mlp(ce::mlp_reset_kernel, ce::mlp_reset_kernel, a, stream);
        } else if (!p.sw.mlp_split) {
            launch_mlp(ce::mlp_step_kernel<true>, ce::mlp_step_kernel<false>, a, stream);
        } else {
            if (p.sw.mlp_phases & 1)
                launch_mlp(ce::mlp_train_kernel<true>, ce::mlp_train_kernel<false>, a, stream);
            if (p.sw.mlp_phases & 2)
                launch_mlp(ce::mlp_info_kernel<true>, ce::mlp_info_kernel<false>, a, stream);
        }
        return CE_OK;
    }
    case Path::LrMfma:
    case Path::Gen: {   // compact is never set off the LrMfma path
        const auto a = make_args<double>(e, act, o, compact);
        if (reset) ce::gen_launch_reset(a, stream);
        else if (p.path == Path::LrMfma) ce::lr_launch_step(a, stream);
        else ce::gen_launch_step(a, stream);
        return CE_OK;
    }
    case Path::Register: {
        const StepFn fn = reset ? p.kern->reset
                                : p.pair ? p.pair : p.staged ? p.kern->step_staged : p.kern->step_global;
        const int grid = (e->cfg.num_envs + ce::kWavesPerBlock - 1) / ce::kWavesPerBlock;
        if (e->cfg.precision == CE_F64) {
            const auto a = make_args<double>(e, act, o);
            fn(&a, grid, p.stage_bytes, stream);
        } else {
            const auto a = make_args<float>(e, act, o);
            fn(&a, grid, p.stage_bytes, stream);
        }
        return CE_OK;
    }
    }
    return CE_OK;
}

// what this engine launches (engine_host.h)
struct OptOps {
    static int step(ce_engine *e, const float *act, const ce_outputs &o, bool device_form) {
        return launch(e, false, act, o, e->host.stream, device_form && e->host.compact);
    }
    static int reset(ce_engine *e, const ce_outputs &o, bool device_form) {
        return launch(e, true, nullptr, o, e->host.stream, device_form && e->host.compact);
    }
    // The k steps as ONE launch of the persistent kernel (optimize_lr_persist.h).
    static int persist(ce_engine *e, int k, const float *act, int64_t stride, const ce_outputs &o,
                       int64_t out_step) {
        ce::lr_launch_persist(make_args<double>(e, act, o, e->host.compact), k, stride, out_step,
                              e->host.stream);
        return CE_OK;
    }
    // one policy row per env
    static void policy_shape(const ce_engine *e, int *obs_dim, int *act_dim, int64_t *rows) {
        *obs_dim = e->plan.obs_dim;
        *act_dim = e->plan.P;
        *rows = e->cfg.num_envs;
    }
};

// Host float64 values <-> a device array of `elem`-byte floats (through a
// float32 copy where elem is 4); both wait for the copy.
int upload_typed(ce_engine *e, void *dst, const double *src, size_t count, size_t elem) {
    const std::vector<float> tmp(src, src + (elem == sizeof(float) ? count : 0));
    const void *from = tmp.empty() ? static_cast<const void *>(src) : tmp.data();
    CE_HIP(hipMemcpyAsync(dst, from, count * elem, hipMemcpyHostToDevice, e->host.stream));
    CE_HIP(hipStreamSynchronize(e->host.stream));
    return CE_OK;
}

int download_typed(ce_engine *e, double *dst, const void *src, size_t count, size_t elem) {
    std::vector<float> tmp(elem == sizeof(float) ? count : 0);
    void *to = tmp.empty() ? static_cast<void *>(dst) : tmp.data();
    CE_HIP(hipMemcpyAsync(to, src, count * elem, hipMemcpyDeviceToHost, e->host.stream));
    CE_HIP(hipStreamSynchronize(e->host.stream));
    std::copy(tmp.begin(), tmp.end(), dst);
    return CE_OK;
}

// E flat float32 weight vectors -> the network path's zero-padded images
int upload_net_images(ce_engine *e, void *img, const float *flat) {
    const size_t E = e->cfg.num_envs, P = e->plan.P, PI = e->plan.wstride;
    std::vector<float> tmp(E * PI);
    for (size_t i = 0; i < E; ++i) ce::net_flat_to_image(e->plan.geo, &flat[i * P], &tmp[i * PI]);
    CE_HIP(hipMemcpyAsync(img, tmp.data(), E * PI * sizeof(float), hipMemcpyHostToDevice, e->host.stream));
    CE_HIP(hipStreamSynchronize(e->host.stream));
    return CE_OK;
}

// W or W0 <-> the flat [E][P] float64 vectors of ce_state: the network
// path's weight images, every other path's typed slab
int download_weights(ce_engine *e, double *dst, const void *src) {
    const size_t E = e->cfg.num_envs, P = e->plan.P, PI = e->plan.wstride;
    if (e->plan.path != Path::Net) return download_typed(e, dst, src, E * P, e->plan.tsize);
    std::vector<float> tmp(E * PI), flat(P);
    CE_HIP(hipMemcpyAsync(tmp.data(), src, E * PI * sizeof(float), hipMemcpyDeviceToHost, e->host.stream));
    CE_HIP(hipStreamSynchronize(e->host.stream));
    for (size_t i = 0; i < E; ++i) {
        ce::net_image_to_flat(e->plan.geo, &tmp[i * PI], flat.data());
        for (size_t p = 0; p < P; ++p) dst[i * P + p] = flat[p];
    }
    return CE_OK;
}

int upload_weights(ce_engine *e, void *dst, const double *src) {
    const size_t E = e->cfg.num_envs, P = e->plan.P;
    if (e->plan.path != Path::Net) return upload_typed(e, dst, src, E * P, e->plan.tsize);
    std::vector<float> flat(E * P);
    for (size_t i = 0; i < E * P; ++i) flat[i] = static_cast<float>(src[i]);
    return upload_net_images(e, dst, flat.data());
}

// ce_create's device allocations after host.create, zeroed where a kernel
// reads them before it writes them.  `image_bytes`: the dataset image's.
// A failure returns its status; ce_create tears down.
int allocate_state(ce_engine *e, size_t image_bytes) {
    const ce::EnginePlan &p = e->plan;
    const size_t E = e->cfg.num_envs, N = e->cfg.n_rows, P = p.P;
    const bool mlp = p.path == Path::MlpFused || p.path == Path::Net;
    const size_t xbytes = p.path == Path::MlpFused ? image_bytes / 2 : image_bytes;
    CE_HIP(hipMalloc(&e->X, xbytes));
    if (p.path == Path::MlpFused) CE_HIP(hipMalloc(&e->Xs, xbytes));
    if (mlp) CE_HIP(hipMalloc(&e->label, N * sizeof(int32_t)));
    if (p.path == Path::Gen && ce::gen_set_lds_limits() != CE_OK) return CE_EHIP;
    CE_HIP(hipMalloc(&e->W, E * p.wstride * p.tsize));
    CE_HIP(hipMalloc(&e->G, E * P * p.gsize));
    CE_HIP(hipMalloc(&e->W0, E * p.wstride * p.tsize));
    if (p.path == Path::Net) {   // the images' padding stays zero
        CE_HIP(hipMemset(e->W, 0, E * p.wstride * p.tsize));
        CE_HIP(hipMemset(e->W0, 0, E * p.wstride * p.tsize));
    }
    CE_HIP(hipMalloc(&e->L, E * sizeof(double)));
    CE_HIP(hipMalloc(&e->step, E * sizeof(int32_t)));
    if (e->cfg.batch_size < e->cfg.n_rows) {
        CE_HIP(hipMalloc(&e->perm, E * N * sizeof(int32_t)));
        CE_HIP(hipMalloc(&e->order, 2 * E * N * sizeof(int32_t)));
        CE_HIP(hipMalloc(&e->order_sel, E * sizeof(int32_t)));
        std::vector<int32_t> ident(E * N);
        for (size_t i = 0; i < E; ++i)
            for (size_t r = 0; r < N; ++r) ident[i * N + r] = static_cast<int32_t>(r);
        CE_HIP(hipMemcpy(e->order, ident.data(), E * N * sizeof(int32_t), hipMemcpyHostToDevice));
        CE_HIP(hipMemcpy(e->perm, ident.data(), E * N * sizeof(int32_t), hipMemcpyHostToDevice));
        CE_HIP(hipMemset(e->order_sel, 0, E * sizeof(int32_t)));
    }
#ifdef CE_DIAG
    CE_HIP(hipMalloc(&e->diag, E * ce::kStamps * sizeof(unsigned long long)));
#endif
    CE_HIP(hipMemset(e->G, 0, E * P * p.gsize));
    CE_HIP(hipMemset(e->L, 0, E * sizeof(double)));
    CE_HIP(hipMemset(e->step, 0, E * sizeof(int32_t)));
    return CE_OK;
}

// The dataset image to X (the fused MLP's second half to Xs) and the MLP
// problem's labels.
int upload_dataset(ce_engine *e, const std::vector<unsigned char> &image, const int32_t *labels) {
    const Path path = e->plan.path;
    const size_t xbytes = path == Path::MlpFused ? image.size() / 2 : image.size();
    bool ok = hipMemcpy(e->X, image.data(), xbytes, hipMemcpyHostToDevice) == hipSuccess;
    if (ok && path == Path::MlpFused)
        ok = hipMemcpy(e->Xs, image.data() + xbytes, xbytes, hipMemcpyHostToDevice) == hipSuccess;
    if (ok && (path == Path::MlpFused || path == Path::Net))
        ok = hipMemcpy(e->label, labels, e->cfg.n_rows * sizeof(int32_t), hipMemcpyHostToDevice) ==
             hipSuccess;
    return ok ? CE_OK : fail(CE_EHIP, "ce_create: dataset upload failed");
}

}  // namespace

extern "C" {

int ce_abi_version(void) { return CE_ABI_VERSION; }

const char *ce_last_error(void) { return ce::last_error().c_str(); }

int ce_seed_draws(uint64_t seed, int32_t n_features, int32_t n_classes, int32_t n_rows,
                  double *init_weights, int32_t *perm) {
    if (n_features <= 0 || n_classes <= 0 || n_rows < 0)
        return fail(CE_EINVAL, "ce_seed_draws: bad shape");
    ce::reset_draws(seed, n_features, n_classes, n_rows, init_weights, perm);
    return CE_OK;
}

int ce_seed_draws_mlp(uint64_t seed, int32_t n_features, int32_t n_hidden, int32_t n_classes,
                      int32_t n_rows, float *init_weights, int32_t *perm) {
    if (n_features <= 0 || n_hidden <= 0 || n_classes <= 0 || n_rows < 0)
        return fail(CE_EINVAL, "ce_seed_draws_mlp: bad shape");
    ce::reset_draws_mlp(seed, n_features, n_hidden, n_classes, n_rows, init_weights, perm);
    return CE_OK;
}

int ce_create(const ce_config *cfg, const double *features, const int32_t *labels,
              ce_engine **out) {
    if (!cfg || !features || !labels || !out) return fail(CE_EINVAL, "ce_create: null argument");
    *out = nullptr;
    ce::EnginePlan plan;
    int rc = ce::plan_engine(cfg, labels, ce::read_switches(), &plan);
    if (rc != CE_OK) return rc;
    ce_engine *e = new (std::nothrow) ce_engine();
    if (!e) return fail(CE_ENOMEM, "ce_create: host allocation failed");
    const auto bail = [&](int code) {
        ce_destroy(e);
        return code;
    };
    e->cfg = *cfg;
    e->plan = std::move(plan);
    const ce::EnginePlan &p = e->plan;
    e->host.many_direct = p.sw.many_direct;
    // the strided form and the K-step kernel (which stores the observation
    // block as 16-byte units) take a 16-byte aligned obs only
    e->host.obs_align = 16;
    e->host.persist = p.persist;
    const size_t E = cfg->num_envs;
    rc = e->host.create(cfg->device, E * p.P * sizeof(float),
                        {E * p.obs_dim * sizeof(float), E * sizeof(float), E * sizeof(float),
                         E * sizeof(float), E * sizeof(int32_t), E});
    if (rc != CE_OK) return bail(rc);
    const std::vector<unsigned char> image = dataset_image(*cfg, p, features, labels);
    if ((rc = allocate_state(e, image.size())) != CE_OK) return bail(rc);
    if ((rc = upload_dataset(e, image, labels)) != CE_OK) return bail(rc);
    if (p.path == Path::Net) {
        const ce::NetArgs a = make_net_args(e, nullptr, e->host.region(e->host.d_out));
        if ((rc = ce::net_create(&e->net, a, cfg->device)) != CE_OK) return bail(rc);
    }
    // Unseeded envs behave like np_random(None): os.urandom seeds.  The host
    // side normally seeds explicitly; default to seed = env index here.
    std::vector<uint64_t> seeds(E);
    for (size_t i = 0; i < E; ++i) seeds[i] = i;
    if ((rc = ce_seed(e, seeds.data(), static_cast<int32_t>(E))) != CE_OK) return bail(rc);
    if (hipStreamSynchronize(e->host.stream) != hipSuccess)
        return bail(fail(CE_EHIP, "ce_create: sync failed"));
    *out = e;
    return CE_OK;
}

void ce_destroy(ce_engine *e) {
    if (!e) return;
    e->host.drain();
    ce::net_destroy(e->net);
    e->host.destroy({e->X, e->Xs, e->label, e->W, e->G, e->W0, e->L, e->step, e->perm, e->order,
                     e->order_sel, e->diag});
    delete e;
}

int ce_set_stream(ce_engine *e, void *stream) { return ce::host_set_stream(e, stream); }

int ce_set_compact_outputs(ce_engine *e, int32_t on) {
    if (!e) return fail(CE_EINVAL, "null engine");
    if (on && e->plan.path != Path::LrMfma)
        return fail(CE_EUNSUPPORTED, "ce_set_compact_outputs: only the two-class full-batch "
                                     "float64 kernel (" + std::string("optimize_lr_mfma_kernel") +
                                     ") writes the compact form; this engine runs " +
                                     e->plan.kernel_name);
    if (e->host.compact != (on != 0)) e->host.graphs.release();   // captured launches carry the form
    e->host.compact = on != 0;
    return CE_OK;
}

int ce_num_envs(const ce_engine *e) { return e ? e->cfg.num_envs : CE_EINVAL; }
int ce_obs_dim(const ce_engine *e) { return e ? e->plan.obs_dim : CE_EINVAL; }
int ce_act_dim(const ce_engine *e) { return e ? e->plan.P : CE_EINVAL; }

int ce_seed(ce_engine *e, const uint64_t *seeds, int32_t n) {
    if (!e || !seeds) return fail(CE_EINVAL, "ce_seed: null argument");
    if (n != e->cfg.num_envs) return fail(CE_EINVAL, "ce_seed: need one seed per env");
    const ce::EnginePlan &p = e->plan;
    const size_t E = n, P = p.P, N = e->cfg.n_rows;
    const bool with_perm = e->perm != nullptr;
    const bool mlp = p.path == Path::MlpFused || p.path == Path::Net;
    std::vector<int32_t> perm(with_perm ? E * N : 0);
    std::vector<float> w32(mlp ? E * P : 0);    // the draws, alive until the last copy is done
    std::vector<double> w64(mlp ? 0 : E * P);
    int rc;
    if (mlp) {
        ce::for_each_strided(E, [&](size_t i) {
            ce::reset_draws_net(seeds[i], static_cast<int>(p.dims.size()), p.dims.data(),
                                static_cast<int>(N), &w32[i * P], with_perm ? &perm[i * N] : nullptr);
        });
        if (p.path == Path::Net) {
            if ((rc = upload_net_images(e, e->W0, w32.data())) != CE_OK) return rc;
        } else {
            CE_HIP(hipMemcpyAsync(e->W0, w32.data(), E * P * sizeof(float), hipMemcpyHostToDevice,
                                  e->host.stream));
        }
    } else {
        for (size_t i = 0; i < E; ++i)
            ce::reset_draws(seeds[i], e->cfg.n_features, e->cfg.n_classes, static_cast<int>(N),
                            &w64[i * P], with_perm ? &perm[i * N] : nullptr);
        if ((rc = upload_typed(e, e->W0, w64.data(), E * P, p.tsize)) != CE_OK) return rc;
    }
    if (with_perm)
        CE_HIP(hipMemcpyAsync(e->perm, perm.data(), E * N * sizeof(int32_t),
                              hipMemcpyHostToDevice, e->host.stream));
    CE_HIP(hipStreamSynchronize(e->host.stream));
    return CE_OK;
}

int ce_reset(ce_engine *e, const ce_outputs *out, uint32_t flags) {
    return ce::host_reset<OptOps>(e, out, flags);
}

int ce_step(ce_engine *e, const float *actions, const ce_outputs *out, uint32_t flags) {
    return ce::host_step<OptOps>(e, actions, out, flags, true);
}

int ce_step_async(ce_engine *e, const float *actions, const ce_outputs *out, uint32_t flags) {
    return ce::host_step<OptOps>(e, actions, out, flags, false);
}

int ce_wait(ce_engine *e) { return ce::host_wait(e); }

int ce_step_many(ce_engine *e, int32_t k, const float *actions, int64_t stride,
                 const ce_outputs *out) {
    return ce::host_step_many<OptOps>(e, k, actions, stride, out, true);
}

int ce_step_many_prepare(ce_engine *e, int32_t k, const float *actions, int64_t stride,
                         const ce_outputs *out) {
    return ce::host_step_many<OptOps>(e, k, actions, stride, out, false);
}

int ce_step_many_strided(ce_engine *e, int32_t k, const float *actions, int64_t stride,
                         const ce_outputs *out, int64_t out_step) {
    return ce::host_step_many_strided<OptOps>(e, k, actions, stride, out, out_step);
}

int ce_rollout_policy(ce_engine *e, const ce_policy *p, int32_t k, const float *obs0,
                      const float *noise, int64_t noise_stride, const ce_outputs *out,
                      int64_t out_step, const ce_policy_outputs *pout, int64_t pout_step) {
    return ce::host_rollout_policy<OptOps>("ce_rollout_policy", e, p, k, obs0,
                                           ce::PolicyNoise::block(noise, noise_stride), out,
                                           out_step, pout, pout_step);
}

int ce_rollout_policy_rng(ce_engine *e, const ce_policy *p, int32_t k, const float *obs0,
                          uint64_t seed, uint32_t t0, uint32_t row0, const ce_outputs *out,
                          int64_t out_step, const ce_policy_outputs *pout, int64_t pout_step) {
    return ce::host_rollout_policy<OptOps>("ce_rollout_policy_rng", e, p, k, obs0,
                                           ce::PolicyNoise::rng(seed, t0, row0), out, out_step,
                                           pout, pout_step);
}

int ce_rollout_policy_vecnorm(ce_engine *e, const ce_policy *p, ce_vecnorm *vn, int32_t k,
                              float *obs_norm, int64_t obs_norm_step, float *reward_norm,
                              int64_t reward_norm_step, uint32_t vn_flags,
                              const ce_rollout_noise *noise, const ce_outputs *out,
                              int64_t out_step, const ce_policy_outputs *pout, int64_t pout_step) {
    const char *who = "ce_rollout_policy_vecnorm";
    const int rc = ce::vecnorm_rollout_plain_ok(who, e != nullptr, p, vn, k, obs_norm,
                                                obs_norm_step, reward_norm, reward_norm_step,
                                                vn_flags, noise, out, pout);
    if (rc != CE_OK) return rc;
    const ce::VecnormRollout v{vn, obs_norm, obs_norm_step, reward_norm, reward_norm_step, vn_flags};
    return ce::host_rollout_policy<OptOps>(who, e, p, k, obs_norm, ce::vecnorm_noise(noise), out,
                                           out_step, pout, pout_step, &v);
}

int ce_set_persistent(ce_engine *e, int32_t on) { return ce::host_set_persistent(e, on); }

const char *ce_step_kernel(const ce_engine *e) { return e ? e->plan.kernel_name.c_str() : ""; }

const char *ce_step_many_kernel(const ce_engine *e) {
    if (!e) return "";
    return e->host.persistent() ? e->plan.many_name.c_str() : e->plan.kernel_name.c_str();
}

int64_t ce_stale_error_count(void) { return ce::stale_errors().count.load(); }

const char *ce_stale_error_note(void) {
    static thread_local std::string copy;
    std::lock_guard<std::mutex> lock(ce::stale_errors().mu);
    copy = ce::stale_errors().note;
    return copy.c_str();
}

// Test hook (not part of include/custom_envs_amd.h): record a stale error as
// an entry point would, so the bookkeeping is testable without a GPU.
int ce_test_note_stale_error(int32_t code) {
    ce::note_stale(code, "injected by a test", "ce_test_note_stale_error");
    return CE_OK;
}

// Test hook (not part of include/custom_envs_amd.h): what ce_create would
// decide for this config under the current CE_* switches, without a device.
// Returns plan_engine's status; on CE_OK the names ce_step_kernel and (with
// the K-step kernel on) ce_step_many_kernel would report, in `cap`-byte buffers.
int ce_test_plan(const ce_config *cfg, const int32_t *labels, char *step_name, char *many_name,
                 int32_t cap) {
    ce::EnginePlan plan;
    const int rc = ce::plan_engine(cfg, labels, ce::read_switches(), &plan);
    if (rc != CE_OK) return rc;
    if (step_name && cap > 0) std::snprintf(step_name, cap, "%s", plan.kernel_name.c_str());
    if (many_name && cap > 0) std::snprintf(many_name, cap, "%s", plan.many_name.c_str());
    return CE_OK;
}

// Test hook (not part of include/custom_envs_amd.h): the dataset image
// ce_create would upload for this config (the fused MLP's: the float32 rows,
// then the operand-ordered copy).  Returns its byte count, or plan_engine's
// failed status; writes the image when `out` has room for it.
int64_t ce_test_dataset_image(const ce_config *cfg, const double *features, const int32_t *labels,
                              void *out, int64_t cap) {
    if (!features) return fail(CE_EINVAL, "ce_create: null argument");
    ce::EnginePlan plan;
    const int rc = ce::plan_engine(cfg, labels, ce::read_switches(), &plan);
    if (rc != CE_OK) return rc;
    const std::vector<unsigned char> image = dataset_image(*cfg, plan, features, labels);
    const int64_t bytes = static_cast<int64_t>(image.size());
    if (out && cap >= bytes) std::memcpy(out, image.data(), image.size());
    return bytes;
}

int ce_host_outputs(ce_engine *e, ce_outputs *view) { return ce::host_outputs(e, view); }

#ifdef CE_DIAG
// Diagnostic builds only (not part of include/custom_envs_amd.h).
int ce_diag_stamps(ce_engine *e, unsigned long long *out) {
    if (!e || !out) return fail(CE_EINVAL, "null argument");
    CE_HIP(hipStreamSynchronize(e->host.stream));
    CE_HIP(hipMemcpy(out, e->diag, sizeof(unsigned long long) * e->cfg.num_envs * ce::kStamps,
                     hipMemcpyDeviceToHost));
    return CE_OK;
}
#endif

int ce_get_state(ce_engine *e, const ce_state *st) {
    if (!e || !st) return fail(CE_EINVAL, "null argument");
    const size_t E = e->cfg.num_envs, P = e->plan.P, N = e->cfg.n_rows;
    int rc;
    CE_HIP(hipStreamSynchronize(e->host.stream));
    if (st->weights && (rc = download_weights(e, st->weights, e->W)) != CE_OK) return rc;
    if (st->init_weights && (rc = download_weights(e, st->init_weights, e->W0)) != CE_OK) return rc;
    if (st->grad_hist && (rc = download_typed(e, st->grad_hist, e->G, E * P, e->plan.gsize)) != CE_OK)
        return rc;
    if (st->loss_hist) CE_HIP(hipMemcpy(st->loss_hist, e->L, E * sizeof(double), hipMemcpyDeviceToHost));
    if (st->step) CE_HIP(hipMemcpy(st->step, e->step, E * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (st->order) {
        if (!e->order) return fail(CE_ESTATE, "row order is only tracked when batch_size < n_rows");
        std::vector<int32_t> sel(E), both(2 * E * N);
        CE_HIP(hipMemcpy(sel.data(), e->order_sel, E * sizeof(int32_t), hipMemcpyDeviceToHost));
        CE_HIP(hipMemcpy(both.data(), e->order, 2 * E * N * sizeof(int32_t), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < E; ++i)
            std::memcpy(st->order + i * N, &both[sel[i] * E * N + i * N], N * sizeof(int32_t));
    }
    return CE_OK;
}

int ce_set_state(ce_engine *e, const ce_state *st) {
    if (!e || !st) return fail(CE_EINVAL, "null argument");
    const size_t E = e->cfg.num_envs, P = e->plan.P, N = e->cfg.n_rows;
    int rc;
    CE_HIP(hipStreamSynchronize(e->host.stream));
    if (st->weights && (rc = upload_weights(e, e->W, st->weights)) != CE_OK) return rc;
    if (st->init_weights && (rc = upload_weights(e, e->W0, st->init_weights)) != CE_OK) return rc;
    if (st->grad_hist && (rc = upload_typed(e, e->G, st->grad_hist, E * P, e->plan.gsize)) != CE_OK)
        return rc;
    if (st->loss_hist) CE_HIP(hipMemcpy(e->L, st->loss_hist, E * sizeof(double), hipMemcpyHostToDevice));
    if (st->step) CE_HIP(hipMemcpy(e->step, st->step, E * sizeof(int32_t), hipMemcpyHostToDevice));
    if (st->order) {
        if (!e->order) return fail(CE_ESTATE, "row order is only tracked when batch_size < n_rows");
        CE_HIP(hipMemcpy(e->order, st->order, E * N * sizeof(int32_t), hipMemcpyHostToDevice));
        CE_HIP(hipMemset(e->order_sel, 0, E * sizeof(int32_t)));
    }
    CE_HIP(hipStreamSynchronize(e->host.stream));
    e->host.was_reset = true;
    return CE_OK;
}

}  // extern "C"
