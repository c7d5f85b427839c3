// What ce_create decides before it touches the device (engine.hip): which of
// the five kernel families runs a config, under which CE_* switches, with
// which sizes and names.  plan_engine is a pure host function -- no HIP call,
// no allocation that outlives it -- so the selection is testable without a
// GPU (ce_test_plan).
#pragma once

#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "common.h"
#include "mlp_kernels.h"
#include "net_engine.h"
#include "optimize_kernels.h"
#include "optimize_mfma.h"

namespace ce {

enum class Path {
    Register,   // optimize_step_kernel / optimize_pair_kernel: a compiled (T, F, K) instance
    Gen,        // optimize_mfma_kernel / optimize_cat_kernel: any float64 F <= 64, K <= 16
    LrMfma,     // optimize_lr_mfma_kernel and its K-step form: two-class, full batch, float64
    MlpFused,   // mlp_*_kernel: config 3 (F -> 64 -> K, B = 32)
    Net,        // net<...>: every other network (net_engine.hip)
};

using StepFn = void (*)(const void *args, int grid, size_t lds, hipStream_t stream);

struct KernelEntry {
    int precision, F, K;
    StepFn step_staged, step_global, reset;
    StepFn step_pair[2];   // U = 1, 2 (nullptr where the shape has no pair path)
};

// The register-path instance compiled for the shape, or nullptr (engine.hip).
const KernelEntry *find_kernel(int precision, int F, int K);

// The CE_* environment switches, read at every ce_create (tests set
// os.environ between engines).  CE_PERSIST is Host::create's.
struct Switches {
    bool generic = false;     // CE_GENERIC=1: the runtime-shape kernel for every softmax shape
    bool lr_mfma = true;      // CE_LR_MFMA=0: the register kernel for the two-class shapes
    bool pair_u_set = false;  // CE_PAIR_U (any value): no two-class MFMA kernel, and
    int pair_u = 0;           //   its value 0 / 1 / 2 = rows in flight (0: one env per wave)
    bool mlp_net = false;     // CE_MLP_NET=1: the layered path for the fused kernel's shape
    bool mlp_split = false;   // CE_MLP_SPLIT=1 or CE_MLP_PHASES: two launches per step
    int mlp_phases = 3;       // CE_MLP_PHASES=train / info: bit 0 train, bit 1 info (profiling)
    bool no_stage = false;    // CE_NO_STAGE=1: rows from L1 / L2, not the LDS stage
    int lr_waves = 0;         // CE_LR_WAVES: force the two-class MFMA kernel's wave count
    int gen_tail = 1;         // CE_GEN_TAIL=0: the runtime-shape kernel's last feature on MFMA too
    int gen_cat = 1;          // CE_GEN_CAT=0: full batch on the one-env-per-wave kernel
    int lr_mode_cap = 3;      // CE_LR_MODE: cap on the two-class MFMA kernel's row-loop mode
    // ce_step_many: up to 32 steps are plain launches, longer runs a cached
    // hipGraph.  Measured (4096 envs, pair kernel): 20 steps 7.7 us per step
    // direct vs 8.0 graph; 100 and 2000 steps equal.  CE_MANY_DIRECT overrides.
    int many_direct = 32;
};

inline Switches read_switches() {
    Switches s;
    const auto is = [](const char *name, char c) {
        const char *v = std::getenv(name);
        return v && v[0] == c;
    };
    const auto num = [](const char *name, int *out) {
        if (const char *v = std::getenv(name)) *out = std::atoi(v);
    };
    s.generic = is("CE_GENERIC", '1');
    s.lr_mfma = !is("CE_LR_MFMA", '0');
    s.pair_u_set = std::getenv("CE_PAIR_U") != nullptr;
    num("CE_PAIR_U", &s.pair_u);
    s.mlp_net = is("CE_MLP_NET", '1');
    if (const char *ph = std::getenv("CE_MLP_PHASES")) {
        if (std::strcmp(ph, "train") == 0) s.mlp_phases = 1;
        if (std::strcmp(ph, "info") == 0) s.mlp_phases = 2;
        s.mlp_split = true;
    }
    s.mlp_split = s.mlp_split || is("CE_MLP_SPLIT", '1');
    s.no_stage = is("CE_NO_STAGE", '1');
    num("CE_LR_WAVES", &s.lr_waves);
    num("CE_GEN_TAIL", &s.gen_tail);
    num("CE_GEN_CAT", &s.gen_cat);
    num("CE_LR_MODE", &s.lr_mode_cap);
    num("CE_MANY_DIRECT", &s.many_direct);
    return s;
}

struct EnginePlan {
    Path path = Path::Register;
    Switches sw;
    // Register
    const KernelEntry *kern = nullptr;
    StepFn pair = nullptr;    // two-envs-per-wave step kernel, when the shape has one
    int pair_u = 0;           // its rows in flight per lane
    bool staged = false;      // dataset fits the per-block LDS stage
    size_t stage_bytes = 0;
    // MlpFused, Net
    std::vector<int> dims;    // network: F, hidden..., K
    NetGeom geo{};            // Net: the weight-image geometry, W / W0 are [E][Pimg] images
    // every path
    int P = 0, obs_dim = 0;
    size_t tsize = 8;         // element size of W / W0
    size_t gsize = 8;         // element size of G (grad_hist)
    size_t wstride = 0;       // elements of W / W0 per env: P, or geo.Pimg on the Net path
    std::string kernel_name;  // what ce_step_kernel reports
    bool persist = false;     // the K-step kernel (optimize_lr_persist.h) exists for the shape
    std::string many_name;    // what ce_step_many_kernel reports while the K-step kernel is on
};

// The MLP problem: the fused config-3 kernel (mlp_kernels.h: 784 -> 64 -> 10,
// B = 32) where its shape holds; every other network on the layered path
// (net_engine.hip); CE_MLP_NET=1 forces the layered path (tests).
inline int plan_mlp(const ce_config *cfg, const Switches &sw, EnginePlan *p) {
    if (cfg->precision != CE_F32)
        return fail(CE_EUNSUPPORTED, "ce_create: the MLP problem computes in float32");
    if (cfg->n_layers < 0 || cfg->n_layers > kNetMaxHidden)
        return fail(CE_EUNSUPPORTED, "ce_create: the network takes 1 to 4 hidden layers");
    std::vector<int> &dims = p->dims;
    dims.push_back(cfg->n_features);
    if (cfg->n_layers == 0) dims.push_back(cfg->n_hidden);
    for (int l = 0; l < cfg->n_layers; ++l) dims.push_back(cfg->hidden[l]);
    dims.push_back(cfg->n_classes);
    for (int d : dims)
        if (d <= 0) return fail(CE_EINVAL, "ce_create: network widths must be positive");
    const bool fused = !sw.mlp_net && dims.size() == 3 && dims[1] == kMlpHidden &&
                       cfg->batch_size == kMlpBatch && cfg->n_features % 8 == 0 &&
                       cfg->n_classes <= kMlpMaxK && cfg->n_rows % 64 == 0 &&
                       cfg->batch_size < cfg->n_rows;
    p->path = fused ? Path::MlpFused : Path::Net;
    if (fused) {
        p->kernel_name = sw.mlp_split ? "mlp_train_kernel+mlp_info_kernel" : "mlp_step_kernel";
        return CE_OK;
    }
    // the hand-written network kernels' limits (net_engine.h)
    const int rc = net_geometry(static_cast<int>(dims.size()) - 2, dims.data(), &p->geo);
    if (rc != CE_OK) return rc;
    std::string name = "net<";
    for (size_t i = 0; i < dims.size(); ++i) name += (i ? "," : "") + std::to_string(dims[i]);
    // ":mfma": the hand-written MFMA kernels of net_kernels.h; ":wide": a
    // hidden layer wider than 256, the tiled kernels of net_wide.h
    p->kernel_name = name + (p->geo.wide ? ">:wide" : ">:mfma");
    return CE_OK;
}

// The register path's stage and kernel.  Two envs per wave where the shape
// allows it.  U = rows each lane keeps in flight: 2 for float64 (its
// dependent-issue latency, ~10 cycles, needs the second chain at 2 waves per
// SIMD), 1 for float32; measured at 4096 envs.  CE_PAIR_U =
// 0 / 1 / 2 overrides (0 = one env per wave).
inline void plan_register(const ce_config *cfg, const Switches &sw, EnginePlan *p) {
    const bool f64 = cfg->precision == CE_F64;
    p->stage_bytes = stage_bytes_total(cfg->n_features, cfg->n_rows, f64 ? 8 : 4);
    p->staged = p->stage_bytes <= kStageLimit && !sw.no_stage;
    p->pair_u = sw.pair_u_set ? sw.pair_u : f64 ? 2 : 1;
    if (p->staged && (p->pair_u == 1 || p->pair_u == 2)) p->pair = p->kern->step_pair[p->pair_u - 1];
    const std::string args = std::string(f64 ? "double" : "float") + "," + std::to_string(cfg->n_features);
    p->kernel_name = p->pair ? "optimize_pair_kernel<" + args + "," + std::to_string(p->pair_u) + ">"
                             : "optimize_step_kernel<" + args + "," + std::to_string(cfg->n_classes) +
                                   (p->staged ? ",true>" : ",false>");
}

// The softmax problem: the two-class full-batch float64 shapes (the
// benchmark's) run on the MFMA kernel with envs along N (optimize_lr_mfma.h):
// 6.09 us per 4096-env step against 6.3 for the two-envs-per-wave register
// kernel; CE_LR_MFMA=0 (or CE_PAIR_U) selects the register
// kernel instead.  Else a register-path instance when the shape has one
// (unless CE_GENERIC=1 forces the runtime-shape kernel, for tests), else the
// runtime-shape MFMA kernel.
inline int plan_softmax(const ce_config *cfg, const Switches &sw, EnginePlan *p) {
    const int F = cfg->n_features, K = cfg->n_classes, N = cfg->n_rows;
    const bool lr = !sw.generic && sw.lr_mfma && !sw.pair_u_set && cfg->precision == CE_F64 &&
                    cfg->batch_size == N &&
                    cfg->num_envs < (1 << 24) &&   // its packed E | F << 24 argument
                    lr_shape_ok(F, K);
    if (lr) {
        p->path = Path::LrMfma;
        p->kernel_name = lr_kernel_name(cfg->num_envs, N, F, sw.lr_waves, sw.lr_mode_cap);
        p->persist = lr_persist_ok(N);
        if (p->persist) p->many_name = lr_persist_name(N, F);
        return CE_OK;
    }
    if (!sw.generic) p->kern = find_kernel(cfg->precision, F, K);
    if (p->kern) {
        p->path = Path::Register;
        plan_register(cfg, sw, p);
        return CE_OK;
    }
    if (cfg->precision != CE_F64 || F > kGenMaxF || K > kGenMaxClasses)
        return fail(CE_EUNSUPPORTED,
                    "ce_create: no kernel for F=" + std::to_string(F) + " K=" + std::to_string(K) +
                        (cfg->precision != CE_F64
                             ? " in float32 (any F <= 64, K <= 16 runs in float64)"
                             : " (the float64 MFMA kernel takes F <= 64, K <= 16)"));
    p->path = Path::Gen;
    p->kernel_name = gen_kernel_name(cfg->num_envs, N, cfg->batch_size, F, K, sw.gen_cat);
    return CE_OK;
}

// Every check of ce_create, then everything it decides.
inline int plan_engine(const ce_config *cfg, const int32_t *labels, const Switches &sw,
                       EnginePlan *p) {
    if (!cfg || !labels || !p) return fail(CE_EINVAL, "ce_create: null argument");
    *p = EnginePlan{};
    p->sw = sw;
    if (cfg->abi_version != CE_ABI_VERSION)
        return fail(CE_EINVAL, "ce_create: ABI version mismatch");
    if (cfg->problem != CE_PROBLEM_SOFTMAX && cfg->problem != CE_PROBLEM_MLP)
        return fail(CE_EUNSUPPORTED, "ce_create: unknown problem");
    if (cfg->precision != CE_F64 && cfg->precision != CE_F32)
        return fail(CE_EINVAL, "ce_create: unknown precision");
    if (cfg->num_envs <= 0 || cfg->n_rows <= 0 || cfg->n_features <= 0 || cfg->n_classes <= 0)
        return fail(CE_EINVAL, "ce_create: sizes must be positive");
    if (cfg->batch_size <= 0 || cfg->batch_size > cfg->n_rows)
        return fail(CE_EINVAL, "ce_create: batch_size must be in [1, n_rows]");
    if (cfg->max_steps <= 0) return fail(CE_EINVAL, "ce_create: max_steps must be positive");
    const bool mlp = cfg->problem == CE_PROBLEM_MLP;
    const int rc = mlp ? plan_mlp(cfg, sw, p) : plan_softmax(cfg, sw, p);
    if (rc != CE_OK) return rc;
    for (int i = 0; i < cfg->n_rows; ++i)
        if (labels[i] < 0 || labels[i] >= cfg->n_classes)
            return fail(CE_EINVAL, "ce_create: label out of range");
    const int64_t P = !mlp ? int64_t(cfg->n_features) * cfg->n_classes
                           : net_params(cfg->n_features, cfg->n_classes,
                                        static_cast<int>(p->dims.size()) - 2, p->dims.data() + 1);
    if (mlp && P > (int64_t(1) << 30))
        return fail(CE_EUNSUPPORTED, "ce_create: network too large (P > 2^30)");
    p->P = static_cast<int>(P);
    // the MLP problem: float32 weights, a float64 grad history
    p->tsize = mlp || cfg->precision == CE_F32 ? sizeof(float) : sizeof(double);
    p->gsize = mlp ? sizeof(double) : p->tsize;
    p->obs_dim = 2 * p->P + 1;
    // the network path keeps W / W0 as per-env weight images (net_kernels.h),
    // zero-padded; G stays in the flat parameter order
    p->wstride = p->path == Path::Net ? static_cast<size_t>(p->geo.Pimg) : static_cast<size_t>(p->P);
    if (p->many_name.empty()) p->many_name = p->kernel_name;
    return CE_OK;
}

}  // namespace ce
