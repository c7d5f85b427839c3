/* Host restatements of log_pos_tab (custom_envs_amd/csrc/optimize_kernels.h)
 * over the generated table (exp2_table.h) and of lr_post4's batched
 * reciprocal beside rcp_newton1 (csrc/optimize_lr_mfma.h).  Every operation
 * the kernels fuse is an explicit fma(); build with -ffp-contract=off.
 * Built and run by tests/test_log_table.py.
 *
 *   tlog log   prints: worst ulp (|log x| >= 0.5)  worst absolute error (below)
 *                      the same two over the forced-index cases alone
 *   tlog rcp   prints: worst ulp of rcp_newton1  worst ulp of the batched form
 *                      1 if every batched result is finite and normal
 *                      worst ulp of the batched form with one Newton step
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "exp2_table.h"

#define TAB CE_EXP2_TAB_SIZE
static const double kTab[TAB] = CE_EXP2_TAB;
static const double kLn2Hi = 6.93147180369123816490e-01, kLn2Lo = 1.90821492927058770002e-10;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rng(void) {                 /* splitmix64 */
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static double uni(void) { return (double)(rng() >> 11) * 0x1p-53; }   /* [0, 1) */

/* The table continued by one entry either way, for the forced indices only:
 * the kernel's own index cannot leave [0, 2047] (the mask). */
static double tab_at(int j) {
    if (j < 0) return 0.5 * kTab[TAB - 1];  /* 2^(-1/2048): halving is exact */
    if (j >= TAB) return 2.0;
    return kTab[j];
}

/* log_pos_tab with the table index moved by `off` (v_log_f32 may put it one
 * off either way; log2f stands for it here) */
static double log_pos_tab(double x, int off) {
    const double kH = kLn2Hi / TAB, kL = kLn2Lo / TAB;
    int ex;
    const double m = frexp(x, &ex);                     /* [1/2, 1) */
    const float lf = log2f((float)m);
    const float sh = fmaf(lf, -(float)(TAB - 1), 0x1.8p23f);
    uint32_t bits;
    memcpy(&bits, &sh, 4);
    const int j = (int)(bits & (TAB - 1)) + off;
    const double z = fma(m, tab_at(j), -1.0);
    const double q = fma(fma(z, -0.25, 1.0 / 3.0), z, -0.5);
    const double lp = fma(z * z, q, z);
    const double n = (double)(ex * TAB - j);
    return fma(n, kH, fma(n, kL, lp));
}

static double worst_ulp, worst_abs;
static void check_log(double x, int off) {
    const long double ref = logl((long double)x);
    const double got = log_pos_tab(x, off);
    const double ar = fabs((double)ref);
    if (ar >= 0.5) {
        const double ulp = nextafter(ar, INFINITY) - ar;
        const double e = (double)(fabsl((long double)got - ref) / ulp);
        if (e > worst_ulp) worst_ulp = e;
    } else {
        const double e = (double)fabsl((long double)got - ref);
        if (e > worst_abs) worst_abs = e;
    }
}

static int run_log(void) {
    const long double span = 256.0L * logl(10.0L);
    for (long i = 0; i < 2000000; ++i) check_log((double)expl(-span * (long double)uni()), 0);
    for (long i = 0; i < 200000; ++i) check_log(1.0 - pow(10.0, -(1.0 + 15.0 * uni())), 0);
    check_log(1.0, 0);
    check_log(1.0 + 16e-16, 0);
    check_log(0.5, 0);
    check_log(1e-256, 0);
    const double all_ulp = worst_ulp, all_abs = worst_abs;
    /* every table boundary 2^(-j/2048), the value itself and its two
     * neighbours, with the index as found and one off either way */
    worst_ulp = worst_abs = 0.0;
    for (int j = 0; j < TAB; ++j) {
        const double b = (j == 0) ? 1.0 : 0.5 * kTab[TAB - j];
        const double xs[3] = {nextafter(b, 0.0), b, nextafter(b, 2.0)};
        for (int k = 0; k < 3; ++k)
            for (int off = -1; off <= 1; ++off) check_log(xs[k], off);
    }
    printf("%.4f %.4e %.4f %.4e\n", all_ulp, all_abs, worst_ulp, worst_abs);
    return 0;
}

/* v_rcp_f64 as profiles/r01_rcp_accuracy.json has it: 1/d within 2^-24
 * relative; here exact 1/d times 1 +- 2^-24 at the ends and random between */
static double rcp_seed(double d) {
    const uint64_t r = rng();
    const double e = (r & 3) == 0 ? 0x1p-24 : (r & 3) == 1 ? -0x1p-24 : (2.0 * uni() - 1.0) * 0x1p-24;
    return (double)((1.0L / (long double)d) * (1.0L + (long double)e));
}
static double rcp_newton1(double d) {
    const double r = rcp_seed(d);
    return fma(r, fma(-d, r, 1.0), r);
}
/* lr_post4 as shipped (order 2): the correction 1 + s of the one seed r0,
 * s = e + e^2 from the residual e = 1 - p r0 (third order: what two Newton
 * steps give), applied to r0 cd and r0 ab, which do not wait for it.
 * Order 1 is the kernel's CE_LR_RCPB_NEWTON=1: rcp_newton1 of the product. */
static void rcp_batched(const double d[4], double inv[4], int order) {
    const double ab = d[0] * d[1], cd = d[2] * d[3];
    const double p = ab * cd;
    double rab, rcd;
    if (order == 1) {
        const double r = rcp_newton1(p);
        rab = r * cd;
        rcd = r * ab;
    } else {
        const double r0 = rcp_seed(p);
        const double e = fma(-p, r0, 1.0);
        const double s = fma(e, e, e);
        const double rab0 = r0 * cd, rcd0 = r0 * ab;
        rab = fma(rab0, s, rab0);
        rcd = fma(rcd0, s, rcd0);
    }
    inv[0] = rab * d[1];
    inv[1] = rab * d[0];
    inv[2] = rcd * d[3];
    inv[3] = rcd * d[2];
}
static double rcp_err(double got, double d) {
    const long double ref = 1.0L / (long double)d;
    const double r = (double)ref;
    const double ulp = r - nextafter(r, 0.0);           /* the smaller neighbour gap at a power of two */
    return (double)(fabsl((long double)got - ref) / ulp);
}

static int run_rcp(void) {
    double ws = 0.0, wb = 0.0, wb1 = 0.0;
    int finite = 1;
    for (long g = 0; g < 1000000; ++g) {
        double d[4], inv[4], inv1[4];
        for (int i = 0; i < 4; ++i) d[i] = exp2(231.0 * uni());   /* log-uniform, magnitudes mixed */
        if (g % 8 == 0)                                           /* the softmax's own: 1 + t */
            for (int i = 0; i < 4; ++i) d[i] = 1.0 + exp2(462.0 * uni() - 231.0);
        if (g % 1000 == 1)                                        /* the top of the range */
            for (int i = 0; i < 4; ++i) d[i] = (rng() & 1) ? 0x1p231 : nextafter(0x1p231, 0.0);
        if (g == 2)
            for (int i = 0; i < 4; ++i) d[i] = 0x1p231;
        rcp_batched(d, inv, 2);
        rcp_batched(d, inv1, 1);
        for (int i = 0; i < 4; ++i) {
            const double s = rcp_newton1(d[i]);
            const double es = rcp_err(s, d[i]), eb = rcp_err(inv[i], d[i]);
            if (es > ws) ws = es;
            const double eb1 = rcp_err(inv1[i], d[i]);
            if (eb > wb) wb = eb;
            if (eb1 > wb1) wb1 = eb1;
            if (!isnormal(inv[i]) || !isnormal(inv1[i])) finite = 0;
        }
    }
    printf("%.4f %.4f %d %.4f\n", ws, wb, finite, wb1);
    return 0;
}

int main(int argc, char **argv) {
    if (argc == 2 && strcmp(argv[1], "log") == 0) return run_log();
    if (argc == 2 && strcmp(argv[1], "rcp") == 0) return run_rcp();
    fprintf(stderr, "usage: tlog log|rcp\n");
    return 2;
}
