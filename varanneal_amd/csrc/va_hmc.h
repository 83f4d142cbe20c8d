// va_hmc.h -- sample exp(-A(X, p)) on the device: B Hamiltonian Monte Carlo chains around the batched evaluation.
//
// After anneal() everything the package says about an estimate is local and Gaussian (va_hvp.h, va_selinv.h,
// va_predict_tlm.h).  This samples the distribution itself at one rung of the ladder: one chain per resident path, the
// potential the action as the package normalises it, its gradient from the handle's own evaluation kernel (whatever that
// is: run_eval, va_capi.hip), so every model the evaluators carry can be sampled.  A trajectory is n_leap evaluations with
// one element-wise kernel between two of them; the path never leaves the device.
//
// The arithmetic is written once as __host__ __device__ phases of ONE LANE (the pattern of va_predict.h): the kernels
// k_hmc<PHASE> give them their parallel decomposition (va_hmc_geo.h), hmc_host drives the same phases lane by lane on the
// CPU (tests/cpu_emul/hmc_check.cpp).  Every element-wise expression is evaluated as written, products and sums rounded
// one by one (fp contraction off), so a NumPy transcription reproduces its bits (tests/_hmc_ref.py).
//
//   generator  Philox4x32-10, key = the caller's 64-bit seed, counter = (chain, iteration, element, stream): a draw
//              depends on nothing else -- not on the geometry, not on how many chains share a call.  Stream 0, words 0 and
//              1 of element i: the normal z_i by Box-Muller, u = (word + 1) 2^-32 in (0, 1], z = sqrt(-2 log u1) cos(2 pi u2).
//              Stream 1, element 0: word 0 the accept uniform, word 1 the step jitter's.  Or the caller's own numbers (noise).
//   begin      p = z / sqrt(minv);  restore point xs = x, gs = g;  K0 = 1/2 sum (p p) minv;
//              eps_it = eps_b (1 + jitter (2 u_jit - 1));  first step: p -= (eps_it / 2) g,  x += (eps_it minv) p
//   mid        p -= eps_it g,  x += (eps_it minv) p                      (n_leap - 1 times, an evaluation before each)
//   end        p -= (eps_it / 2) g  after the last evaluation;  K1 = 1/2 sum (p p) minv
//   commit     dH = (A1 + K1) - (A0 + K0);  accept iff dH is finite and log(u_acc) < -dH;  on rejection x, g are restored
//              from xs, gs (a NaN never survives an iteration);  Welford update of every variable's mean and sum of squared
//              deviations;  the kept columns of every thin-th iteration;  the traces
// Sums: a lane adds its elements in order, the workgroup's lanes by a binary tree over the lane index, a chain's
// workgroups in order, recomputed by every workgroup of the chain in commit -- no atomics, the same bits on every call.
// The current action sits in A_cur[parity of the iteration][chain]: commit reads one parity and writes the other, so no
// workgroup of a chain can see the word another one has already replaced.
// Box bounds: va_hmc refuses a bounded handle; va_hmc_box.h runs these phases' arithmetic on an unconstrained z with x = T(z).
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "va_core.h"
#include "va_hmc_geo.h"

namespace va {

enum { HMC_BEGIN = 0, HMC_MID = 1, HMC_END = 2, HMC_COMMIT = 3 };

struct HmcArgs {
    double *x, *g;                 // [B][ld]: the chains' paths; the finished gradient of the last evaluation at them
    double *p, *xs, *gs;           // [B][ld]: momentum; restore point of the iteration
    const double *minv, *sminv;    // inverse mass and its square root: [n_var] (minv_stride 0) or [B][n_var] (minv_stride n_var)
    long minv_stride;
    const double *eps;             // [B]
    double jitter;
    const double *noise;           // NULL: the generator; or [n_iter][B][n_var + 2]: normals, accept uniform, jitter uniform
    uint32_t k0, k1;               // the seed's low and high word
    uint32_t chain0;               // counter of chain 0 of this call
    const double *A_eval;          // [B] the action of the last evaluation
    double *A_cur;                 // [2][B]
    double *part;                  // [2][B * nwg] partial kinetic sums of begin / end
    double *mean, *m2;             // [B][n_var]
    double *A_trace, *dH;          // [B][n_iter]
    int32_t *accepted;             // [B][n_iter]
    double *kept;                  // [B][n_iter / thin][n_keep]
    const int64_t *keep_idx;       // [n_keep]
    long n_keep, ld, n_var;
    int B, n_iter, it, thin;
    HmcGeo geo;
};

// ---------------------------------------------------------------- generator
VA_HD void hmc_philox(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t *out)
{
    for (int r = 0; r < 10; ++r) {
        const uint64_t m0 = (uint64_t)0xD2511F53u * c0, m1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(m1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)m1, n2 = (uint32_t)(m0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)m0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

VA_HD double hmc_u01(uint32_t w)      // (0, 1]: exact in binary64
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return ((double)w + 1.0) * 2.3283064365386962890625e-10;
}

VA_HD double hmc_box_muller(uint32_t w0, uint32_t w1)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double u1 = hmc_u01(w0), u2 = hmc_u01(w1);
    const double r = sqrt(-2.0 * log(u1));
    const double c = cos(6.283185307179586 * u2);
    return r * c;
}

// element i's normal of (chain b, iteration it)
VA_HD double hmc_normal(const HmcArgs &a, int b, int it, long i)
{
    if (a.noise) return a.noise[((size_t)it * a.B + b) * (size_t)(a.n_var + 2) + i];
    uint32_t w[4];
    hmc_philox(a.k0, a.k1, a.chain0 + (uint32_t)b, (uint32_t)it, (uint32_t)i, 0u, w);
    return hmc_box_muller(w[0], w[1]);
}
// the accept uniform and the jitter uniform of (chain b, iteration it)
VA_HD void hmc_uniforms(const HmcArgs &a, int b, int it, double &u_acc, double &u_jit)
{
    if (a.noise) {
        const double *n = a.noise + ((size_t)it * a.B + b) * (size_t)(a.n_var + 2) + a.n_var;
        u_acc = n[0]; u_jit = n[1];
        return;
    }
    uint32_t w[4];
    hmc_philox(a.k0, a.k1, a.chain0 + (uint32_t)b, (uint32_t)it, 0u, 1u, w);
    u_acc = hmc_u01(w[0]); u_jit = hmc_u01(w[1]);
}

VA_HD double hmc_eps_it(const HmcArgs &a, int b, int it)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double u_acc, u_jit;
    hmc_uniforms(a, b, it, u_acc, u_jit);
    const double s = 2.0 * u_jit - 1.0;
    const double f = 1.0 + a.jitter * s;
    return a.eps[b] * f;
}

VA_HD bool hmc_finite(double v) { return v - v == 0.0; }

// ---------------------------------------------------------------- phases of one lane
// begin: momentum, restore point, first half kick and drift; returns the lane's share of sum (p p) minv
VA_HD double hmc_begin_lane(const HmcArgs &a, long wg, int tid)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int b = (int)(wg / a.geo.nwg);
    const long w = wg % a.geo.nwg;
    const size_t row = (size_t)b * a.ld;
    const double eps = hmc_eps_it(a, b, a.it), half = 0.5 * eps;
    double ks = 0.0;
    for (int e = 0; e < HMC_EPT; ++e) {
        const long i = hmc_element(a.n_var, w, tid, e);
        if (i < 0) continue;
        const double mi = a.minv[(size_t)b * a.minv_stride + i], smi = a.sminv[(size_t)b * a.minv_stride + i];
        const double xv = a.x[row + i], gv = a.g[row + i];
        double pv = hmc_normal(a, b, a.it, i) / smi;
        a.xs[row + i] = xv; a.gs[row + i] = gv;
        const double pp = pv * pv;
        ks = ks + pp * mi;
        pv = pv - half * gv;
        const double c = eps * mi;
        a.p[row + i] = pv;
        a.x[row + i] = xv + c * pv;
    }
    return ks;
}

VA_HD void hmc_mid_lane(const HmcArgs &a, long wg, int tid)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int b = (int)(wg / a.geo.nwg);
    const long w = wg % a.geo.nwg;
    const size_t row = (size_t)b * a.ld;
    const double eps = hmc_eps_it(a, b, a.it);
    for (int e = 0; e < HMC_EPT; ++e) {
        const long i = hmc_element(a.n_var, w, tid, e);
        if (i < 0) continue;
        const double mi = a.minv[(size_t)b * a.minv_stride + i];
        const double pv = a.p[row + i] - eps * a.g[row + i];
        const double c = eps * mi;
        a.p[row + i] = pv;
        a.x[row + i] = a.x[row + i] + c * pv;
    }
}

// end: last half kick; returns the lane's share of sum (p p) minv
VA_HD double hmc_end_lane(const HmcArgs &a, long wg, int tid)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int b = (int)(wg / a.geo.nwg);
    const long w = wg % a.geo.nwg;
    const size_t row = (size_t)b * a.ld;
    const double half = 0.5 * hmc_eps_it(a, b, a.it);
    double ks = 0.0;
    for (int e = 0; e < HMC_EPT; ++e) {
        const long i = hmc_element(a.n_var, w, tid, e);
        if (i < 0) continue;
        const double pv = a.p[row + i] - half * a.g[row + i];
        a.p[row + i] = pv;
        const double pp = pv * pv;
        ks = ks + pp * a.minv[(size_t)b * a.minv_stride + i];
    }
    return ks;
}

// the decision of (chain b, iteration a.it), from the partial sums in workgroup order: the same bits whoever calls it
VA_HD bool hmc_decide(const HmcArgs &a, int b, double &dH, double &A_new)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double *p0 = a.part + (size_t)b * a.geo.nwg, *p1 = a.part + (size_t)a.geo.grid + (size_t)b * a.geo.nwg;
    double s0 = 0.0, s1 = 0.0;
    for (long w = 0; w < a.geo.nwg; ++w) { s0 = s0 + p0[w]; s1 = s1 + p1[w]; }
    const double K0 = 0.5 * s0, K1 = 0.5 * s1;
    const double A0 = a.A_cur[(size_t)(a.it & 1) * a.B + b], A1 = a.A_eval[b];
    dH = (A1 + K1) - (A0 + K0);
    double u_acc, u_jit;
    hmc_uniforms(a, b, a.it, u_acc, u_jit);
    const bool acc = hmc_finite(dH) && log(u_acc) < -dH;
    A_new = acc ? A1 : A0;
    return acc;
}

// commit: select, restore, statistics, kept columns, traces
VA_HD void hmc_commit_lane(const HmcArgs &a, long wg, int tid, bool acc, double dH, double A_new)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const int b = (int)(wg / a.geo.nwg);
    const long w = wg % a.geo.nwg;
    const size_t row = (size_t)b * a.ld, srow = (size_t)b * a.n_var;
    const double n = (double)(a.it + 1);
    for (int e = 0; e < HMC_EPT; ++e) {
        const long i = hmc_element(a.n_var, w, tid, e);
        if (i < 0) continue;
        double xv = a.x[row + i];
        if (!acc) {
            xv = a.xs[row + i];
            a.x[row + i] = xv;
            a.g[row + i] = a.gs[row + i];
        }
        const double m = a.mean[srow + i];
        const double d = xv - m;
        const double mn = m + d / n;
        a.mean[srow + i] = mn;
        a.m2[srow + i] = a.m2[srow + i] + d * (xv - mn);
    }
    if (w != 0) return;
    // (chunk 0 of the chain.  The kept columns are read where the decision says the state is: xs is not written in this
    // phase, and x of an accepted iteration is not either)
    if (a.n_keep > 0 && (a.it + 1) % a.thin == 0) {
        const double *src = (acc ? a.x : a.xs) + row;
        double *dst = a.kept + ((size_t)b * (a.n_iter / a.thin) + (size_t)((a.it + 1) / a.thin - 1)) * a.n_keep;
        for (long k = tid; k < a.n_keep; k += HMC_THREADS) dst[k] = src[a.keep_idx[k]];
    }
    if (tid == 0) {
        const size_t t = (size_t)b * a.n_iter + a.it;
        a.A_trace[t] = A_new; a.dH[t] = dH; a.accepted[t] = acc ? 1 : 0;
        a.A_cur[(size_t)((a.it + 1) & 1) * a.B + b] = A_new;
    }
}

// the lanes' sums of one workgroup, added by a binary tree over the lane index (what the kernel does through LDS)
inline double hmc_tree_host(std::vector<double> &v)
{
    for (int s = HMC_THREADS / 2; s >= 1; s >>= 1)
        for (int t = 0; t < s; ++t) v[t] = v[t] + v[t + s];
    return v[0];
}

// ---------------------------------------------------------------- the same phases, lane by lane on the host
// Every pointer of `a` is host memory; a.geo from plan_hmc; A_cur[0][b], x and g hold the start point's action, path and
// gradient.  eval(): the action and gradient at a.x into a.A_eval and a.g, called n_leap times per iteration.
// after(it): called after each iteration's commit (a test reads its traces there).
template <class EVAL, class AFTER>
inline void hmc_host(HmcArgs a, int n_leap, EVAL &&eval, AFTER &&after)
{
    std::vector<double> lane(HMC_THREADS);
    for (int it = 0; it < a.n_iter; ++it) {
        a.it = it;
        for (long wg = 0; wg < a.geo.grid; ++wg) {
            for (int t = 0; t < HMC_THREADS; ++t) lane[t] = hmc_begin_lane(a, wg, t);
            a.part[wg] = hmc_tree_host(lane);
        }
        for (int l = 0; l < n_leap; ++l) {
            if (l)
                for (long wg = 0; wg < a.geo.grid; ++wg)
                    for (int t = 0; t < HMC_THREADS; ++t) hmc_mid_lane(a, wg, t);
            eval();
        }
        for (long wg = 0; wg < a.geo.grid; ++wg) {
            for (int t = 0; t < HMC_THREADS; ++t) lane[t] = hmc_end_lane(a, wg, t);
            a.part[(size_t)a.geo.grid + wg] = hmc_tree_host(lane);
        }
        // (every workgroup decides before any of them commits: on the device the phases of a kernel run side by side, and
        // hmc_decide reads nothing that commit writes for this iteration)
        std::vector<double> dH(a.B), An(a.B);
        std::vector<char> acc(a.B);
        for (int b = 0; b < a.B; ++b) acc[b] = hmc_decide(a, b, dH[b], An[b]) ? 1 : 0;
        for (long wg = 0; wg < a.geo.grid; ++wg) {
            const int b = (int)(wg / a.geo.nwg);
            for (int t = 0; t < HMC_THREADS; ++t) hmc_commit_lane(a, wg, t, acc[b] != 0, dH[b], An[b]);
        }
        after(it);
    }
}

}  // namespace va

// ---------------------------------------------------------------- the kernels and their launchers (va_hmc.hip)
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

namespace va {

// one phase of one iteration (a.it) for every chain, asynchronous on s
hipError_t launch_hmc(const HmcArgs &a, int phase, hipStream_t s);
// what the kernels draw for (seed, chain, iteration): the 4 words of each of the n elements' counters and of the extra
// stream's ([n + 1][4]), the n normals, the two uniforms; device buffers
hipError_t launch_hmc_noise(uint32_t k0, uint32_t k1, uint32_t chain, uint32_t it, long n, uint32_t *words, double *normals,
                            double *uniforms, hipStream_t s);

}  // namespace va
#endif
