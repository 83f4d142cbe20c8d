// va_hmc_box.h -- the sampler of va_hmc.h for box-bounded problems: an unconstrained chain in z with x = T(z) element by
// element, T a map of the line onto the entry's interval.  The target in z is
//         U(z) = A(T(z)) - sum_i log|T_i'(z_i)|
// so the x = T(z) of the chain's states follow exp(-A) restricted to the box.  The structure is va_hmc.h's: __host__
// __device__ phases of ONE LANE, kernels k_hmc_box<PHASE> over them on the geometry of va_hmc_geo.h (va_hmc.hip),
// hmc_host_box driving the same phases lane by lane on the CPU (tests/cpu_emul/hmc_box_check.cpp), the generator, the tree
// and the workgroup-order sums of va_hmc.h, fp contraction off.  A NumPy transcription reproduces the bits
// (tests/_hmc_box_ref.py).
//
// The map.  Entry i has a kind, from its bounds (-/+HUGE_VAL: none; hmc_box_kinds, va_hmc_geo.h):
//   kind  bounds      x                   dx/dz                  d log|dx/dz| / dz
//   0     none        z                   1                      0
//   1     lower       lo + w              w / r                  1/r - z/(z z + 4)
//   2     upper       hi - w              -(w / r)               as kind 1
//   3     both        lo + (hi - lo) s    (hi - lo)/(2 q q q)    -3 z/(1 + z z)
//   r = sqrt(z z + 4);  w = (z + r)/2 for z >= 0, 2/(r - z) for z < 0 (no cancellation; the branch belongs to the
//   definition);  q = sqrt(1 + z z);  s = (1 + z/q)/2.  Kind 3's x is clamped to [lo, hi] (a rounding of the last sum).
// Deliberately algebraic: positions and momenta need + - * / sqrt only, each correctly rounded in IEEE arithmetic, so the
// bits do not depend on a library's exp or tanh.  log enters the energy alone (lj = log|dx/dz|).  The price is a polynomial
// tail: |dx/dz| falls like 1/z^2 (kinds 1, 2) and 1/|z|^3 (kind 3), so exp(-U) has heavy tails in z wherever the
// posterior has mass AT a bound -- fine for bounds used as guards, weak for posteriors piled on one.
// The inverse (hmc_box_inverse) runs on the host: kinds 1, 2  z = w - 1/w;  kind 3  z = u/sqrt((1 - u)(1 + u)),
// u = 2 (x - lo)/(hi - lo) - 1.
//
// The phases, on z [B][ld] of the call's own workspace (x, g are the handle's: the evaluator reads x, writes g = dA/dx):
//   begin   gz = g dx - dlj at the starting z;  p = normal / sqrt(minv);  restore point zs, xs, gs;  the lane's shares of
//           sum (p p) minv and of sum lj (two partial arrays);  p -= (eps_it/2) gz;  z += (eps_it minv) p;  x = T(z)
//   mid     gz at z;  p -= eps_it gz;  z += (eps_it minv) p;  x = T(z)
//   end     gz at z;  p -= (eps_it/2) gz;  both shares at the final z
//   commit  dH = ((A1 - L1) + K1) - ((A0 - L0) + K0), L the sums of lj in workgroup order;  the decision as va_hmc.h;  on
//           rejection z, x, g are restored;  Welford statistics, kept columns, traces of x, A as va_hmc.h
// minv is the inverse mass of z.  Kind 0 is va_hmc.h's arithmetic as written there (gz = g, x = z, lj = 0, A - 0 = A): a
// chain whose entries are all free takes the steps k_hmc would, bit for bit.
#pragma once
#include "va_hmc.h"

namespace va {

struct HmcBoxArgs {
    HmcArgs h;                     // everything va_hmc.h's phases take; h.x / h.g the paths and their gradient in x
    double *z, *zs;                // [B][ld]: the chain's unconstrained state; its restore point
    const int32_t *kind;           // [n_var] 0 .. 3, shared by the chains
    const double *lo, *hi;         // [n_var]
    double *lpart;                 // [2][B * nwg] partial sums of log|dx/dz| of begin / end
};

// the table above for one entry.  lj = log|dx/dz|
VA_HD void hmc_box_map(int kind, double lo, double hi, double z, double *x, double *dx, double *dlj, double *lj)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (kind == 0) { *x = z; *dx = 1.0; *dlj = 0.0; *lj = 0.0; return; }
    const double zz = z * z;
    if (kind == 3) {
        const double q2 = 1.0 + zz;
        const double q = sqrt(q2);
        const double s = (1.0 + z / q) / 2.0;
        const double wd = hi - lo;
        double xv = lo + wd * s;
        xv = xv < lo ? lo : xv;
        xv = xv > hi ? hi : xv;
        const double d = wd / (2.0 * (q * q * q));
        *x = xv; *dx = d; *dlj = (-3.0 * z) / q2; *lj = log(d);
        return;
    }
    const double r2 = zz + 4.0;
    const double r = sqrt(r2);
    const double w = z >= 0.0 ? (z + r) / 2.0 : 2.0 / (r - z);
    const double d = w / r;
    *x = kind == 1 ? lo + w : hi - w;
    *dx = kind == 1 ? d : -d;
    *dlj = 1.0 / r - z / r2;
    *lj = log(d);
}

// x = T(z) alone, the operations of hmc_box_map in the same order (the same bits): what a drift needs at the new z
VA_HD double hmc_box_x(int kind, double lo, double hi, double z)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (kind == 0) return z;
    const double zz = z * z;
    if (kind == 3) {
        const double q = sqrt(1.0 + zz);
        const double s = (1.0 + z / q) / 2.0;
        double xv = lo + (hi - lo) * s;
        xv = xv < lo ? lo : xv;
        return xv > hi ? hi : xv;
    }
    const double r = sqrt(zz + 4.0);
    const double w = z >= 0.0 ? (z + r) / 2.0 : 2.0 / (r - z);
    return kind == 1 ? lo + w : hi - w;
}

// T^-1 on the host, x strictly inside its interval (hmc_box_check_start, va_hmc_geo.h)
inline double hmc_box_inverse(int kind, double lo, double hi, double x)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (kind == 0) return x;
    if (kind == 3) {
        const double u = 2.0 * (x - lo) / (hi - lo) - 1.0;
        return u / sqrt((1.0 - u) * (1.0 + u));
    }
    const double w = kind == 1 ? x - lo : hi - x;
    return w - 1.0 / w;
}

// ---------------------------------------------------------------- phases of one lane
// entry i's kind and bounds
#define VA_HMC_BOX_ENTRY(a, i) const int kd = (a).kind[i]; const double lov = (a).lo[i], hiv = (a).hi[i]

// begin: returns the lane's share of sum (p p) minv; *ls its share of sum lj, both at the starting z
VA_HD double hmc_box_begin_lane(const HmcBoxArgs &a, long wg, int tid, double *ls)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const HmcArgs &h = a.h;
    const int b = (int)(wg / h.geo.nwg);
    const long w = wg % h.geo.nwg;
    const size_t row = (size_t)b * h.ld;
    const double eps = hmc_eps_it(h, b, h.it), half = 0.5 * eps;
    double ks = 0.0, lsum = 0.0;
    for (int e = 0; e < HMC_EPT; ++e) {
        const long i = hmc_element(h.n_var, w, tid, e);
        if (i < 0) continue;
        VA_HMC_BOX_ENTRY(a, i);
        const double mi = h.minv[(size_t)b * h.minv_stride + i], smi = h.sminv[(size_t)b * h.minv_stride + i];
        const double zv = a.z[row + i], xv = h.x[row + i], gv = h.g[row + i];
        double xm, dx, dlj, lj;
        hmc_box_map(kd, lov, hiv, zv, &xm, &dx, &dlj, &lj);
        const double gz = kd == 0 ? gv : gv * dx - dlj;
        double pv = hmc_normal(h, b, h.it, i) / smi;
        a.zs[row + i] = zv; h.xs[row + i] = xv; h.gs[row + i] = gv;
        const double pp = pv * pv;
        ks = ks + pp * mi;
        lsum = lsum + lj;
        pv = pv - half * gz;
        const double c = eps * mi;
        const double zn = zv + c * pv;
        h.p[row + i] = pv;
        a.z[row + i] = zn;
        h.x[row + i] = hmc_box_x(kd, lov, hiv, zn);
    }
    *ls = lsum;
    return ks;
}

VA_HD void hmc_box_mid_lane(const HmcBoxArgs &a, long wg, int tid)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const HmcArgs &h = a.h;
    const int b = (int)(wg / h.geo.nwg);
    const long w = wg % h.geo.nwg;
    const size_t row = (size_t)b * h.ld;
    const double eps = hmc_eps_it(h, b, h.it);
    for (int e = 0; e < HMC_EPT; ++e) {
        const long i = hmc_element(h.n_var, w, tid, e);
        if (i < 0) continue;
        VA_HMC_BOX_ENTRY(a, i);
        const double mi = h.minv[(size_t)b * h.minv_stride + i];
        const double zv = a.z[row + i], gv = h.g[row + i];
        double xm, dx, dlj, lj;
        hmc_box_map(kd, lov, hiv, zv, &xm, &dx, &dlj, &lj);
        const double gz = kd == 0 ? gv : gv * dx - dlj;
        const double pv = h.p[row + i] - eps * gz;
        const double c = eps * mi;
        const double zn = zv + c * pv;
        h.p[row + i] = pv;
        a.z[row + i] = zn;
        h.x[row + i] = hmc_box_x(kd, lov, hiv, zn);
    }
}

// end: last half kick; returns the lane's share of sum (p p) minv; *ls its share of sum lj, both at the final z
VA_HD double hmc_box_end_lane(const HmcBoxArgs &a, long wg, int tid, double *ls)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const HmcArgs &h = a.h;
    const int b = (int)(wg / h.geo.nwg);
    const long w = wg % h.geo.nwg;
    const size_t row = (size_t)b * h.ld;
    const double half = 0.5 * hmc_eps_it(h, b, h.it);
    double ks = 0.0, lsum = 0.0;
    for (int e = 0; e < HMC_EPT; ++e) {
        const long i = hmc_element(h.n_var, w, tid, e);
        if (i < 0) continue;
        VA_HMC_BOX_ENTRY(a, i);
        const double gv = h.g[row + i];
        double xm, dx, dlj, lj;
        hmc_box_map(kd, lov, hiv, a.z[row + i], &xm, &dx, &dlj, &lj);
        const double gz = kd == 0 ? gv : gv * dx - dlj;
        const double pv = h.p[row + i] - half * gz;
        h.p[row + i] = pv;
        const double pp = pv * pv;
        ks = ks + pp * h.minv[(size_t)b * h.minv_stride + i];
        lsum = lsum + lj;
    }
    *ls = lsum;
    return ks;
}
#undef VA_HMC_BOX_ENTRY

// the decision of (chain b, iteration a.h.it) from the partial sums in workgroup order
VA_HD bool hmc_box_decide(const HmcBoxArgs &a, int b, double &dH, double &A_new)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const HmcArgs &h = a.h;
    const size_t o0 = (size_t)b * h.geo.nwg, o1 = (size_t)h.geo.grid + (size_t)b * h.geo.nwg;
    double s0 = 0.0, s1 = 0.0, L0 = 0.0, L1 = 0.0;
    for (long w = 0; w < h.geo.nwg; ++w) {
        s0 = s0 + h.part[o0 + w]; s1 = s1 + h.part[o1 + w];
        L0 = L0 + a.lpart[o0 + w]; L1 = L1 + a.lpart[o1 + w];
    }
    const double K0 = 0.5 * s0, K1 = 0.5 * s1;
    const double A0 = h.A_cur[(size_t)(h.it & 1) * h.B + b], A1 = h.A_eval[b];
    dH = ((A1 - L1) + K1) - ((A0 - L0) + K0);
    double u_acc, u_jit;
    hmc_uniforms(h, b, h.it, u_acc, u_jit);
    const bool acc = hmc_finite(dH) && log(u_acc) < -dH;
    A_new = acc ? A1 : A0;
    return acc;
}

// commit: va_hmc.h's, after z has been put back where the iteration is rejected (the statistics and kept columns are of x)
VA_HD void hmc_box_commit_lane(const HmcBoxArgs &a, long wg, int tid, bool acc, double dH, double A_new)
{
    const HmcArgs &h = a.h;
    if (!acc) {
        const size_t row = (size_t)(wg / h.geo.nwg) * h.ld;
        const long w = wg % h.geo.nwg;
        for (int e = 0; e < HMC_EPT; ++e) {
            const long i = hmc_element(h.n_var, w, tid, e);
            if (i >= 0) a.z[row + i] = a.zs[row + i];
        }
    }
    hmc_commit_lane(h, wg, tid, acc, dH, A_new);
}

// ---------------------------------------------------------------- the same phases, lane by lane on the host
// As hmc_host (va_hmc.h); a.z holds the start in z and a.h.x = T(z), a.h.g the gradient there, A_cur[0][b] the action.
template <class EVAL, class AFTER>
inline void hmc_host_box(HmcBoxArgs a, int n_leap, EVAL &&eval, AFTER &&after)
{
    HmcArgs &h = a.h;
    std::vector<double> lane(HMC_THREADS), llane(HMC_THREADS);
    for (int it = 0; it < h.n_iter; ++it) {
        h.it = it;
        for (long wg = 0; wg < h.geo.grid; ++wg) {
            for (int t = 0; t < HMC_THREADS; ++t) lane[t] = hmc_box_begin_lane(a, wg, t, &llane[t]);
            h.part[wg] = hmc_tree_host(lane);
            a.lpart[wg] = hmc_tree_host(llane);
        }
        for (int l = 0; l < n_leap; ++l) {
            if (l)
                for (long wg = 0; wg < h.geo.grid; ++wg)
                    for (int t = 0; t < HMC_THREADS; ++t) hmc_box_mid_lane(a, wg, t);
            eval();
        }
        for (long wg = 0; wg < h.geo.grid; ++wg) {
            for (int t = 0; t < HMC_THREADS; ++t) lane[t] = hmc_box_end_lane(a, wg, t, &llane[t]);
            h.part[(size_t)h.geo.grid + wg] = hmc_tree_host(lane);
            a.lpart[(size_t)h.geo.grid + wg] = hmc_tree_host(llane);
        }
        std::vector<double> dH(h.B), An(h.B);
        std::vector<char> acc(h.B);
        for (int b = 0; b < h.B; ++b) acc[b] = hmc_box_decide(a, b, dH[b], An[b]) ? 1 : 0;
        for (long wg = 0; wg < h.geo.grid; ++wg) {
            const int b = (int)(wg / h.geo.nwg);
            for (int t = 0; t < HMC_THREADS; ++t) hmc_box_commit_lane(a, wg, t, acc[b] != 0, dH[b], An[b]);
        }
        after(it);
    }
}

}  // namespace va

// ---------------------------------------------------------------- the kernels and their launchers (va_hmc.hip)
#if defined(__HIPCC__)
namespace va {

// one phase of one iteration (a.h.it) for every chain, asynchronous on s
hipError_t launch_hmc_box(const HmcBoxArgs &a, int phase, hipStream_t s);
// hmc_box_map over a table of n entries on the device (kind, lo, hi, z in; x, dx, dlj, lj out: device buffers)
hipError_t launch_hmc_box_map(long n, const int32_t *kind, const double *lo, const double *hi, const double *z, double *x, double *dx,
                              double *dlj, double *lj, hipStream_t s);

}  // namespace va
#endif
