// va_lyap.h -- Lyapunov spectra of the fitted model: K tangents carried along a trajectory by the tangent-linear RK4 map
// and re-orthonormalised together every few steps (Benettin's method), free or coupled to the drive by a gain.
//
// There are T trajectories, each with a state x (D), parameters p (NP), K <= D tangents V (K x D) and an optional gain
// vector g (D), g >= 0 (NULL: zeros).  Per RK4 substep the nominal state moves exactly as k_predict moves it
// (va_predict.h), and every tangent by va_predict_tlm.h's rule with a zero parameter tangent and the gain term:
//     k1' = J(x) v - g o v,   k2' = J(x + h/2 k1)(v + h/2 k1') - g o (v + h/2 k1'),   ...,   v += h/6 (k1' + 2 k2' + 2 k3' + k4')
// J(x_stage) w = RHS::jvp(x_stage; w, 0).  With the gain this is the exact derivative, on the manifold y = x, of the jointly
// RK4-discretised drive-response pair  x' = f(x),  y' = f(y) + g o (x - y)  with respect to y: the tangent of the DISCRETE
// map, like everything else here.  Stage times, substeps and stimulus interpolation are va_predict.h's.
// After every qr_every model steps the thin QR  V^T = Q R,  R_jj > 0  is taken (tangents are the rows of V), V <- Q^T, and
// for QR index m >= n_skip  S_j += log R_jj, in time order.  n_steps is a multiple of qr_every; n_qr = n_steps / qr_every,
// 0 <= n_skip < n_qr.  Out per trajectory: logsum[K] = S, x_end[D], Q_end[K][D], optionally the trace [n_qr][K] of every
// log R_jj (transient included), and status: when some R_jj is zero or not finite, status = j + 1 of the first such j of the
// first such QR and logsum is NaN for that trajectory (Q_end then holds what the arithmetic gave); nothing else is touched.
// Q0 = NULL starts from the first K unit vectors.  The exponents are logsum / ((n_qr - n_skip) qr_every dt): the host's.
//
// The QR is Gram-Schmidt, column by column, each projection applied to the remaining tangents as soon as its vector is
// final (the modified form), with the projection coefficient taken against the UNNORMALISED vector:
//     for j = 0 .. K-1:   d_j = u_j . u_j,   R_jj = sqrt(d_j);   for k > j:  c = (u_j . v_k) / d_j,   v_k -= c u_j
//     q_j = u_j / R_jj
// All of a step's K - j dot products are formed at once, one lane each, summed along the columns in index order -- the
// same bits on every call -- and every lane of a tangent element applies its projection: two synchronisations per column,
// 2 K per QR against the 4 substeps qr_every of the steps between two QRs.  The unnormalised coefficient costs nothing and
// makes an exactly repeated (or exactly doubled) tangent an exact zero: R_jj = 0, status j + 1.  The thin QR with a positive
// diagonal is unique, so the choice of scheme is invisible beyond rounding; Gram matrix + Cholesky would have the shorter
// dependency chain but squares the condition number of V, which grows like exp((l_1 - l_K) qr_every dt).
//
// Like va_predict_tlm.h the arithmetic is written once as __host__ __device__ phases of ONE LANE; k_lyap gives them their
// decomposition (va_lyap_geo.h), lyap_host drives them lane by lane on the CPU (tests/cpu_emul/lyap_check.cpp).  A lane
// owns E elements (slot, column) of its workgroup; state, tangents and k-accumulators live in registers; the stage inputs
// go through two LDS images, ONE synchronisation per stage.  The QR works in the image that holds the step's result (the
// one the next first stage reads) and in the registers that own its elements.
#pragma once
#include <math.h>
#include <vector>

#include "va_core.h"
#include "va_predict.h"
#include "va_lyap_geo.h"

namespace va {

struct LyapArgs {
    const double *x0;        // [T][D]
    const double *p;         // [T][NP]
    const double *Q0;        // [T][K][D], or NULL: the first K unit vectors
    const double *coupling;  // [T][D] gains, or NULL: none
    const double *stim;      // NULL or [n_steps + 1][nstim], shared by the trajectories
    double *logsum;          // [T][K]
    double *x_end;           // [T][D]
    double *Q_end;           // [T][K][D]
    double *trace;           // [T][n_qr][K], or NULL
    int *status;             // [T]
    int T, D, NP, K, nstim, n_steps, substeps, qr_every, n_skip;
    double t0, dt;
    LyapGeo geo;
};

// one element of a lane: kind 0 nobody's, 1 nominal, 2 tangent
struct LyapElem {
    int kind, col;
    int k;                   // a tangent's index 0 .. K-1
    int xoff, noff;          // the element's slot and its trajectory's nominal slot in a stage image (doubles)
    int poff, goff, coff;    // the trajectory's parameters and gains; the tangent's entry of the QR's tables
    long traj;
};

template <int E> struct LyapLane {
    double x[E], acc[E];     // state or tangent, and its k-accumulator
    double g0, g1, gn;       // the lane's stimulus column at the rows n, n + 1 and (prefetched) n + 2
    double S;                // the log sum of the tangent whose dot products this lane forms
    int dr, dk;              // that tangent: trajectory slot and index (dk < 0: none)
    long dtraj;
    LyapElem el[E];
};

// the workgroup's LDS (lyap_lds_doubles)
struct LyapLds { double *xs, *ps, *zs, *gs, *sts, *cs, *dd, *stat; int img; };
VA_HD LyapLds lyap_lds(const LyapArgs &a, double *base)
{
    LyapLds l;
    const int RW = a.geo.RW;
    l.img = RW * (a.K + 1) * a.geo.pitch;
    l.xs = base; l.ps = l.xs + 2 * (size_t)l.img; l.zs = l.ps + (size_t)RW * a.NP; l.gs = l.zs + a.NP; l.sts = l.gs + (size_t)RW * a.D;
    l.cs = l.sts + 2 * (size_t)a.nstim; l.dd = l.cs + (size_t)RW * a.K; l.stat = l.dd + (size_t)RW * a.K;
    return l;
}

VA_HD bool lyap_bad_diag(double R) { return !(R > 0.0) || !(R <= 1.7976931348623157e308); }

// phase 0: the lane's elements and their start values (x0 / Q0 or unit vectors) into the registers and the first stage
// input; the workgroup's parameters, gains and the one zero parameter tangent; the lane's stimulus column at rows 0 and 1
template <int E>
VA_HD void lyap_load(const LyapArgs &a, const LyapLds &l, long wg, int tid, LyapLane<E> &L)
{
    const LyapGeo &g = a.geo;
    const int D = a.D, K = a.K, P = g.pitch;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        LyapElem &el = L.el[e];
        int r, s;
        lyap_elem(K, D, tid + e * g.threads, &r, &s, &el.col);
        el.traj = wg * g.RW + r;
        el.kind = (r < g.RW && el.traj < a.T) ? (s == 0 ? 1 : 2) : 0;
        el.k = s - 1;
        el.noff = r * (K + 1) * P; el.xoff = el.noff + s * P;
        el.poff = r * a.NP; el.goff = r * D; el.coff = r * K + (s > 0 ? s - 1 : 0);
        L.x[e] = 0.0; L.acc[e] = 0.0;
        if (el.kind == 1) L.x[e] = a.x0[(size_t)el.traj * D + el.col];
        else if (el.kind == 2) L.x[e] = a.Q0 ? a.Q0[((size_t)el.traj * K + el.k) * D + el.col] : (el.col == el.k ? 1.0 : 0.0);
        if (el.kind) l.xs[el.xoff + el.col] = L.x[e];
    }
    // (the trajectories of a workgroup are neighbours in p and coupling as they are in the LDS image)
    const long np = (long)g.RW * a.NP, first = wg * np, all = (long)a.T * a.NP;
    for (long e = tid; e < np; e += g.threads) l.ps[e] = first + e < all ? a.p[first + e] : 0.0;
    for (int e = tid; e < a.NP; e += g.threads) l.zs[e] = 0.0;
    const long ng = (long)g.RW * D, gfirst = wg * ng, gall = (long)a.T * D;
    for (long e = tid; e < ng; e += g.threads) l.gs[e] = (a.coupling && gfirst + e < gall) ? a.coupling[gfirst + e] : 0.0;
    if (tid < g.RW) l.stat[tid] = 0.0;
    L.dr = tid / K; L.dk = tid - L.dr * K; L.dtraj = wg * g.RW + L.dr; L.S = 0.0;
    if (L.dr >= g.RW || L.dtraj >= a.T) { L.dr = 0; L.dk = -1; L.dtraj = 0; }
    L.g0 = 0.0; L.g1 = 0.0; L.gn = 0.0;
    if (tid < a.nstim) { L.g1 = a.stim[tid]; L.gn = a.stim[a.nstim + tid]; }
}

// start of model step n: the lane's stimulus column moves on one row; row n + 2 is asked for a step ahead of its use
template <int E>
VA_HD void lyap_stim_step(const LyapArgs &a, int tid, int n, LyapLane<E> &L)
{
    L.g0 = L.g1; L.g1 = L.gn;
    if (tid < a.nstim && n + 2 <= a.n_steps) L.gn = a.stim[(size_t)(n + 2) * a.nstim + tid];
}

// before the synchronisation of a stage: the stimulus at the stage's time into the image the stage reads
template <int E, int STAGE>
VA_HD void lyap_stim_stage(const LyapArgs &a, const LyapLds &l, int tid, int s, const LyapLane<E> &L)
{
    constexpr int in = STAGE & 1;
    if (tid < a.nstim)
        l.sts[in * a.nstim + tid] = predict_interp(L.g0, L.g1, ((double)s + predict_c<STAGE>()) / (double)a.substeps);
}

// after it: k = f(stage input) for a nominal element, k' = jvp(nominal stage input; tangent stage input, 0) - g o (tangent
// stage input) for a tangent; the next stage's input into the other image
template <class RHS, int E, int STAGE>
VA_HD void lyap_stage(const LyapArgs &a, const LyapLds &l, long long q, const PredictStep &hs, LyapLane<E> &L)
{
    constexpr int in = STAGE & 1;
    const int D = a.D;
    const double *xin = l.xs + (size_t)in * l.img;
    double *xout = l.xs + (size_t)(in ^ 1) * l.img;
    const double *st = l.sts + in * a.nstim;
    const double t = predict_time(a.t0, q, predict_c<STAGE>(), hs.h);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const LyapElem &el = L.el[e];
        if (el.kind) {
            double k;
            if (el.kind == 1) k = predict_f<RHS>(xin + el.noff, el.col, D, l.ps + el.poff, t, st);
            else {
                k = RHS::jvp(xin + el.noff, xin + el.xoff, l.zs, el.col, D, l.ps + el.poff, t, st);
                if (a.coupling) k -= l.gs[el.goff + el.col] * xin[el.xoff + el.col];
            }
            double *xo = xout + el.xoff + el.col;
            if (STAGE == 0) { L.acc[e] = k; *xo = L.x[e] + hs.hh * k; }
            else if (STAGE == 1) { L.acc[e] += 2.0 * k; *xo = L.x[e] + hs.hh * k; }
            else if (STAGE == 2) { L.acc[e] += 2.0 * k; *xo = L.x[e] + hs.h * k; }
            else { L.acc[e] += k; L.x[e] += hs.h6 * L.acc[e]; *xo = L.x[e]; }
        }
    }
}

// QR, column j, first half: the lane of tangent k >= j sums u_j . v_k and u_j . u_j along the columns; k = j keeps the squared
// norm and looks at R_jj, k > j leaves the projection coefficient
template <int E>
VA_HD void lyap_qr_dots(const LyapArgs &a, const LyapLds &l, int j, const LyapLane<E> &L)
{
    if (L.dk < j) return;
    const int P = a.geo.pitch;
    const double *u = l.xs + (size_t)(L.dr * (a.K + 1) + j + 1) * P, *v = l.xs + (size_t)(L.dr * (a.K + 1) + L.dk + 1) * P;
    double s = 0.0, d = 0.0;
    for (int i = 0; i < a.D; ++i) { const double ui = u[i]; s += ui * v[i]; d += ui * ui; }
    if (L.dk == j) {
        l.dd[L.dr * a.K + j] = d;
        if (lyap_bad_diag(sqrt(d)) && l.stat[L.dr] == 0.0) l.stat[L.dr] = (double)(j + 1);
    } else l.cs[L.dr * a.K + L.dk] = s / d;
}

// second half: every element of a tangent k > j takes its projection on u_j off
template <int E>
VA_HD void lyap_qr_update(const LyapArgs &a, const LyapLds &l, int j, LyapLane<E> &L)
{
    const int P = a.geo.pitch;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const LyapElem &el = L.el[e];
        if (el.kind == 2 && el.k > j) {
            L.x[e] -= l.cs[el.coff] * l.xs[el.noff + (j + 1) * P + el.col];
            l.xs[el.xoff + el.col] = L.x[e];
        }
    }
}

// after the last column: q_k = u_k / R_kk into the registers and the image; log R_kk into the trace and, past the transient,
// the sum.  m: the QR's index
template <int E>
VA_HD void lyap_qr_finish(const LyapArgs &a, const LyapLds &l, int m, LyapLane<E> &L)
{
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const LyapElem &el = L.el[e];
        if (el.kind == 2) {
            L.x[e] = L.x[e] / sqrt(l.dd[el.coff]);
            l.xs[el.xoff + el.col] = L.x[e];
        }
    }
    if (L.dk >= 0) {
        const double lr = log(sqrt(l.dd[L.dr * a.K + L.dk]));
        if (a.trace) a.trace[((size_t)L.dtraj * (a.n_steps / a.qr_every) + m) * a.K + L.dk] = lr;
        if (m >= a.n_skip) L.S += lr;
    }
}

// the end: state and tangents from the registers, the sums and the status
template <int E>
VA_HD void lyap_store(const LyapArgs &a, const LyapLds &l, const LyapLane<E> &L)
{
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const LyapElem &el = L.el[e];
        if (el.kind == 1) a.x_end[(size_t)el.traj * a.D + el.col] = L.x[e];
        else if (el.kind == 2) a.Q_end[((size_t)el.traj * a.K + el.k) * a.D + el.col] = L.x[e];
    }
    if (L.dk >= 0) {
        const double st = l.stat[L.dr];
        a.logsum[(size_t)L.dtraj * a.K + L.dk] = st != 0.0 ? __builtin_nan("") : L.S;
        if (L.dk == 0) a.status[L.dtraj] = (int)st;
    }
}

// ---------------------------------------------------------------- the same phases, lane by lane on the host
// (every pointer of `a` is host memory; a.geo from plan_lyap)
template <class RHS, int E>
inline void lyap_host_e(const LyapArgs &a)
{
    const int nt = a.geo.threads;
    const PredictStep hs = predict_step_sizes(a.dt, a.substeps);
    std::vector<double> mem(lyap_lds_doubles(a.geo.RW, a.K, a.D, a.NP, a.nstim) + 1, 0.0);
    std::vector<LyapLane<E>> L(nt);
    const LyapLds l = lyap_lds(a, mem.data());
    for (long wg = 0; wg < a.geo.grid; ++wg) {
        for (int tid = 0; tid < nt; ++tid) lyap_load<E>(a, l, wg, tid, L[tid]);
        long long q = 0;
        int until_qr = a.qr_every, m = 0;
        for (int n = 0; n < a.n_steps; ++n) {
            if (a.nstim) for (int tid = 0; tid < nt; ++tid) lyap_stim_step<E>(a, tid, n, L[tid]);
            for (int s = 0; s < a.substeps; ++s, ++q) {
                for (int tid = 0; tid < nt; ++tid) lyap_stim_stage<E, 0>(a, l, tid, s, L[tid]);
                for (int tid = 0; tid < nt; ++tid) lyap_stage<RHS, E, 0>(a, l, q, hs, L[tid]);
                for (int tid = 0; tid < nt; ++tid) lyap_stim_stage<E, 1>(a, l, tid, s, L[tid]);
                for (int tid = 0; tid < nt; ++tid) lyap_stage<RHS, E, 1>(a, l, q, hs, L[tid]);
                for (int tid = 0; tid < nt; ++tid) lyap_stim_stage<E, 2>(a, l, tid, s, L[tid]);
                for (int tid = 0; tid < nt; ++tid) lyap_stage<RHS, E, 2>(a, l, q, hs, L[tid]);
                for (int tid = 0; tid < nt; ++tid) lyap_stim_stage<E, 3>(a, l, tid, s, L[tid]);
                for (int tid = 0; tid < nt; ++tid) lyap_stage<RHS, E, 3>(a, l, q, hs, L[tid]);
            }
            if (--until_qr == 0) {
                until_qr = a.qr_every;
                for (int j = 0; j < a.K; ++j) {
                    for (int tid = 0; tid < nt; ++tid) lyap_qr_dots<E>(a, l, j, L[tid]);
                    if (j + 1 < a.K) for (int tid = 0; tid < nt; ++tid) lyap_qr_update<E>(a, l, j, L[tid]);
                }
                for (int tid = 0; tid < nt; ++tid) lyap_qr_finish<E>(a, l, m, L[tid]);
                ++m;
            }
        }
        for (int tid = 0; tid < nt; ++tid) lyap_store<E>(a, l, L[tid]);
    }
}

template <class RHS>
inline void lyap_host(const LyapArgs &a)
{
    switch (a.geo.E) {
    case 1: lyap_host_e<RHS, 1>(a); break;
    case 2: lyap_host_e<RHS, 2>(a); break;
    case 3: lyap_host_e<RHS, 3>(a); break;
    case 4: lyap_host_e<RHS, 4>(a); break;
    case 5: lyap_host_e<RHS, 5>(a); break;
    case 6: lyap_host_e<RHS, 6>(a); break;
    case 7: lyap_host_e<RHS, 7>(a); break;
    default: lyap_host_e<RHS, 8>(a); break;
    }
}

}  // namespace va

// ---------------------------------------------------------------- the kernel
#if defined(__HIPCC__)
#include "va_eval_flat.h"      // wave_sync_lds

namespace va {

template <class RHS, int E, bool WAVE>
__global__ __launch_bounds__(WAVE ? 64 : LYAP_MAX_THREADS) void k_lyap(const LyapArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double lyap_mem[];
    const LyapLds l = lyap_lds(a, lyap_mem);
    const int tid = (int)threadIdx.x;
    const PredictStep hs = predict_step_sizes(a.dt, a.substeps);
    LyapLane<E> L;
    lyap_load<E>(a, l, (long)blockIdx.x, tid, L);
    long long q = 0;
    int until_qr = a.qr_every, m = 0;
    for (int n = 0; n < a.n_steps; ++n) {
        if (a.nstim) lyap_stim_step<E>(a, tid, n, L);
        for (int s = 0; s < a.substeps; ++s, ++q) {
            lyap_stim_stage<E, 0>(a, l, tid, s, L); predict_sync<WAVE>(); lyap_stage<RHS, E, 0>(a, l, q, hs, L);
            lyap_stim_stage<E, 1>(a, l, tid, s, L); predict_sync<WAVE>(); lyap_stage<RHS, E, 1>(a, l, q, hs, L);
            lyap_stim_stage<E, 2>(a, l, tid, s, L); predict_sync<WAVE>(); lyap_stage<RHS, E, 2>(a, l, q, hs, L);
            lyap_stim_stage<E, 3>(a, l, tid, s, L); predict_sync<WAVE>(); lyap_stage<RHS, E, 3>(a, l, q, hs, L);
        }
        if (--until_qr == 0) {
            until_qr = a.qr_every;
            for (int j = 0; j < a.K; ++j) {
                predict_sync<WAVE>();      // (the step's result, or column j - 1's projections, are in the image)
                lyap_qr_dots<E>(a, l, j, L);
                predict_sync<WAVE>();
                if (j + 1 < a.K) lyap_qr_update<E>(a, l, j, L);
            }
            lyap_qr_finish<E>(a, l, m, L);
            ++m;
        }
    }
    predict_sync<WAVE>();                  // (the status of the last QR)
    lyap_store<E>(a, l, L);
}

// can a model of DC columns (a generated module; 0: any D) run with E elements per lane beside a workgroup barrier?
constexpr bool lyap_can(int DC, int E)
{
    return DC == 0 || (DC <= LYAP_MAX_D && (DC + 1) * DC > 64 && (DC + 1) * DC > LYAP_MAX_THREADS * (E - 1));
}

template <class RHS, int E, int DC>
inline hipError_t launch_lyap_e(const LyapArgs &a, hipStream_t s)
{
    if constexpr (lyap_can(DC, E)) {
        hipLaunchKernelGGL((k_lyap<RHS, E, false>), dim3((unsigned)a.geo.grid), dim3((unsigned)a.geo.threads), a.geo.lds_bytes, s, a);
        return hipGetLastError();
    }
    return hipErrorInvalidValue;      // (a geometry plan_lyap does not make for this D)
}

// launch the instantiation a.geo names.  DC > 0: the model's D is a constant (a generated module): only the
// instantiations that D can run are compiled (E depends on the number of exponents of the call as well)
template <class RHS, int DC>
inline hipError_t launch_lyap(const LyapArgs &a, hipStream_t s)
{
    if (DC > 0 && a.D != DC) return hipErrorInvalidValue;
    LyapGeo g;
    if (!plan_lyap(a.D, a.T, a.K, a.NP, a.nstim, g)) return hipErrorInvalidValue;
    if (g.RW != a.geo.RW || g.threads != a.geo.threads || g.E != a.geo.E || g.wave != a.geo.wave || g.pitch != a.geo.pitch
        || g.lds_bytes != a.geo.lds_bytes || g.grid != a.geo.grid) return hipErrorInvalidValue;
    if (g.wave) {
        if constexpr (DC == 0 || 2 * DC <= 64) {
            hipLaunchKernelGGL((k_lyap<RHS, 1, true>), dim3((unsigned)g.grid), dim3(64), g.lds_bytes, s, a);
            return hipGetLastError();
        }
        return hipErrorInvalidValue;
    }
    switch (g.E) {
    case 1: return launch_lyap_e<RHS, 1, DC>(a, s);
    case 2: return launch_lyap_e<RHS, 2, DC>(a, s);
    case 3: return launch_lyap_e<RHS, 3, DC>(a, s);
    case 4: return launch_lyap_e<RHS, 4, DC>(a, s);
    case 5: return launch_lyap_e<RHS, 5, DC>(a, s);
    case 6: return launch_lyap_e<RHS, 6, DC>(a, s);
    case 7: return launch_lyap_e<RHS, 7, DC>(a, s);
    default: return launch_lyap_e<RHS, 8, DC>(a, s);
    }
}

}  // namespace va
#endif
