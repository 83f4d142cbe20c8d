// va_enkf.h -- tracking new data from the estimates: the ensemble Kalman filter, forecast and analysis alternating on the
// device without a return to the host.
//
// There are T points, each with M members x (M x D), the members' full parameter vectors p (M x NP), a list est of NQ
// positions in p that the filter updates (NQ = 0: states only) and observations Y (n_obs x L) of the Lidx columns, NaN for
// a missing one; shared by the points are obs_var (L), inflation >= 1, obs_every, substeps, t0 and the stimulus
// [n_obs obs_every + 1][nstim].  For observation row k = 0 .. n_obs - 1:
//   1 forecast    every member moves obs_every model steps exactly as k_predict moves a trajectory (va_predict.h: the same
//                 RK4 rule, stage times, substeps and stimulus interpolation), each with its own parameter vector
//   2 statistics  of the D + NQ augmented variables z = (x, p[est]): mean_f = sum_m z_m / M in member order,
//                 sd_f = sqrt(sum_m (z_m - mean)^2 / (M - 1))
//   3 inflation   z_m = mean + inflation (z_m - mean), skipped exactly at inflation = 1
//   4 analysis    the serial ensemble square-root filter (Whitaker & Hamill 2002): for j = 0 .. L-1 in order, unless
//                 y = Y[k][j] is NaN, with c = Lidx[j], r = obs_var[j]:
//                     h_m = x_m[c],  hbar = sum_m h_m / M,  a_m = h_m - hbar,  s = sum_m a_m^2 / (M - 1),  d = s + r
//                     zbar_i = sum_m z_mi / M,  c_i = sum_m (z_mi - zbar_i) a_m / (M - 1),  K_i = c_i / d
//                     alpha = 1 / (1 + sqrt(r / d)),   z_mi += K_i (y - hbar) - alpha K_i a_m
//                 (the increment form: a zero gain leaves a member alone); every observation sees the members as the
//                 previous one left them
//   5 statistics  mean_a, sd_a, by 2's formulas
// status is 0, or k + 1 of the first row at whose forecast some augmented variable of some member is not finite: from that
// row on the point's four statistics are NaN, x_end / p_end hold what the arithmetic gave, no other point is touched.
//
// Like va_lyap.h the arithmetic is written once as __host__ __device__ phases of ONE LANE; k_enkf gives them their
// decomposition (va_enkf_geo.h), enkf_host drives them lane by lane on the CPU (tests/cpu_emul/enkf_check.cpp).  A lane owns
// E elements (member, column) of its point; their state and k-accumulators live in registers; the stage inputs go through
// two LDS images, ONE synchronisation per stage; the members' parameters are in LDS [M][NP].  For the analysis the D + NQ
// augmented variables are dealt to the lanes: a variable's lane walks its column across the M slots (pitch odd: no LDS bank
// twice) and forms hbar, s, d and its own zbar_i, c_i, K_i -- all sums in member order on that one lane, no atomics, the
// same bits on every call -- and leaves K_i in a table, from which every element then takes its increment.  An estimated
// parameter has no element registers: its variable lane updates its M LDS entries itself, while it holds K_i.  The updated
// members are written to the OTHER image, so that no element reads a_m from a column c already updated: an assimilated
// observation costs TWO synchronisations (the image complete before the sums, the table complete before the increments), a
// missing one none.
#pragma once
#include <math.h>
#include <vector>

#include "va_core.h"
#include "va_predict.h"
#include "va_enkf_geo.h"

namespace va {

struct EnkfArgs {
    const double *x0;        // [T][M][D]
    const double *p;         // [T][M][NP]
    const double *Y;         // [T][n_obs][L], NaN: missing
    const double *obs_var;   // [L]
    const double *stim;      // NULL or [n_obs obs_every + 1][nstim], shared by the points
    const int *est;          // [NQ] positions in a parameter vector
    const int *Lidx;         // [L] observed columns
    double *mean_f, *sd_f, *mean_a, *sd_a;      // [T][n_obs][D + NQ]
    double *x_end;           // [T][M][D]
    double *p_end;           // [T][M][NP]
    int *status;             // [T]
    int T, D, NP, NQ, L, M, nstim, n_obs, obs_every, substeps;
    double t0, dt, inflation;
    EnkfGeo geo;
};

// one element of a lane: its column, its member's slot in a stage image and its member's parameters (doubles)
struct EnkfElem { int live, col, xoff, poff; };

template <int E> struct EnkfLane {
    double x[E], acc[E];     // state and its k-accumulator
    double g0, g1, gn;       // the lane's stimulus column at the rows n, n + 1 and (prefetched) n + 2
    EnkfElem el[E];
};

// the workgroup's LDS (enkf_lds_doubles).  sc: hbar, y - hbar, alpha, status
struct EnkfLds { double *xs, *ps, *sts, *mu, *sg, *kt, *sc; int img; };
VA_HD EnkfLds enkf_lds(const EnkfArgs &a, double *base)
{
    EnkfLds l;
    const int NV = a.D + a.NQ;
    l.img = a.M * a.geo.pitch;
    l.xs = base; l.ps = l.xs + 2 * (size_t)l.img; l.sts = l.ps + (size_t)a.M * a.NP; l.mu = l.sts + 2 * (size_t)a.nstim;
    l.sg = l.mu + NV; l.kt = l.sg + NV; l.sc = l.kt + NV;
    return l;
}

VA_HD bool enkf_not_finite(double v) { return !(fabs(v) <= 1.7976931348623157e308); }

// phase 0: the lane's elements and their start values into the registers and the first stage input (image 0); the point's
// parameters; the lane's stimulus column at rows 0 and 1
template <int E>
VA_HD void enkf_load(const EnkfArgs &a, const EnkfLds &l, long wg, int tid, EnkfLane<E> &L)
{
    const EnkfGeo &g = a.geo;
    const int D = a.D;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        EnkfElem &el = L.el[e];
        const int q = tid + e * g.threads, m = q / D;
        el.col = q - m * D;
        el.live = m < a.M ? 1 : 0;
        el.xoff = m * g.pitch; el.poff = m * a.NP;
        L.x[e] = 0.0; L.acc[e] = 0.0;
        if (el.live) {
            L.x[e] = a.x0[((size_t)wg * a.M + m) * D + el.col];
            l.xs[el.xoff + el.col] = L.x[e];
        }
    }
    const long np = (long)a.M * a.NP;
    for (long e = tid; e < np; e += g.threads) l.ps[e] = a.p[(size_t)wg * np + e];
    if (tid == 0) l.sc[3] = 0.0;
    L.g0 = 0.0; L.g1 = 0.0; L.gn = 0.0;
    if (tid < a.nstim) { L.g1 = a.stim[tid]; L.gn = a.stim[a.nstim + tid]; }
}

// start of model step n: the lane's stimulus column moves on one row; row n + 2 is asked for a step ahead of its use
template <int E>
VA_HD void enkf_stim_step(const EnkfArgs &a, int tid, int n, EnkfLane<E> &L)
{
    L.g0 = L.g1; L.g1 = L.gn;
    if (tid < a.nstim && n + 2 <= a.n_obs * a.obs_every) L.gn = a.stim[(size_t)(n + 2) * a.nstim + tid];
}

// before the synchronisation of a stage: the stimulus at the stage's time into the table the stage reads
template <int E, int STAGE>
VA_HD void enkf_stim_stage(const EnkfArgs &a, const EnkfLds &l, int tid, int s, const EnkfLane<E> &L)
{
    constexpr int in = STAGE & 1;
    if (tid < a.nstim)
        l.sts[in * a.nstim + tid] = predict_interp(L.g0, L.g1, ((double)s + predict_c<STAGE>()) / (double)a.substeps);
}

// after it: k = f(stage input) with the member's own parameters; the next stage's input into the other image.  cur: the
// image that holds the members at the start of the sub-step (the analysis moves it), and holds them again after stage 3
template <class RHS, int E, int STAGE>
VA_HD void enkf_stage(const EnkfArgs &a, const EnkfLds &l, int cur, long long q, const PredictStep &hs, EnkfLane<E> &L)
{
    const int in = cur ^ (STAGE & 1);
    const double *xin = l.xs + (size_t)in * l.img;
    double *xout = l.xs + (size_t)(in ^ 1) * l.img;
    const double *st = l.sts + (STAGE & 1) * a.nstim;
    const double t = predict_time(a.t0, q, predict_c<STAGE>(), hs.h);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const EnkfElem &el = L.el[e];
        if (el.live) {
            const double k = predict_f<RHS>(xin + el.xoff, el.col, a.D, l.ps + el.poff, t, st);
            double *xo = xout + el.xoff + el.col;
            if (STAGE == 0) { L.acc[e] = k; *xo = L.x[e] + hs.hh * k; }
            else if (STAGE == 1) { L.acc[e] += 2.0 * k; *xo = L.x[e] + hs.hh * k; }
            else if (STAGE == 2) { L.acc[e] += 2.0 * k; *xo = L.x[e] + hs.h * k; }
            else { L.acc[e] += k; L.x[e] += hs.h6 * L.acc[e]; *xo = L.x[e]; }
        }
    }
}

// column v of the augmented variables across the members: a state column of image `cur`, or an estimated parameter
VA_HD double *enkf_column(const EnkfArgs &a, const EnkfLds &l, int cur, int v, int *stride)
{
    if (v < a.D) { *stride = a.geo.pitch; return l.xs + (size_t)cur * l.img + v; }
    *stride = a.NP;
    return l.ps + a.est[v - a.D];
}

// mean and standard deviation of every augmented variable, one lane each, summed across the members in member order.
// FORECAST: into the tables, and the point's status when a member is not finite; otherwise the analysis statistics of row k
// straight to mean_a / sd_a
template <bool FORECAST>
VA_HD void enkf_stats(const EnkfArgs &a, const EnkfLds &l, int cur, long wg, int tid, int k)
{
    const int NV = a.D + a.NQ, M = a.M;
    for (int v = tid; v < NV; v += a.geo.threads) {
        int stride;
        const double *z = enkf_column(a, l, cur, v, &stride);
        double sum = 0.0;
        bool bad = false;
        for (int m = 0; m < M; ++m) { const double zm = z[(size_t)m * stride]; sum += zm; bad = bad || enkf_not_finite(zm); }
        const double mean = sum / (double)M;
        double var = 0.0;
        for (int m = 0; m < M; ++m) { const double dz = z[(size_t)m * stride] - mean; var += dz * dz; }
        const double sd = sqrt(var / (double)(M - 1));
        if (FORECAST) {
            l.mu[v] = mean; l.sg[v] = sd;
            if (bad && l.sc[3] == 0.0) l.sc[3] = (double)(k + 1);      // (every lane that writes here in this phase writes k + 1)
        } else {
            const bool lost = l.sc[3] != 0.0;
            const size_t o = ((size_t)wg * a.n_obs + k) * NV + v;
            a.mean_a[o] = lost ? __builtin_nan("") : mean;
            a.sd_a[o] = lost ? __builtin_nan("") : sd;
        }
    }
}

// after the forecast statistics: row k of mean_f / sd_f from the tables (NaN once the point is lost), and the inflation
// about the mean -- elements in their registers and in place in image `cur`, an estimated parameter by its variable's lane
template <int E>
VA_HD void enkf_inflate(const EnkfArgs &a, const EnkfLds &l, int cur, long wg, int tid, int k, EnkfLane<E> &L)
{
    const int NV = a.D + a.NQ;
    const bool lost = l.sc[3] != 0.0, inflate = a.inflation != 1.0;
    for (int v = tid; v < NV; v += a.geo.threads) {
        const size_t o = ((size_t)wg * a.n_obs + k) * NV + v;
        a.mean_f[o] = lost ? __builtin_nan("") : l.mu[v];
        a.sd_f[o] = lost ? __builtin_nan("") : l.sg[v];
        if (inflate && v >= a.D) {
            int stride;
            double *z = enkf_column(a, l, cur, v, &stride);
            const double mean = l.mu[v];
            for (int m = 0; m < a.M; ++m) z[(size_t)m * stride] = mean + a.inflation * (z[(size_t)m * stride] - mean);
        }
    }
    if (inflate) {
        double *xc = l.xs + (size_t)cur * l.img;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const EnkfElem &el = L.el[e];
            if (el.live) {
                const double mean = l.mu[el.col];
                L.x[e] = mean + a.inflation * (L.x[e] - mean);
                xc[el.xoff + el.col] = L.x[e];
            }
        }
    }
}

// observation j = value y of column Lidx[j], first half: the lane of variable i forms hbar, s, d and its own zbar_i, c_i and
// K_i; variable 0's lane leaves hbar, y - hbar and alpha for the elements; an estimated parameter is updated here
VA_HD void enkf_gain(const EnkfArgs &a, const EnkfLds &l, int cur, int tid, int j, double y)
{
    const int NV = a.D + a.NQ, M = a.M, P = a.geo.pitch;
    const double *h = l.xs + (size_t)cur * l.img + a.Lidx[j];
    const double r = a.obs_var[j];
    for (int v = tid; v < NV; v += a.geo.threads) {
        int stride;
        double *z = enkf_column(a, l, cur, v, &stride);
        double hsum = 0.0, zsum = 0.0;
        for (int m = 0; m < M; ++m) { hsum += h[(size_t)m * P]; zsum += z[(size_t)m * stride]; }
        const double hbar = hsum / (double)M, zbar = zsum / (double)M;
        double s = 0.0, c = 0.0;
        for (int m = 0; m < M; ++m) {
            const double am = h[(size_t)m * P] - hbar;
            s += am * am;
            c += (z[(size_t)m * stride] - zbar) * am;
        }
        const double d = s / (double)(M - 1) + r;
        const double K = c / (double)(M - 1) / d;
        const double alpha = 1.0 / (1.0 + sqrt(r / d));
        l.kt[v] = K;
        if (v == 0) { l.sc[0] = hbar; l.sc[1] = y - hbar; l.sc[2] = alpha; }
        if (v >= a.D)
            for (int m = 0; m < M; ++m) z[(size_t)m * stride] += K * (y - hbar) - alpha * K * (h[(size_t)m * P] - hbar);
    }
}

// second half: every element takes its increment; a_m from image `cur`, the updated member into the other image
template <int E>
VA_HD void enkf_update(const EnkfArgs &a, const EnkfLds &l, int cur, int j, EnkfLane<E> &L)
{
    const double *xc = l.xs + (size_t)cur * l.img;
    double *xo = l.xs + (size_t)(cur ^ 1) * l.img;
    const int c = a.Lidx[j];
    const double hbar = l.sc[0], innov = l.sc[1], alpha = l.sc[2];
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const EnkfElem &el = L.el[e];
        if (el.live) {
            const double K = l.kt[el.col], am = xc[el.xoff + c] - hbar;
            L.x[e] += K * innov - alpha * K * am;
            xo[el.xoff + el.col] = L.x[e];
        }
    }
}

// the end: the members from the registers, their parameters from LDS, the status
template <int E>
VA_HD void enkf_store(const EnkfArgs &a, const EnkfLds &l, long wg, int tid, const EnkfLane<E> &L)
{
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const EnkfElem &el = L.el[e];
        if (el.live) a.x_end[(size_t)wg * a.M * a.D + (size_t)(el.xoff / a.geo.pitch) * a.D + el.col] = L.x[e];
    }
    const long np = (long)a.M * a.NP;
    for (long e = tid; e < np; e += a.geo.threads) a.p_end[(size_t)wg * np + e] = l.ps[e];
    if (tid == 0) a.status[wg] = (int)l.sc[3];
}

VA_HD bool enkf_missing(double y) { return y != y; }

// ---------------------------------------------------------------- the same phases, lane by lane on the host
// (every pointer of `a` is host memory; a.geo from plan_enkf)
template <class RHS, int E>
inline void enkf_host_e(const EnkfArgs &a)
{
    const int nt = a.geo.threads;
    const PredictStep hs = predict_step_sizes(a.dt, a.substeps);
    std::vector<double> mem(enkf_lds_doubles(a.M, a.D, a.NP, a.NQ, a.nstim) + 1, 0.0);
    std::vector<EnkfLane<E>> L(nt);
    const EnkfLds l = enkf_lds(a, mem.data());
    for (long wg = 0; wg < a.geo.grid; ++wg) {
        for (int tid = 0; tid < nt; ++tid) enkf_load<E>(a, l, wg, tid, L[tid]);
        long long q = 0;
        int cur = 0, n = 0;
        for (int k = 0; k < a.n_obs; ++k) {
            for (int w = 0; w < a.obs_every; ++w, ++n) {
                if (a.nstim) for (int tid = 0; tid < nt; ++tid) enkf_stim_step<E>(a, tid, n, L[tid]);
                for (int s = 0; s < a.substeps; ++s, ++q) {
                    for (int tid = 0; tid < nt; ++tid) enkf_stim_stage<E, 0>(a, l, tid, s, L[tid]);
                    for (int tid = 0; tid < nt; ++tid) enkf_stage<RHS, E, 0>(a, l, cur, q, hs, L[tid]);
                    for (int tid = 0; tid < nt; ++tid) enkf_stim_stage<E, 1>(a, l, tid, s, L[tid]);
                    for (int tid = 0; tid < nt; ++tid) enkf_stage<RHS, E, 1>(a, l, cur, q, hs, L[tid]);
                    for (int tid = 0; tid < nt; ++tid) enkf_stim_stage<E, 2>(a, l, tid, s, L[tid]);
                    for (int tid = 0; tid < nt; ++tid) enkf_stage<RHS, E, 2>(a, l, cur, q, hs, L[tid]);
                    for (int tid = 0; tid < nt; ++tid) enkf_stim_stage<E, 3>(a, l, tid, s, L[tid]);
                    for (int tid = 0; tid < nt; ++tid) enkf_stage<RHS, E, 3>(a, l, cur, q, hs, L[tid]);
                }
            }
            for (int tid = 0; tid < nt; ++tid) enkf_stats<true>(a, l, cur, wg, tid, k);
            for (int tid = 0; tid < nt; ++tid) enkf_inflate<E>(a, l, cur, wg, tid, k, L[tid]);
            for (int j = 0; j < a.L; ++j) {
                const double y = a.Y[((size_t)wg * a.n_obs + k) * a.L + j];
                if (enkf_missing(y)) continue;
                for (int tid = 0; tid < nt; ++tid) enkf_gain(a, l, cur, tid, j, y);
                for (int tid = 0; tid < nt; ++tid) enkf_update<E>(a, l, cur, j, L[tid]);
                cur ^= 1;
            }
            for (int tid = 0; tid < nt; ++tid) enkf_stats<false>(a, l, cur, wg, tid, k);
        }
        for (int tid = 0; tid < nt; ++tid) enkf_store<E>(a, l, wg, tid, L[tid]);
    }
}

template <class RHS>
inline void enkf_host(const EnkfArgs &a)
{
    switch (a.geo.E) {
    case 1: enkf_host_e<RHS, 1>(a); break;
    case 2: enkf_host_e<RHS, 2>(a); break;
    case 3: enkf_host_e<RHS, 3>(a); break;
    case 4: enkf_host_e<RHS, 4>(a); break;
    case 5: enkf_host_e<RHS, 5>(a); break;
    case 6: enkf_host_e<RHS, 6>(a); break;
    case 7: enkf_host_e<RHS, 7>(a); break;
    default: enkf_host_e<RHS, 8>(a); break;
    }
}

}  // namespace va

// ---------------------------------------------------------------- the kernel
#if defined(__HIPCC__)
#include "va_eval_flat.h"      // wave_sync_lds

namespace va {

template <class RHS, int E, bool WAVE>
__global__ __launch_bounds__(WAVE ? 64 : ENKF_MAX_THREADS) void k_enkf(const EnkfArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double enkf_mem[];
    const EnkfLds l = enkf_lds(a, enkf_mem);
    const int tid = (int)threadIdx.x;
    const long wg = (long)blockIdx.x;
    const PredictStep hs = predict_step_sizes(a.dt, a.substeps);
    EnkfLane<E> L;
    enkf_load<E>(a, l, wg, tid, L);
    long long q = 0;
    int cur = 0, n = 0;
    for (int k = 0; k < a.n_obs; ++k) {
        for (int w = 0; w < a.obs_every; ++w, ++n) {
            if (a.nstim) enkf_stim_step<E>(a, tid, n, L);
            for (int s = 0; s < a.substeps; ++s, ++q) {
                enkf_stim_stage<E, 0>(a, l, tid, s, L); predict_sync<WAVE>(); enkf_stage<RHS, E, 0>(a, l, cur, q, hs, L);
                enkf_stim_stage<E, 1>(a, l, tid, s, L); predict_sync<WAVE>(); enkf_stage<RHS, E, 1>(a, l, cur, q, hs, L);
                enkf_stim_stage<E, 2>(a, l, tid, s, L); predict_sync<WAVE>(); enkf_stage<RHS, E, 2>(a, l, cur, q, hs, L);
                enkf_stim_stage<E, 3>(a, l, tid, s, L); predict_sync<WAVE>(); enkf_stage<RHS, E, 3>(a, l, cur, q, hs, L);
            }
        }
        predict_sync<WAVE>();                  // (the forecast is in image cur)
        enkf_stats<true>(a, l, cur, wg, tid, k);
        predict_sync<WAVE>();                  // (the tables and the status)
        enkf_inflate<E>(a, l, cur, wg, tid, k, L);
        for (int j = 0; j < a.L; ++j) {
            const double y = a.Y[((size_t)wg * a.n_obs + k) * a.L + j];      // (the same for every lane of the workgroup)
            if (enkf_missing(y)) continue;
            predict_sync<WAVE>();              // (the inflated members, or observation j - 1's increments, are in image cur)
            enkf_gain(a, l, cur, tid, j, y);
            predict_sync<WAVE>();
            enkf_update<E>(a, l, cur, j, L);
            cur ^= 1;
        }
        predict_sync<WAVE>();
        enkf_stats<false>(a, l, cur, wg, tid, k);
    }
    enkf_store<E>(a, l, wg, tid, L);
}

// can a model of DC columns (a generated module; 0: any D) run with E elements per lane beside a workgroup barrier: is
// there an ensemble of M >= 2 members with 64 < M DC and 256 (E - 1) < M DC <= 256 E?
constexpr bool enkf_can(int DC, int E)
{
    if (DC == 0) return true;
    for (int M = 2; M * DC <= ENKF_MAX_ELEMS; ++M) {
        const int elems = M * DC;
        if (elems <= 64) continue;
        const int up = ((elems + 63) / 64) * 64, threads = up < ENKF_MAX_THREADS ? up : ENKF_MAX_THREADS;
        if ((elems + threads - 1) / threads == E) return true;
    }
    return false;
}

template <class RHS, int E, int DC>
inline hipError_t launch_enkf_e(const EnkfArgs &a, hipStream_t s)
{
    if constexpr (enkf_can(DC, E)) {
        hipLaunchKernelGGL((k_enkf<RHS, E, false>), dim3((unsigned)a.geo.grid), dim3((unsigned)a.geo.threads), a.geo.lds_bytes, s, a);
        return hipGetLastError();
    }
    return hipErrorInvalidValue;      // (a geometry plan_enkf does not make for this D)
}

// launch the instantiation a.geo names.  DC > 0: the model's D is a constant (a generated module): only the
// instantiations that D can run are compiled (E depends on the number of members of the call as well)
template <class RHS, int DC>
inline hipError_t launch_enkf(const EnkfArgs &a, hipStream_t s)
{
    if (DC > 0 && a.D != DC) return hipErrorInvalidValue;
    EnkfGeo g;
    if (!plan_enkf(a.D, a.T, a.M, a.NP, a.NQ, a.nstim, g)) return hipErrorInvalidValue;
    if (g.threads != a.geo.threads || g.E != a.geo.E || g.wave != a.geo.wave || g.pitch != a.geo.pitch
        || g.lds_bytes != a.geo.lds_bytes || g.grid != a.geo.grid) return hipErrorInvalidValue;
    if (g.wave) {
        if constexpr (DC == 0 || 2 * DC <= 64) {
            hipLaunchKernelGGL((k_enkf<RHS, 1, true>), dim3((unsigned)g.grid), dim3(64), g.lds_bytes, s, a);
            return hipGetLastError();
        }
        return hipErrorInvalidValue;
    }
    switch (g.E) {
    case 1: return launch_enkf_e<RHS, 1, DC>(a, s);
    case 2: return launch_enkf_e<RHS, 2, DC>(a, s);
    case 3: return launch_enkf_e<RHS, 3, DC>(a, s);
    case 4: return launch_enkf_e<RHS, 4, DC>(a, s);
    case 5: return launch_enkf_e<RHS, 5, DC>(a, s);
    case 6: return launch_enkf_e<RHS, 6, DC>(a, s);
    case 7: return launch_enkf_e<RHS, 7, DC>(a, s);
    default: return launch_enkf_e<RHS, 8, DC>(a, s);
    }
}

}  // namespace va
#endif
