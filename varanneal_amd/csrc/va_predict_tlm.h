// va_predict_tlm.h -- forecast spread: the tangent-linear model of the RK4 predictor (va_predict.h), and the reduction of
// its tangents to variances and same-time covariance blocks.
//
// For T trajectories, each with nvec tangent directions v = [v_x (D) | v_p (NPest)], the nominal trajectory is integrated
// exactly as k_predict does it, and with it the exact derivative of the DISCRETE RK4 map along every direction:
//     k1 = f(x)            k1' = jvp(x;            v_x,             v_p)
//     k2 = f(x + h/2 k1)   k2' = jvp(x + h/2 k1;   v_x + h/2 k1',   v_p)
//     k3 = f(x + h/2 k2)   k3' = jvp(x + h/2 k2;   v_x + h/2 k2',   v_p)
//     k4 = f(x + h k3)     k4' = jvp(x + h k3;     v_x + h k3',     v_p)
//     x   += h/6 (k1 + 2 k2 + 2 k3 + k4)           v_x += h/6 (k1' + 2 k2' + 2 k3' + k4')        v_p constant
// with jvp(x; v, q) = J(x) v + (df/dp) q = RHS::jvp (the term va_hvp.h calls fdot).  Stage times, stimulus interpolation,
// substeps and every are va_predict.h's; the stimulus is known, so it has no tangent.  v_p is scattered into a full-length
// parameter tangent through the handle's Pidx (zero where a parameter is not estimated), as hvp_ctx does it.
//
// When the directions of a trajectory are the columns of a square root S of the covariance Sigma_0 of (x0, p_est), the
// sums over directions  var_n,i = sum_c dX_c,n,i^2  and  cov_n,ij = sum_c dX_c,n,i dX_c,n,j  (k_spread) are the linearised
// forecast covariance M_n Sigma_0 M_n^T.
//
// Like va_predict.h the arithmetic is written once as __host__ __device__ phases of ONE LANE; k_predict_tlm gives them
// their decomposition (va_predict_tlm_geo.h), predict_tlm_host drives them lane by lane on the CPU
// (tests/cpu_emul/predict_tlm_check.cpp).  A lane owns E elements (slot, column) of its workgroup: slot 0 of a trajectory
// is the nominal state, slots 1 .. chunk are tangents.  State, tangents and k-accumulators live in registers; the stage
// inputs of all slots go through two LDS images written and read in turn, ONE synchronisation per stage (va_predict.h
// says why one is enough).  A tangent element reads its own slot's image and the nominal's.
#pragma once
#include <vector>

#include "va_core.h"
#include "va_predict.h"
#include "va_predict_tlm_geo.h"

namespace va {

struct PredictTlmArgs {
    const double *x0;        // [T][D]
    const double *p;         // [T][NP]
    const double *V0;        // [T][nvec][D + NPest]
    const double *stim;      // NULL or [n_steps + 1][nstim], shared by the trajectories
    const int *Pidx;         // [NPest]: where an estimated parameter sits in the full vector
    double *out;             // [T][n_out][D]: the nominal trajectory
    double *dX;              // [T][nvec][n_out][D]: the tangents' state parts (NULL: not stored)
    int T, D, NP, NPest, nvec, nstim, n_steps, substeps, every, n_out;
    double t0, dt;
    PredictTlmGeo geo;
};

// one element of a lane: kind 0 nobody's, 1 nominal, 2 tangent
struct PredictTlmElem {
    int kind, col;
    int xoff, noff;          // the element's slot and its trajectory's nominal slot in a stage image (doubles)
    int poff, qoff;          // the trajectory's parameters, the direction's parameter tangent
    double *g;               // row 0 of the element's output column (NULL: not stored)
};

template <int E> struct PredictTlmLane {
    double x[E], acc[E];     // state or tangent, and its k-accumulator
    double g0, g1, gn;       // the lane's stimulus column at the rows n, n + 1 and (prefetched) n + 2
    PredictTlmElem el[E];
};

// the workgroup's LDS: stage inputs [2][img], parameters [RW][NP], parameter tangents [RW][chunk][NP], stimulus [2][nstim]
struct PredictTlmLds { double *xs, *ps, *qs, *sts; int img; };
VA_HD PredictTlmLds predict_tlm_lds(const PredictTlmArgs &a, double *base)
{
    PredictTlmLds l;
    l.img = a.geo.RW * (a.geo.chunk + 1) * a.D;
    l.xs = base; l.ps = l.xs + 2 * (size_t)l.img; l.qs = l.ps + (size_t)a.geo.RW * a.NP;
    l.sts = l.qs + (size_t)a.geo.RW * a.geo.chunk * a.NP;
    return l;
}

// workgroup wg = (trajectory group, chunk of directions)
struct PredictTlmWork { long group; int ck; };
VA_HD PredictTlmWork predict_tlm_work(const PredictTlmArgs &a, long wg)
{
    PredictTlmWork w;
    w.group = wg / a.geo.nchunks; w.ck = (int)(wg - w.group * a.geo.nchunks);
    return w;
}

// phase 0: the lane's elements, their start values (x0 / V0's state part) into the registers, the first stage input and
// output row 0; the workgroup's parameters and parameter tangents; the lane's stimulus column at rows 0 and 1
template <int E>
VA_HD void predict_tlm_load(const PredictTlmArgs &a, const PredictTlmLds &l, long wg, int tid, PredictTlmLane<E> &L)
{
    const PredictTlmGeo &g = a.geo;
    const PredictTlmWork w = predict_tlm_work(a, wg);
    const int D = a.D, nw = D + a.NPest;
    const size_t rowD = (size_t)a.n_out * D;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        PredictTlmElem &el = L.el[e];
        int r, s;
        predict_tlm_elem(g, D, tid + e * g.threads, &r, &s, &el.col);
        const long traj = w.group * g.RW + r;
        const int dir = w.ck * g.chunk + s - 1;
        el.kind = (r < g.RW && traj < a.T) ? (s == 0 ? 1 : (dir < a.nvec ? 2 : 0)) : 0;
        el.noff = r * (g.chunk + 1) * D; el.xoff = el.noff + s * D;
        el.poff = r * a.NP; el.qoff = (r * g.chunk + (s > 0 ? s - 1 : 0)) * a.NP;
        el.g = nullptr;
        L.x[e] = 0.0; L.acc[e] = 0.0;
        if (el.kind == 1) {
            L.x[e] = a.x0[(size_t)traj * D + el.col];
            if (w.ck == 0) el.g = a.out + (size_t)traj * rowD + el.col;       // (the other chunks recompute it and keep it to themselves)
        } else if (el.kind == 2) {
            L.x[e] = a.V0[((size_t)traj * a.nvec + dir) * nw + el.col];
            if (a.dX) el.g = a.dX + ((size_t)traj * a.nvec + dir) * rowD + el.col;
        }
        if (el.kind) {
            l.xs[el.xoff + el.col] = L.x[e];
            if (el.g) el.g[0] = L.x[e];
        }
    }
    // parameters: the trajectories of a workgroup are neighbours in p as they are in the LDS image
    const long np = (long)g.RW * a.NP, first = w.group * np, all = (long)a.T * a.NP;
    for (long e = tid; e < np; e += g.threads) l.ps[e] = first + e < all ? a.p[first + e] : 0.0;
    // parameter tangents: one lane per (trajectory, direction) of the workgroup zeroes the full-length vector and scatters v_p
    for (int rd = tid; rd < g.RW * g.chunk; rd += g.threads) {
        const int r = rd / g.chunk, s1 = rd - r * g.chunk;
        const long traj = w.group * g.RW + r;
        const int dir = w.ck * g.chunk + s1;
        double *q = l.qs + (size_t)rd * a.NP;
        for (int k = 0; k < a.NP; ++k) q[k] = 0.0;
        if (traj < a.T && dir < a.nvec) {
            const double *vp = a.V0 + ((size_t)traj * a.nvec + dir) * nw + D;
            for (int k = 0; k < a.NPest; ++k) q[a.Pidx[k]] = vp[k];
        }
    }
    L.g0 = 0.0; L.g1 = 0.0; L.gn = 0.0;
    if (tid < a.nstim) { L.g1 = a.stim[tid]; L.gn = a.stim[a.nstim + tid]; }
}

// start of model step n: the lane's stimulus column moves on one row; row n + 2 is asked for a step ahead of its use
template <int E>
VA_HD void predict_tlm_stim_step(const PredictTlmArgs &a, int tid, int n, PredictTlmLane<E> &L)
{
    L.g0 = L.g1; L.g1 = L.gn;
    if (tid < a.nstim && n + 2 <= a.n_steps) L.gn = a.stim[(size_t)(n + 2) * a.nstim + tid];
}

// before the synchronisation of a stage: the stimulus at the stage's time into the image the stage reads
template <int E, int STAGE>
VA_HD void predict_tlm_stim_stage(const PredictTlmArgs &a, const PredictTlmLds &l, int tid, int s, const PredictTlmLane<E> &L)
{
    constexpr int in = STAGE & 1;
    if (tid < a.nstim)
        l.sts[in * a.nstim + tid] = predict_interp(L.g0, L.g1, ((double)s + predict_c<STAGE>()) / (double)a.substeps);
}

// after it: k = f(stage input) for a nominal element, k' = jvp(nominal stage input; tangent stage input, v_p) for a tangent;
// the next stage's input into the other image (va_predict.h predict_stage: the same update for both kinds)
template <class RHS, int E, int STAGE>
VA_HD void predict_tlm_stage(const PredictTlmArgs &a, const PredictTlmLds &l, long long q, const PredictStep &hs, PredictTlmLane<E> &L)
{
    constexpr int in = STAGE & 1;
    const int D = a.D;
    const double *xin = l.xs + (size_t)in * l.img;
    double *xout = l.xs + (size_t)(in ^ 1) * l.img;
    const double *st = l.sts + in * a.nstim;
    const double t = predict_time(a.t0, q, predict_c<STAGE>(), hs.h);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const PredictTlmElem &el = L.el[e];
        if (el.kind) {
            const double k = el.kind == 1 ? predict_f<RHS>(xin + el.noff, el.col, D, l.ps + el.poff, t, st)
                                          : RHS::jvp(xin + el.noff, xin + el.xoff, l.qs + el.qoff, el.col, D, l.ps + el.poff, t, st);
            double *xo = xout + el.xoff + el.col;
            if (STAGE == 0) { L.acc[e] = k; *xo = L.x[e] + hs.hh * k; }
            else if (STAGE == 1) { L.acc[e] += 2.0 * k; *xo = L.x[e] + hs.hh * k; }
            else if (STAGE == 2) { L.acc[e] += 2.0 * k; *xo = L.x[e] + hs.h * k; }
            else { L.acc[e] += k; L.x[e] += hs.h6 * L.acc[e]; *xo = L.x[e]; }
        }
    }
}

// the state and the tangents after a model step that is to be kept: output row `row`
template <int E>
VA_HD void predict_tlm_store(const PredictTlmArgs &a, size_t row, const PredictTlmLane<E> &L)
{
#pragma unroll
    for (int e = 0; e < E; ++e)
        if (L.el[e].g) L.el[e].g[row * a.D] = L.x[e];
}

// ---------------------------------------------------------------- the reduction over directions
struct SpreadArgs {
    const double *dX;        // [T][nvec][n_out][D]
    double *var;             // [T][n_out][D], or NULL
    double *cov;             // [T][n_out][D][D], or NULL
    int T, nvec, n_out, D;
};

// products and sums as written, in direction order, never contracted: the bits of the same loop in NumPy, on every call
VA_HD double spread_sum(const double *a, const double *b, int nvec, size_t pitch)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double s = 0.0;
    for (int c = 0; c < nvec; ++c) {
        const double pr = a[c * pitch] * b[c * pitch];
        s = s + pr;
    }
    return s;
}

// entry e of the variances ([T][n_out][D]) / of the covariance blocks ([T][n_out][D][D])
VA_HD void spread_var_entry(const SpreadArgs &a, size_t e)
{
    const size_t row = (size_t)a.n_out * a.D, t = e / row, ni = e - t * row;
    const double *d = a.dX + t * a.nvec * row + ni;
    a.var[e] = spread_sum(d, d, a.nvec, row);
}
VA_HD void spread_cov_entry(const SpreadArgs &a, size_t e)
{
    const size_t D = a.D, row = (size_t)a.n_out * D, j = e % D, tni = e / D, t = tni / row, ni = tni - t * row, n = ni / D;
    const double *d = a.dX + t * a.nvec * row;
    a.cov[e] = spread_sum(d + ni, d + n * D + j, a.nvec, row);
}
inline void spread_host(const SpreadArgs &a)
{
    const size_t nv = (size_t)a.T * a.n_out * a.D;
    if (a.var) for (size_t e = 0; e < nv; ++e) spread_var_entry(a, e);
    if (a.cov) for (size_t e = 0; e < nv * a.D; ++e) spread_cov_entry(a, e);
}

// ---------------------------------------------------------------- the same phases, lane by lane on the host
// (every pointer of `a` is host memory; a.geo from plan_predict_tlm)
template <class RHS, int E>
inline void predict_tlm_host_e(const PredictTlmArgs &a)
{
    const int nt = a.geo.threads;
    const PredictStep hs = predict_step_sizes(a.dt, a.substeps);
    std::vector<double> mem(predict_tlm_lds_doubles(a.geo.RW, a.geo.chunk, a.D, a.NP, a.nstim) + 1, 0.0);
    std::vector<PredictTlmLane<E>> L(nt);
    const PredictTlmLds l = predict_tlm_lds(a, mem.data());
    for (long wg = 0; wg < a.geo.grid; ++wg) {
        for (int tid = 0; tid < nt; ++tid) predict_tlm_load<E>(a, l, wg, tid, L[tid]);
        long long q = 0;
        int until_out = a.every;
        size_t row = 1;
        for (int n = 0; n < a.n_steps; ++n) {
            if (a.nstim) for (int tid = 0; tid < nt; ++tid) predict_tlm_stim_step<E>(a, tid, n, L[tid]);
            for (int s = 0; s < a.substeps; ++s, ++q) {
                for (int tid = 0; tid < nt; ++tid) predict_tlm_stim_stage<E, 0>(a, l, tid, s, L[tid]);
                for (int tid = 0; tid < nt; ++tid) predict_tlm_stage<RHS, E, 0>(a, l, q, hs, L[tid]);
                for (int tid = 0; tid < nt; ++tid) predict_tlm_stim_stage<E, 1>(a, l, tid, s, L[tid]);
                for (int tid = 0; tid < nt; ++tid) predict_tlm_stage<RHS, E, 1>(a, l, q, hs, L[tid]);
                for (int tid = 0; tid < nt; ++tid) predict_tlm_stim_stage<E, 2>(a, l, tid, s, L[tid]);
                for (int tid = 0; tid < nt; ++tid) predict_tlm_stage<RHS, E, 2>(a, l, q, hs, L[tid]);
                for (int tid = 0; tid < nt; ++tid) predict_tlm_stim_stage<E, 3>(a, l, tid, s, L[tid]);
                for (int tid = 0; tid < nt; ++tid) predict_tlm_stage<RHS, E, 3>(a, l, q, hs, L[tid]);
            }
            if (--until_out == 0) {
                until_out = a.every;
                for (int tid = 0; tid < nt; ++tid) predict_tlm_store<E>(a, row, L[tid]);
                ++row;
            }
        }
    }
}

template <class RHS>
inline void predict_tlm_host(const PredictTlmArgs &a)
{
    switch (a.geo.E) {
    case 1: predict_tlm_host_e<RHS, 1>(a); break;
    case 2: predict_tlm_host_e<RHS, 2>(a); break;
    case 3: predict_tlm_host_e<RHS, 3>(a); break;
    case 4: predict_tlm_host_e<RHS, 4>(a); break;
    case 5: predict_tlm_host_e<RHS, 5>(a); break;
    case 6: predict_tlm_host_e<RHS, 6>(a); break;
    case 7: predict_tlm_host_e<RHS, 7>(a); break;
    default: predict_tlm_host_e<RHS, 8>(a); break;
    }
}

}  // namespace va

// ---------------------------------------------------------------- the kernels
#if defined(__HIPCC__)
#include "va_eval_flat.h"      // wave_sync_lds

namespace va {

template <class RHS, int E, bool WAVE>
__global__ __launch_bounds__(WAVE ? 64 : 256) void k_predict_tlm(const PredictTlmArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double predict_tlm_mem[];
    const PredictTlmLds l = predict_tlm_lds(a, predict_tlm_mem);
    const int tid = (int)threadIdx.x;
    const PredictStep hs = predict_step_sizes(a.dt, a.substeps);
    PredictTlmLane<E> L;
    predict_tlm_load<E>(a, l, (long)blockIdx.x, tid, L);
    long long q = 0;
    int until_out = a.every;
    size_t row = 1;
    for (int n = 0; n < a.n_steps; ++n) {
        if (a.nstim) predict_tlm_stim_step<E>(a, tid, n, L);
        for (int s = 0; s < a.substeps; ++s, ++q) {
            predict_tlm_stim_stage<E, 0>(a, l, tid, s, L); predict_sync<WAVE>(); predict_tlm_stage<RHS, E, 0>(a, l, q, hs, L);
            predict_tlm_stim_stage<E, 1>(a, l, tid, s, L); predict_sync<WAVE>(); predict_tlm_stage<RHS, E, 1>(a, l, q, hs, L);
            predict_tlm_stim_stage<E, 2>(a, l, tid, s, L); predict_sync<WAVE>(); predict_tlm_stage<RHS, E, 2>(a, l, q, hs, L);
            predict_tlm_stim_stage<E, 3>(a, l, tid, s, L); predict_sync<WAVE>(); predict_tlm_stage<RHS, E, 3>(a, l, q, hs, L);
        }
        if (--until_out == 0) {
            until_out = a.every;
            predict_tlm_store<E>(a, row, L);
            ++row;
        }
    }
}

// one thread per entry of cov and, the first of them, of var.  (A template: the header enters several translation units.)
template <int NT>
__global__ __launch_bounds__(NT) void k_spread(const SpreadArgs a)
{
    const size_t nv = (size_t)a.T * a.n_out * a.D, nc = a.cov ? nv * a.D : 0;
    const size_t e = (size_t)blockIdx.x * NT + threadIdx.x;
    if (e < nc) spread_cov_entry(a, e);
    if (a.var && e < nv) spread_var_entry(a, e);
}

inline hipError_t launch_spread(const SpreadArgs &a, hipStream_t s)
{
    const size_t nv = (size_t)a.T * a.n_out * a.D, n = a.cov ? nv * a.D : nv;
    if (!a.var && !a.cov) return hipSuccess;
    if ((n + 255) / 256 > 2147483647UL) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_spread<256>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

// launch the instantiation a.geo names.  DC > 0: the model's D is a constant (a generated module): only the
// instantiations that D can run are compiled (E depends on the number of directions of the call as well)
template <class RHS, int E, int DC>
inline hipError_t launch_predict_tlm_e(const PredictTlmArgs &a, hipStream_t s)
{
    // (a workgroup has at least the 2 D elements of the nominal and one direction; past D = 512 exactly those)
    constexpr bool can = DC == 0 || (DC > 32 && 2 * DC <= 256 * E && (DC <= 512 ? E <= PREDICT_MAX_E : 2 * DC > 256 * (E - 1)));
    if constexpr (can) {
        hipLaunchKernelGGL((k_predict_tlm<RHS, E, false>), dim3((unsigned)a.geo.grid), dim3((unsigned)a.geo.threads), a.geo.lds_bytes, s, a);
        return hipGetLastError();
    }
    return hipErrorInvalidValue;      // (a geometry plan_predict_tlm does not make for this D)
}

template <class RHS, int DC>
inline hipError_t launch_predict_tlm(const PredictTlmArgs &a, hipStream_t s)
{
    if (DC > 0 && a.D != DC) return hipErrorInvalidValue;
    if (a.geo.wave != (2 * a.D <= 64 ? 1 : 0) || a.geo.E < 1 || a.geo.E > PREDICT_TLM_MAX_E) return hipErrorInvalidValue;
    if (a.geo.wave) {
        if constexpr (DC == 0 || 2 * DC <= 64) {
            if (a.geo.E != 1 || a.geo.threads != 64) return hipErrorInvalidValue;
            hipLaunchKernelGGL((k_predict_tlm<RHS, 1, true>), dim3((unsigned)a.geo.grid), dim3(64), a.geo.lds_bytes, s, a);
            return hipGetLastError();
        }
        return hipErrorInvalidValue;
    }
    switch (a.geo.E) {
    case 1: return launch_predict_tlm_e<RHS, 1, DC>(a, s);
    case 2: return launch_predict_tlm_e<RHS, 2, DC>(a, s);
    case 3: return launch_predict_tlm_e<RHS, 3, DC>(a, s);
    case 4: return launch_predict_tlm_e<RHS, 4, DC>(a, s);
    case 5: return launch_predict_tlm_e<RHS, 5, DC>(a, s);
    case 6: return launch_predict_tlm_e<RHS, 6, DC>(a, s);
    case 7: return launch_predict_tlm_e<RHS, 7, DC>(a, s);
    default: return launch_predict_tlm_e<RHS, 8, DC>(a, s);
    }
}

}  // namespace va
#endif
