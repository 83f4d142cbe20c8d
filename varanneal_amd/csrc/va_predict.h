// va_predict.h -- forecast from estimated states: T trajectories of the model integrated forward with classical RK4.
//
// What a user does after anneal(): integrate the model from the last estimated state with the estimated parameters
// and compare with data held back from the fit.  The reference has no such routine; its examples leave it to the user.
//
// The arithmetic is written once as __host__ __device__ phases of ONE LANE (the pattern of va_core.h): the kernel
// k_predict gives them their parallel decomposition, predict_host drives the same phases lane by lane on the CPU
// (tests/cpu_emul/predict_check.cpp), so the rule, the lane -> column mapping and the LDS layout are covered by the CPU suite.
//
//   step       h = dt_model / substeps;  k1 = f(x), k2 = f(x + h/2 k1), k3 = f(x + h/2 k2), k4 = f(x + h k3),
//              x += h/6 (k1 + 2 k2 + 2 k3 + k4)
//   time       stage offset c = 0, 1/2, 1/2, 1 of sub-step s of model step n:  t0 + (n substeps + s + c) h
//   stimulus   [n_steps + 1][nstim] sampled at the model-step times; at a stage time the rows n and n + 1 are
//              interpolated linearly with weight (s + c) / substeps -- nothing is extrapolated
//   parameters one full vector per trajectory, constant over the forecast
//
// Decomposition (va_predict_geo.h).  Integration is sequential in time: all parallelism is over trajectories and
// columns, and the cost is latency per stage.  A lane owns E columns of one trajectory: their state and their
// k-accumulators live in registers.  f reads its neighbours, so the stage input goes through LDS -- two images, written
// and read in turn, which leaves ONE synchronisation per stage: the write of stage j + 1's input is separated from the
// reads of stage j - 1's by the synchronisation of stage j.
//   D <= 64    one wave per workgroup, RW = 64 / D trajectories side by side (the layout of k_eval4); the
//              synchronisation is the wave's own LDS order, no workgroup barrier
//   D <= 1024  one trajectory per workgroup of min(256, D rounded up to 64) threads, a workgroup barrier per stage
// Global traffic: x0 and p once, one stimulus row per model step (prefetched a step ahead), the output rows.
#pragma once
#include <vector>

#include "va_core.h"
#include "va_predict_geo.h"

namespace va {

struct PredictArgs {
    const double *x0;        // [T][D]
    const double *p;         // [T][NP]
    const double *stim;      // NULL or [n_steps + 1][nstim], shared by the trajectories
    double *out;             // [T][n_out][D]: model steps 0, every, 2 every, ...
    int T, D, NP, nstim, n_steps, substeps, every, n_out;
    double t0, dt;
    PredictGeo geo;
};

struct PredictStep { double h, hh, h6; };      // h, h / 2, h / 6
VA_HD PredictStep predict_step_sizes(double dt, int substeps)
{
    const double h = dt / (double)substeps;
    PredictStep s = {h, 0.5 * h, h / 6.0};
    return s;
}

// what a lane keeps in registers: its columns' state and k-accumulators, and its stimulus column at the rows n, n + 1
// and (prefetched) n + 2
template <int E> struct PredictLane {
    double x[E], acc[E];
    double g0, g1, gn;
};

// a lane's place: its trajectory, its slot in the workgroup and its first column; Dl = D, or 0 for a lane without a trajectory
struct PredictCtx { int tid, slot, col0, Dl, cstride; long traj; };
VA_HD PredictCtx predict_ctx(const PredictArgs &a, long wg, int tid)
{
    PredictCtx c;
    c.tid = tid; c.cstride = a.geo.threads;
    predict_lane(a.geo, a.D, tid, &c.slot, &c.col0);
    c.traj = wg * a.geo.RW + c.slot;
    const bool live = c.slot < a.geo.RW && c.traj < a.T;
    c.Dl = live ? a.D : 0;
    if (!live) { c.slot = 0; c.traj = 0; }         // (addresses formed from them are never used)
    return c;
}

// the workgroup's LDS: stage inputs [2][RW][D], parameters [RW][NP], interpolated stimulus [2][nstim]
struct PredictLds { double *xs, *ps, *sts; };
VA_HD PredictLds predict_lds(const PredictArgs &a, double *base)
{
    PredictLds l;
    l.xs = base; l.ps = l.xs + 2 * (size_t)a.geo.RW * a.D; l.sts = l.ps + (size_t)a.geo.RW * a.NP;
    return l;
}

template <int STAGE> VA_HD double predict_c() { return STAGE == 0 ? 0.0 : (STAGE == 3 ? 1.0 : 0.5); }
// q = n substeps + s: sub-steps taken so far
VA_HD double predict_time(double t0, long long q, double c, double h) { return t0 + ((double)q + c) * h; }
VA_HD double predict_interp(double a0, double a1, double w) { return (1.0 - w) * a0 + w * a1; }

template <class RHS>
VA_HD double predict_f(const double *x, int i, int D, const double *p, double t, const double *st)
{
    double fv = RHS::f(x, i, D, p, t, st);
    if constexpr (rhs_linear<RHS>::value) {          // (the generator split a dense constant linear part off: va_core.h)
        const double *A0 = RHS::lin_A0();
        for (int j = 0; j < D; ++j) fv += A0[i * RHS::LIN_DP + j] * x[j];
    }
    return fv;
}

// phase 0: x0 into the registers, the first stage input and output row 0 (x0 itself); the workgroup's parameters;
// the lane's stimulus column at rows 0 and 1
template <int E>
VA_HD void predict_load(const PredictArgs &a, const PredictCtx &c, const PredictLds &l, long wg, PredictLane<E> &L)
{
    const double *x0 = a.x0 + (size_t)c.traj * a.D;
    double *out = a.out + (size_t)c.traj * a.n_out * a.D;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = c.col0 + e * c.cstride;
        L.x[e] = 0.0; L.acc[e] = 0.0;
        if (i < c.Dl) {
            L.x[e] = x0[i];
            l.xs[(size_t)c.slot * a.D + i] = L.x[e];
            out[i] = L.x[e];
        }
    }
    // (the trajectories of a workgroup are neighbours in p as they are in the LDS image)
    const long np = (long)a.geo.RW * a.NP, first = wg * np, all = (long)a.T * a.NP;
    for (long e = c.tid; e < np; e += c.cstride) l.ps[e] = first + e < all ? a.p[first + e] : 0.0;
    L.g0 = 0.0; L.g1 = 0.0; L.gn = 0.0;
    if (c.tid < a.nstim) { L.g1 = a.stim[c.tid]; L.gn = a.stim[a.nstim + c.tid]; }
}

// start of model step n: the lane's stimulus column moves on one row; row n + 2 is asked for a step ahead of its use
template <int E>
VA_HD void predict_stim_step(const PredictArgs &a, const PredictCtx &c, int n, PredictLane<E> &L)
{
    L.g0 = L.g1; L.g1 = L.gn;
    if (c.tid < a.nstim && n + 2 <= a.n_steps) L.gn = a.stim[(size_t)(n + 2) * a.nstim + c.tid];
}

// before the synchronisation of a stage: the stimulus at the stage's time into the image the stage reads
template <int E, int STAGE>
VA_HD void predict_stim_stage(const PredictArgs &a, const PredictCtx &c, const PredictLds &l, int s, PredictLane<E> &L)
{
    constexpr int in = STAGE & 1;
    if (c.tid < a.nstim)
        l.sts[in * a.nstim + c.tid] = predict_interp(L.g0, L.g1, ((double)s + predict_c<STAGE>()) / (double)a.substeps);
}

// after it: k = f(stage input) for the lane's columns; the next stage's input -- after the fourth stage the new state,
// which is the first input of the next sub-step -- into the other image
template <class RHS, int E, int STAGE>
VA_HD void predict_stage(const PredictArgs &a, const PredictCtx &c, const PredictLds &l, long long q, const PredictStep &hs, PredictLane<E> &L)
{
    constexpr int in = STAGE & 1;
    const int D = a.D;
    const double *xin = l.xs + ((size_t)in * a.geo.RW + c.slot) * D;
    double *xout = l.xs + ((size_t)(in ^ 1) * a.geo.RW + c.slot) * D;
    const double *p = l.ps + (size_t)c.slot * a.NP;
    const double t = predict_time(a.t0, q, predict_c<STAGE>(), hs.h);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = c.col0 + e * c.cstride;
        if (i < c.Dl) {
            const double k = predict_f<RHS>(xin, i, D, p, t, l.sts + in * a.nstim);
            if (STAGE == 0) { L.acc[e] = k; xout[i] = L.x[e] + hs.hh * k; }
            else if (STAGE == 1) { L.acc[e] += 2.0 * k; xout[i] = L.x[e] + hs.hh * k; }
            else if (STAGE == 2) { L.acc[e] += 2.0 * k; xout[i] = L.x[e] + hs.h * k; }
            else { L.acc[e] += k; L.x[e] += hs.h6 * L.acc[e]; xout[i] = L.x[e]; }
        }
    }
}

// the state after a model step that is to be kept: output row `row`
template <int E>
VA_HD void predict_store(const PredictArgs &a, const PredictCtx &c, size_t row, const PredictLane<E> &L)
{
    double *out = a.out + ((size_t)c.traj * a.n_out + row) * a.D;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const int i = c.col0 + e * c.cstride;
        if (i < c.Dl) out[i] = L.x[e];
    }
}

// ---------------------------------------------------------------- the same phases, lane by lane on the host
// (every pointer of `a` is host memory; a.geo from plan_predict)
template <class RHS, int E>
inline void predict_host_e(const PredictArgs &a)
{
    const int nt = a.geo.threads;
    const PredictStep hs = predict_step_sizes(a.dt, a.substeps);
    std::vector<double> mem(predict_lds_doubles(a.geo.RW, a.D, a.NP, a.nstim) + 1, 0.0);
    std::vector<PredictLane<E>> L(nt);
    std::vector<PredictCtx> c(nt);
    const PredictLds l = predict_lds(a, mem.data());
    for (long wg = 0; wg < a.geo.grid; ++wg) {
        for (int tid = 0; tid < nt; ++tid) { c[tid] = predict_ctx(a, wg, tid); predict_load<E>(a, c[tid], l, wg, L[tid]); }
        long long q = 0;
        int until_out = a.every;
        size_t row = 1;
        for (int n = 0; n < a.n_steps; ++n) {
            if (a.nstim) for (int tid = 0; tid < nt; ++tid) predict_stim_step<E>(a, c[tid], n, L[tid]);
            for (int s = 0; s < a.substeps; ++s, ++q) {
                for (int tid = 0; tid < nt; ++tid) predict_stim_stage<E, 0>(a, c[tid], l, s, L[tid]);
                for (int tid = 0; tid < nt; ++tid) predict_stage<RHS, E, 0>(a, c[tid], l, q, hs, L[tid]);
                for (int tid = 0; tid < nt; ++tid) predict_stim_stage<E, 1>(a, c[tid], l, s, L[tid]);
                for (int tid = 0; tid < nt; ++tid) predict_stage<RHS, E, 1>(a, c[tid], l, q, hs, L[tid]);
                for (int tid = 0; tid < nt; ++tid) predict_stim_stage<E, 2>(a, c[tid], l, s, L[tid]);
                for (int tid = 0; tid < nt; ++tid) predict_stage<RHS, E, 2>(a, c[tid], l, q, hs, L[tid]);
                for (int tid = 0; tid < nt; ++tid) predict_stim_stage<E, 3>(a, c[tid], l, s, L[tid]);
                for (int tid = 0; tid < nt; ++tid) predict_stage<RHS, E, 3>(a, c[tid], l, q, hs, L[tid]);
            }
            if (--until_out == 0) {
                until_out = a.every;
                for (int tid = 0; tid < nt; ++tid) predict_store<E>(a, c[tid], row, L[tid]);
                ++row;
            }
        }
    }
}

template <class RHS>
inline void predict_host(const PredictArgs &a)
{
    switch (a.geo.E) {
    case 1: predict_host_e<RHS, 1>(a); break;
    case 2: predict_host_e<RHS, 2>(a); break;
    case 3: predict_host_e<RHS, 3>(a); break;
    default: predict_host_e<RHS, 4>(a); break;
    }
}

}  // namespace va

// ---------------------------------------------------------------- the kernel
#if defined(__HIPCC__)
#include "va_eval_flat.h"      // wave_sync_lds

namespace va {

template <bool WAVE> __device__ __forceinline__ void predict_sync()
{
    if (WAVE) wave_sync_lds();      // lanes of ONE wave exchange the stage input: LDS is in order within a wave
    else __syncthreads();
}

template <class RHS, int E, bool WAVE>
__global__ __launch_bounds__(WAVE ? 64 : 256) void k_predict(const PredictArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double predict_mem[];
    const PredictLds l = predict_lds(a, predict_mem);
    const PredictCtx c = predict_ctx(a, (long)blockIdx.x, (int)threadIdx.x);
    const PredictStep hs = predict_step_sizes(a.dt, a.substeps);
    PredictLane<E> L;
    predict_load<E>(a, c, l, (long)blockIdx.x, L);
    long long q = 0;
    int until_out = a.every;
    size_t row = 1;
    for (int n = 0; n < a.n_steps; ++n) {
        if (a.nstim) predict_stim_step<E>(a, c, n, L);
        for (int s = 0; s < a.substeps; ++s, ++q) {
            predict_stim_stage<E, 0>(a, c, l, s, L); predict_sync<WAVE>(); predict_stage<RHS, E, 0>(a, c, l, q, hs, L);
            predict_stim_stage<E, 1>(a, c, l, s, L); predict_sync<WAVE>(); predict_stage<RHS, E, 1>(a, c, l, q, hs, L);
            predict_stim_stage<E, 2>(a, c, l, s, L); predict_sync<WAVE>(); predict_stage<RHS, E, 2>(a, c, l, q, hs, L);
            predict_stim_stage<E, 3>(a, c, l, s, L); predict_sync<WAVE>(); predict_stage<RHS, E, 3>(a, c, l, q, hs, L);
        }
        if (--until_out == 0) {
            until_out = a.every;
            predict_store<E>(a, c, row, L);
            ++row;
        }
    }
}

// launch the instantiation a.geo names.  DC > 0: the model's D is a constant (a generated module): only the
// instantiation that D runs is compiled
template <class RHS, int DC>
inline hipError_t launch_predict(const PredictArgs &a, hipStream_t s)
{
    const dim3 grid((unsigned)a.geo.grid), block((unsigned)a.geo.threads);
    constexpr int EC = DC <= 64 ? 1 : (DC + 255) / 256;      // (the only E a module's D can have)
    if (DC > 0 && (a.D != DC || a.geo.E != EC)) return hipErrorInvalidValue;
    if (a.geo.wave) {
        if constexpr (DC == 0 || DC <= 64) hipLaunchKernelGGL((k_predict<RHS, 1, true>), grid, block, a.geo.lds_bytes, s, a);
    } else if (a.geo.E == 1) {
        if constexpr (DC == 0 || (DC > 64 && EC == 1)) hipLaunchKernelGGL((k_predict<RHS, 1, false>), grid, block, a.geo.lds_bytes, s, a);
    } else if (a.geo.E == 2) {
        if constexpr (DC == 0 || (DC > 64 && EC == 2)) hipLaunchKernelGGL((k_predict<RHS, 2, false>), grid, block, a.geo.lds_bytes, s, a);
    } else if (a.geo.E == 3) {
        if constexpr (DC == 0 || (DC > 64 && EC == 3)) hipLaunchKernelGGL((k_predict<RHS, 3, false>), grid, block, a.geo.lds_bytes, s, a);
    } else {
        if constexpr (DC == 0 || (DC > 64 && EC == 4)) hipLaunchKernelGGL((k_predict<RHS, 4, false>), grid, block, a.geo.lds_bytes, s, a);
    }
    return hipGetLastError();
}

}  // namespace va
#endif
