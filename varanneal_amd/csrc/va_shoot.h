// va_shoot.h -- strong-constraint shooting on the device: for T points (x0, p) the whole unbounded L-BFGS minimisation of the
// misfit  cost(x0, p_est) = sum_l w_l (x_l(t; x0, p) - y_l)^2  of the model's RK4 trajectory, in ONE launch.
//
// A workgroup carries the points plan_predict_adj gives it in misfit mode (va_shoot_geo.h) and loops over evaluations:
//   a. evaluate   cost, gx0 and gp of every point's trial (x0, p) with va_predict_adj.h's own phases, in their order: the
//                 load phase runs again every time (stimulus lanes, zeroed partials and cost shares, image 0 of xs), the
//                 nominal trajectory is not stored (the lanes' output pointers are cleared after the load), and the finish
//                 phase's results land in the workgroup's part of the workspace.  Checkpoints: one set per workgroup.
//   b. step       lane r of the workgroup owns point r: it reads the evaluation and moves the point's minimiser on --
//                 what SciPy's L-BFGS-B does without bounds, as the ladder minimiser does it (va_core.h ls_step): dcsrch with
//                 ftol 1e-3, gtol 0.9, xtol 0.1, first step min(1 / |g|, 1e10), then 1; the pair is kept when
//                 dr > epsmch ddum; a failed search restarts from the iterate with emptied memory, status 2 if it was
//                 empty; stops in SciPy's order (maxiter, maxfun, max|g| <= gtol, f_old - f <= ftol max(|f_old|, |f|, 1)).
//                 The direction is the two-loop recursion over the stored pairs with H0 = (s.y / y.y) I, the same matrix
//                 as L-BFGS-B's compact form.  Every loop runs over the n = D + NPest variables in index order on that one
//                 lane: no atomics, no tree whose shape depends on the geometry -- the same bits every call, and whoever a
//                 point shares a wave with.  The next trial goes to the point's (x0, p) in global memory.
//   c. end        a finished point is frozen: its lanes still walk the phases (the synchronisations are the workgroup's), its
//                 (x0, p) and state no longer change.  The loop ends when every point's flag in LDS is set, read after a
//                 synchronisation, and at the latest after maxfun + 2 trips, a bound the launch knows.
// Two things differ from SciPy's driver, both on purpose.  A search that still wants a trial once nfev > maxfun stops with
// status 1 at the iterate (SciPy tests the budget only between iterations): nfev <= maxfun + 1.  A cost that is not finite
// ends a search as a failed one, and at the first evaluation returns the point unchanged with status 3.
//
// The step is __host__ __device__ code of one lane like the evaluation; shoot_host drives both lane by lane on the CPU
// (tests/cpu_emul/shoot_check.cpp).
#pragma once
#include <vector>

#include "va_predict_adj.h"
#include "va_shoot_geo.h"

namespace va {

struct ShootArgs {
    PredictAdjArgs adj;      // misfit mode, ncot = 1.  x0, p: the trial points (x, p below); out NULL; gx0 [T][D], gp [T][NPest],
                             // cost [T]: the evaluation's results; geo = the plan's adj
    double *x, *p;           // [T][D], [T][NP]: in: the start; out: the returned point (full parameter vectors)
    ShootState *st;          // [T]
    double *work;            // [T][point_doubles]
    size_t point_doubles;
    int m, maxls;
    long long maxiter, maxfun;
    double ftol, gtol;
};

struct ShootView { double *xk, *gk, *d, *ys, *al, *S, *Y; };
VA_HD ShootView shoot_view(const ShootArgs &sa, long traj)
{
    const size_t n = (size_t)(sa.adj.D + sa.adj.NPest), m = (size_t)sa.m;
    ShootView v;
    v.xk = sa.work + (size_t)traj * sa.point_doubles; v.gk = v.xk + n; v.d = v.gk + n; v.ys = v.d + n; v.al = v.ys + m;
    v.S = v.al + m; v.Y = v.S + m * n;
    return v;
}
VA_HD double *shoot_done_flags(const PredictAdjArgs &a, const PredictAdjLds &l) { return l.sts + 6 * (size_t)a.nstim; }

// variable i of a point: column i of x0, or estimated parameter i - D
VA_HD double shoot_g(const PredictAdjArgs &a, long traj, int i)
{
    return i < a.D ? a.gx0[(size_t)traj * a.D + i] : a.gp[(size_t)traj * a.NPest + (i - a.D)];
}
VA_HD double *shoot_xp(const ShootArgs &sa, long traj, int i)
{
    const PredictAdjArgs &a = sa.adj;
    return i < a.D ? sa.x + (size_t)traj * a.D + i : sa.p + (size_t)traj * a.NP + a.Pidx[i - a.D];
}
VA_HD bool shoot_finite(double v) { return fabs(v) <= 1.7976931348623157e308; }
VA_HD double shoot_absmax(double gmax, double g) { return (g != g || gmax != gmax) ? g + gmax : fmax(gmax, fabs(g)); }

VA_HD void shoot_finish(ShootState &s, double *done, int r, int status) { s.status = status; s.phase = SH_DONE; done[r] = 1.0; }
VA_HD void shoot_restore(const ShootArgs &sa, const ShootView &v, long traj, int n)
{
    for (int i = 0; i < n; ++i) *shoot_xp(sa, traj, i) = v.xk[i];
}

// d = -H gk by the two-loop recursion over the pairs head .. head + col - 1 (oldest first), H0 = I / theta
VA_HD void shoot_direction(const ShootState &s, const ShootView &v, int n, int m)
{
    for (int i = 0; i < n; ++i) v.d[i] = v.gk[i];
    for (int j = s.col - 1; j >= 0; --j) {
        const int slot = (s.head + j) % m;
        const double *S = v.S + (size_t)slot * n, *Y = v.Y + (size_t)slot * n;
        double dot = 0.0;
        for (int i = 0; i < n; ++i) dot += S[i] * v.d[i];
        const double al = dot / v.ys[slot];
        v.al[j] = al;
        for (int i = 0; i < n; ++i) v.d[i] -= al * Y[i];
    }
    const double gamma = 1.0 / s.theta;
    for (int i = 0; i < n; ++i) v.d[i] *= gamma;
    for (int j = 0; j < s.col; ++j) {
        const int slot = (s.head + j) % m;
        const double *S = v.S + (size_t)slot * n, *Y = v.Y + (size_t)slot * n;
        double dot = 0.0;
        for (int i = 0; i < n; ++i) dot += Y[i] * v.d[i];
        const double c = v.al[j] - dot / v.ys[slot];
        for (int i = 0; i < n; ++i) v.d[i] += c * S[i];
    }
    for (int i = 0; i < n; ++i) v.d[i] = -v.d[i];
}

// a new search from the iterate (xk, gk, s.f): direction, first step, dcsrch's start, the first trial into (x0, p).  A
// direction that does not descend, or a step dcsrch refuses: once more with emptied memory, status 2 if it was empty
VA_HD void shoot_begin_search(const ShootArgs &sa, ShootState &s, const ShootView &v, long traj, double *done, int r)
{
    const int n = sa.adj.D + sa.adj.NPest;
    for (int pass = 0; pass < 2; ++pass) {
        if (s.col == 0) for (int i = 0; i < n; ++i) v.d[i] = -v.gk[i];
        else shoot_direction(s, v, n, sa.m);
        double gd = 0.0;
        for (int i = 0; i < n; ++i) gd += v.gk[i] * v.d[i];
        double stp = s.iter == 0 ? fmin(1.0 / sqrt(-gd), 1e10) : 1.0;       // lnsrlb; d = -g at iteration 0
        LsState ls = LsState();
        int task = LS_ERROR;
        if (gd < 0.0) task = dcsrch(s.f, gd, stp, 1e-3, 0.9, 0.1, 0.0, 1e10, LS_START, ls);
        if (task != LS_ERROR) {
            s.gdold = gd; s.stp = stp; s.ls = ls; s.nls = 0; s.phase = SH_LS;
            for (int i = 0; i < n; ++i) *shoot_xp(sa, traj, i) = trial(v.xk[i], stp, v.d[i]);
            return;
        }
        if (s.col == 0) break;
        s.col = 0; s.head = 0; s.theta = 1.0;
    }
    shoot_restore(sa, v, traj, n);
    shoot_finish(s, done, r, 2);
}

// before the first evaluation: lane r arms point r, or marks an idle slot as done
VA_HD void shoot_init(const ShootArgs &sa, double *done, long wg, int tid)
{
    const PredictAdjArgs &a = sa.adj;
    if (tid >= a.geo.RW) return;
    const long traj = predict_adj_work(a, wg).group * a.geo.RW + tid;
    if (traj >= a.T) { done[tid] = 1.0; return; }
    ShootState s = ShootState();
    s.phase = SH_START; s.theta = 1.0;
    sa.st[traj] = s;
    done[tid] = 0.0;
}

// the step: lane r consumes the evaluation of point r's trial
VA_HD void shoot_step(const ShootArgs &sa, double *done, long wg, int tid)
{
    const PredictAdjArgs &a = sa.adj;
    if (tid >= a.geo.RW) return;
    const long traj = predict_adj_work(a, wg).group * a.geo.RW + tid;
    if (traj >= a.T) return;
    ShootState &s = sa.st[traj];
    if (s.phase == SH_DONE) return;
    const double epsmch = 2.220446049250313e-16;
    const int n = a.D + a.NPest, m = sa.m;
    const ShootView v = shoot_view(sa, traj);
    const double ft = a.cost[traj];
    if (s.phase == SH_START) {
        s.f = ft; s.f_start = ft; s.nfev = 1;
        double gmax = 0.0;
        for (int i = 0; i < n; ++i) {
            const double g = shoot_g(a, traj, i);
            v.gk[i] = g; v.xk[i] = *shoot_xp(sa, traj, i);
            gmax = shoot_absmax(gmax, g);
        }
        s.gmax = gmax;
        if (!shoot_finite(ft)) { shoot_finish(s, done, tid, 3); return; }
        if (gmax <= sa.gtol) { shoot_finish(s, done, tid, 0); return; }
        shoot_begin_search(sa, s, v, traj, done, tid);
        return;
    }
    s.nfev += 1;
    double gd = 0.0;
    for (int i = 0; i < n; ++i) gd += shoot_g(a, traj, i) * v.d[i];
    const double stp_eval = s.stp;
    bool fail = !shoot_finite(ft) || !shoot_finite(gd);
    if (!fail) {
        LsState ls = s.ls;
        double stp = stp_eval;
        const int task = dcsrch(ft, gd, stp, 1e-3, 0.9, 0.1, 0.0, 1e10, LS_FG, ls);
        if (task == LS_FG) {
            s.nls += 1;
            if (s.nls >= sa.maxls) fail = true;
            else if (s.nfev > sa.maxfun) { shoot_restore(sa, v, traj, n); shoot_finish(s, done, tid, 1); return; }
            else {
                s.ls = ls; s.stp = stp;
                for (int i = 0; i < n; ++i) *shoot_xp(sa, traj, i) = trial(v.xk[i], stp, v.d[i]);
                return;
            }
        }
    }
    if (fail) {
        if (s.col == 0) { shoot_restore(sa, v, traj, n); shoot_finish(s, done, tid, 2); return; }
        s.col = 0; s.head = 0; s.theta = 1.0;                     // (the iterate, its gradient and cost were not touched)
        shoot_begin_search(sa, s, v, traj, done, tid);
        return;
    }
    // the trial is the new iterate
    const double fold = s.f;
    s.f = ft; s.iter += 1;
    const double dr = (gd - s.gdold) * stp_eval, ddum = -s.gdold * stp_eval;
    const bool pair = dr > epsmch * ddum;
    int slot = 0;
    if (pair) {
        if (s.col < m) { slot = (s.head + s.col) % m; s.col += 1; }
        else { slot = s.head; s.head = (s.head + 1) % m; }
    }
    double *S = v.S + (size_t)slot * n, *Y = v.Y + (size_t)slot * n;
    double gmax = 0.0, yy = 0.0;
    for (int i = 0; i < n; ++i) {
        const double g = shoot_g(a, traj, i);
        if (pair) {
            const double y = g - v.gk[i];
            Y[i] = y; S[i] = stp_eval * v.d[i];
            yy += y * y;
        }
        v.gk[i] = g; v.xk[i] = *shoot_xp(sa, traj, i);
        gmax = shoot_absmax(gmax, g);
    }
    if (pair) { v.ys[slot] = dr; s.theta = yy / dr; }
    s.gmax = gmax;
    if (s.iter >= sa.maxiter || s.nfev > sa.maxfun) { shoot_finish(s, done, tid, 1); return; }
    if (gmax <= sa.gtol) { shoot_finish(s, done, tid, 0); return; }
    if (fold - ft <= sa.ftol * fmax(fmax(fabs(fold), fabs(ft)), 1.0)) { shoot_finish(s, done, tid, 0); return; }
    shoot_begin_search(sa, s, v, traj, done, tid);
}

// after a synchronisation behind the step: are all points of the workgroup done?
VA_HD bool shoot_all_done(const PredictAdjArgs &a, const double *done)
{
    bool all = true;
    for (int r = 0; r < a.geo.RW; ++r) all = all && done[r] != 0.0;
    return all;
}

// behind the loop: a point the trip bound stopped returns its iterate with status 1
VA_HD void shoot_final(const ShootArgs &sa, double *done, long wg, int tid)
{
    const PredictAdjArgs &a = sa.adj;
    if (tid >= a.geo.RW) return;
    const long traj = predict_adj_work(a, wg).group * a.geo.RW + tid;
    if (traj >= a.T) return;
    ShootState &s = sa.st[traj];
    if (s.phase == SH_DONE) return;
    if (s.phase == SH_LS) shoot_restore(sa, shoot_view(sa, traj), traj, a.D + a.NPest);
    shoot_finish(s, done, tid, 1);
}
VA_HD int shoot_trips(const ShootArgs &sa) { return (int)sa.maxfun + 2; }

// the nominal trajectory is nobody's output here
template <int E> VA_HD void shoot_no_output(PredictAdjLane<E> &L)
{
#pragma unroll
    for (int e = 0; e < E; ++e)
        if (L.el[e].kind == 1) L.el[e].o = nullptr;
}

// ---------------------------------------------------------------- the same phases, lane by lane on the host
// (every pointer of `sa` is host memory)
template <class RHS, int E>
inline void shoot_eval_host(const PredictAdjArgs &a, const PredictAdjLds &l, long wg, std::vector<PredictAdjLane<E>> &L)
{
    const int nt = a.geo.threads;
    const PredictAdjStep hs = predict_adj_step_sizes(a.dt, a.substeps);
#define VA_SHOOT_ALL(call) for (int tid = 0; tid < nt; ++tid) call
    VA_SHOOT_ALL((predict_adj_load<E>(a, l, wg, tid, L[tid])));
    VA_SHOOT_ALL((shoot_no_output<E>(L[tid])));
    VA_SHOOT_ALL((predict_adj_row<E>(a, 0, L[tid])));
    long long q = 0;
    int until_out = a.every;
    size_t row = 1;
    for (int n = 0; n < a.n_steps; ++n) {
        if (a.nstim) VA_SHOOT_ALL((predict_adj_fstim_step<E>(a, tid, n, L[tid])));
        for (int s = 0; s < a.substeps; ++s, ++q) {
            VA_SHOOT_ALL((predict_adj_fstim_stage<E, 0>(a, l, tid, s, L[tid])));
            VA_SHOOT_ALL((predict_adj_fstage<RHS, E, 0>(a, l, q, hs, L[tid])));
            VA_SHOOT_ALL((predict_adj_fstim_stage<E, 1>(a, l, tid, s, L[tid])));
            VA_SHOOT_ALL((predict_adj_fstage<RHS, E, 1>(a, l, q, hs, L[tid])));
            VA_SHOOT_ALL((predict_adj_fstim_stage<E, 2>(a, l, tid, s, L[tid])));
            VA_SHOOT_ALL((predict_adj_fstage<RHS, E, 2>(a, l, q, hs, L[tid])));
            VA_SHOOT_ALL((predict_adj_fstim_stage<E, 3>(a, l, tid, s, L[tid])));
            VA_SHOOT_ALL((predict_adj_fstage<RHS, E, 3>(a, l, q, hs, L[tid])));
        }
        if (--until_out == 0) {
            until_out = a.every;
            VA_SHOOT_ALL((predict_adj_row<E>(a, row, L[tid])));
            ++row;
        }
    }
    VA_SHOOT_ALL((predict_adj_turn<E>(a, l, tid, L[tid])));
    for (int n = a.n_steps - 1; n >= 0; --n) {
        if (a.nstim) VA_SHOOT_ALL((predict_adj_bstim_step<E>(a, tid, n, L[tid])));
        for (int s = a.substeps - 1; s >= 0; --s) {
            q = (long long)n * a.substeps + s;
            VA_SHOOT_ALL((predict_adj_head<E>(a, l, tid, n, s, q, hs, L[tid])));
            VA_SHOOT_ALL((predict_adj_refwd<RHS, E, 0>(a, l, n, s, q, hs, L[tid])));
            VA_SHOOT_ALL((predict_adj_refwd<RHS, E, 1>(a, l, n, s, q, hs, L[tid])));
            VA_SHOOT_ALL((predict_adj_refwd<RHS, E, 2>(a, l, n, s, q, hs, L[tid])));
            VA_SHOOT_ALL((predict_adj_bstage<RHS, E, 3>(a, l, n, s, q, hs, L[tid])));
            VA_SHOOT_ALL((predict_adj_bstage<RHS, E, 2>(a, l, n, s, q, hs, L[tid])));
            VA_SHOOT_ALL((predict_adj_bstage<RHS, E, 1>(a, l, n, s, q, hs, L[tid])));
            VA_SHOOT_ALL((predict_adj_bstage<RHS, E, 0>(a, l, n, s, q, hs, L[tid])));
        }
    }
    VA_SHOOT_ALL((predict_adj_finish_store<E>(a, l, L[tid])));
    VA_SHOOT_ALL((predict_adj_finish_sum(a, l, wg, tid)));
#undef VA_SHOOT_ALL
}

template <class RHS, int E>
inline void shoot_host_e(const ShootArgs &sa)
{
    const PredictAdjArgs &a = sa.adj;
    const int nt = a.geo.threads;
    std::vector<double> mem(predict_adj_lds_doubles(a.geo.RW, a.geo.chunk, a.D, a.NP, a.nstim) + a.geo.RW + 1, 0.0);
    std::vector<PredictAdjLane<E>> L(nt);
    const PredictAdjLds l = predict_adj_lds(a, mem.data());
    double *done = shoot_done_flags(a, l);
    for (long wg = 0; wg < a.geo.grid; ++wg) {
        for (int tid = 0; tid < nt; ++tid) shoot_init(sa, done, wg, tid);
        for (int trip = 0; trip < shoot_trips(sa); ++trip) {
            shoot_eval_host<RHS, E>(a, l, wg, L);
            for (int tid = 0; tid < nt; ++tid) shoot_step(sa, done, wg, tid);
            if (shoot_all_done(a, done)) break;
        }
        for (int tid = 0; tid < nt; ++tid) shoot_final(sa, done, wg, tid);
    }
}

template <class RHS>
inline void shoot_host(const ShootArgs &sa)
{
    switch (sa.adj.geo.E) {
    case 1: shoot_host_e<RHS, 1>(sa); break;
    case 2: shoot_host_e<RHS, 2>(sa); break;
    case 3: shoot_host_e<RHS, 3>(sa); break;
    default: shoot_host_e<RHS, 4>(sa); break;
    }
}

}  // namespace va

// ---------------------------------------------------------------- the kernel
#if defined(__HIPCC__)

namespace va {

// one evaluation: k_predict_adj's sequence of phases and synchronisations
template <class RHS, int E, bool WAVE>
__device__ __forceinline__ void shoot_eval(const PredictAdjArgs &a, const PredictAdjLds &l, long wg, int tid, const PredictAdjStep &hs)
{
    PredictAdjLane<E> L;
    predict_adj_load<E>(a, l, wg, tid, L);
    shoot_no_output<E>(L);
    predict_adj_row<E>(a, 0, L);
    long long q = 0;
    int until_out = a.every;
    size_t row = 1;
    for (int n = 0; n < a.n_steps; ++n) {
        if (a.nstim) predict_adj_fstim_step<E>(a, tid, n, L);
        for (int s = 0; s < a.substeps; ++s, ++q) {
            predict_adj_fstim_stage<E, 0>(a, l, tid, s, L); predict_sync<WAVE>(); predict_adj_fstage<RHS, E, 0>(a, l, q, hs, L);
            predict_adj_fstim_stage<E, 1>(a, l, tid, s, L); predict_sync<WAVE>(); predict_adj_fstage<RHS, E, 1>(a, l, q, hs, L);
            predict_adj_fstim_stage<E, 2>(a, l, tid, s, L); predict_sync<WAVE>(); predict_adj_fstage<RHS, E, 2>(a, l, q, hs, L);
            predict_adj_fstim_stage<E, 3>(a, l, tid, s, L); predict_sync<WAVE>(); predict_adj_fstage<RHS, E, 3>(a, l, q, hs, L);
        }
        if (--until_out == 0) {
            until_out = a.every;
            predict_adj_row<E>(a, row, L);
            ++row;
        }
    }
    predict_sync<WAVE>();
    predict_adj_turn<E>(a, l, tid, L);
    for (int n = a.n_steps - 1; n >= 0; --n) {
        if (a.nstim) predict_adj_bstim_step<E>(a, tid, n, L);
        for (int s = a.substeps - 1; s >= 0; --s) {
            q = (long long)n * a.substeps + s;
            predict_adj_head<E>(a, l, tid, n, s, q, hs, L);
            predict_sync<WAVE>(); predict_adj_refwd<RHS, E, 0>(a, l, n, s, q, hs, L);
            predict_sync<WAVE>(); predict_adj_refwd<RHS, E, 1>(a, l, n, s, q, hs, L);
            predict_sync<WAVE>(); predict_adj_refwd<RHS, E, 2>(a, l, n, s, q, hs, L);
            predict_sync<WAVE>(); predict_adj_bstage<RHS, E, 3>(a, l, n, s, q, hs, L);
            predict_sync<WAVE>(); predict_adj_bstage<RHS, E, 2>(a, l, n, s, q, hs, L);
            predict_sync<WAVE>(); predict_adj_bstage<RHS, E, 1>(a, l, n, s, q, hs, L);
            predict_sync<WAVE>(); predict_adj_bstage<RHS, E, 0>(a, l, n, s, q, hs, L);
        }
    }
    predict_adj_finish_store<E>(a, l, L);
    predict_sync<WAVE>();
    predict_adj_finish_sum(a, l, wg, tid);
}

// The trial points and the evaluation's results cross lanes through GLOBAL memory (the step's lane writes x0 and p, the
// load phase's lanes read them; finish writes gx0, gp and cost, the step's lane reads them), so the synchronisations around
// the step are workgroup barriers with their fences in the wave form too: wave_sync_lds orders LDS only.
template <class RHS, int E, bool WAVE>
__global__ __launch_bounds__(WAVE ? 64 : 256) void k_shoot(const ShootArgs sa)
{
    extern __shared__ __attribute__((aligned(16))) double shoot_mem[];
    const PredictAdjArgs &a = sa.adj;
    const PredictAdjLds l = predict_adj_lds(a, shoot_mem);
    double *done = shoot_done_flags(a, l);
    const int tid = (int)threadIdx.x;
    const long wg = (long)blockIdx.x;
    const PredictAdjStep hs = predict_adj_step_sizes(a.dt, a.substeps);
    shoot_init(sa, done, wg, tid);
    __syncthreads();
    const int trips = shoot_trips(sa);
    for (int trip = 0; trip < trips; ++trip) {
        shoot_eval<RHS, E, WAVE>(a, l, wg, tid, hs);
        __syncthreads();
        shoot_step(sa, done, wg, tid);
        __syncthreads();
        if (shoot_all_done(a, done)) break;      // (the same LDS words for every lane: uniform)
    }
    shoot_final(sa, done, wg, tid);
}

// E of the workgroup form at a width known when the module is compiled (plan_predict_adj with one cotangent set)
constexpr int shoot_e_of(int D)
{
    const int elems = 2 * D, up = ((elems + 63) / 64) * 64, threads = up < 256 ? up : 256;
    return (elems + threads - 1) / threads;
}

template <class RHS, int E, int DC>
inline hipError_t launch_shoot_e(const ShootArgs &sa, size_t lds_bytes, hipStream_t s)
{
    constexpr bool can = DC == 0 || (DC > 32 && DC <= SHOOT_MAX_D && shoot_e_of(DC) == E);
    if constexpr (can) {
        hipLaunchKernelGGL((k_shoot<RHS, E, false>), dim3((unsigned)sa.adj.geo.grid), dim3((unsigned)sa.adj.geo.threads), lds_bytes, s, sa);
        return hipGetLastError();
    }
    return hipErrorInvalidValue;      // (a geometry plan_shoot does not make for this D)
}

// launch the instantiation sa.adj.geo names.  DC > 0: the model's D is a constant (a generated module): only the
// instantiation that D runs is compiled, none past SHOOT_MAX_D
template <class RHS, int DC>
inline hipError_t launch_shoot(const ShootArgs &sa, hipStream_t s)
{
    const PredictAdjArgs &a = sa.adj;
    const PredictAdjGeo &g = a.geo;
    if (DC > 0 && a.D != DC) return hipErrorInvalidValue;
    if (a.D < 1 || a.D > SHOOT_MAX_D || a.ncot != 1 || a.G || !a.Y || g.nchunks != 1 || g.chunk != 1) return hipErrorInvalidValue;
    if (g.wave != (2 * a.D <= 64 ? 1 : 0) || g.E < 1 || g.E > PREDICT_MAX_E || g.RW < 1 || g.RW > g.threads) return hipErrorInvalidValue;
    if (sa.m < 1 || sa.m > MAX_M || sa.maxfun < 1 || sa.maxfun > SHOOT_MAX_FUN) return hipErrorInvalidValue;
    const size_t lds_bytes = g.lds_bytes + sizeof(double) * (size_t)g.RW;
    if (lds_bytes > PREDICT_ADJ_LDS_LIMIT || !a.ckpt || !sa.x || !sa.st || !sa.work) return hipErrorInvalidValue;
    if (g.wave) {
        if constexpr (DC == 0 || 2 * DC <= 64) {
            if (g.E != 1 || g.threads != 64) return hipErrorInvalidValue;
            hipLaunchKernelGGL((k_shoot<RHS, 1, true>), dim3((unsigned)g.grid), dim3(64), lds_bytes, s, sa);
            return hipGetLastError();
        }
        return hipErrorInvalidValue;
    }
    switch (g.E) {
    case 1: return launch_shoot_e<RHS, 1, DC>(sa, lds_bytes, s);
    case 2: return launch_shoot_e<RHS, 2, DC>(sa, lds_bytes, s);
    case 3: return launch_shoot_e<RHS, 3, DC>(sa, lds_bytes, s);
    default: return launch_shoot_e<RHS, 4, DC>(sa, lds_bytes, s);
    }
}

}  // namespace va
#endif
