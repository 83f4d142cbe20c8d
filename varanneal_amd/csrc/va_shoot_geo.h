// va_shoot_geo.h -- launch geometry, per-point workspace and argument checks of the strong-constraint shooting kernel k_shoot
// (va_shoot.h), as plain host C++: shared by the launcher (va_shoot, va_capi.hip), by the host emulation of the kernel
// (shoot_host) and by the CPU check (tests/cpu_emul/shoot_check.cpp, tests/test_shoot_cpu.py).
//
// The workgroups are the adjoint predictor's in misfit mode (plan_predict_adj with ncot = 1, va_predict_adj_geo.h): a point
// -- one (x0, p_est) to fit -- takes 2 D elements, the nominal trajectory and its one cotangent set.
//   D <= 16      one wave, RW = 64 / (2 D) points side by side
//   D <= 32      one wave, one point
//   D <= 512     one point, 128 .. 256 threads with barriers, E = 1 .. 4 elements per lane
//   wider        refused: the host route (Annealer.shoot(device=False)) remains.  E >= 5 is where the adjoint kernel's
//                register pressure shows, and every width a generated module may have is one more kernel to compile.
// In misfit mode no workgroup ever talks to another, so a point's whole minimisation stays inside its workgroup.
//
// LDS: the adjoint predictor's images (predict_adj_lds_doubles) and RW doubles behind them: the points' "done" flags.
// Global workspace per point (doubles), all of it touched by the point's own lane only:
//   xk [n], gk [n], d [n]        the iterate, its gradient, the search direction;  n = D + NPest
//   ys [m], al [m]               s.y of the stored pairs, the two-loop recursion's alphas
//   S [m][n], Y [m][n]           the L-BFGS pairs, a ring of m slots
// i.e. 3 n + 2 m + 2 m n doubles: 4360 bytes at D = 20, one parameter, m = 10; 85 KiB at D = 512.  The history is read and
// written once per ITERATION, an evaluation's checkpoints (Q D doubles) twice per EVALUATION, so the history lives in global
// memory and LDS limits nothing that the adjoint predictor does not limit already.  Beside it per point: ShootState, the
// trial point (x0 [D], p [NP], read by the evaluation's load phase), the evaluation's results (gx0 [D], gp [NPest], cost) and
// the checkpoints of the point's slot in its workgroup.
#pragma once
#include <stddef.h>
#include <stdio.h>

#include "va_core.h"
#include "va_predict_adj_geo.h"

namespace va {

constexpr int SHOOT_MAX_D = 512;             // E <= 4 elements per lane
constexpr int SHOOT_MAX_FUN = 100000;        // evaluations per point: the kernel's trip count is maxfun + 2

enum { SH_START = 0, SH_LS = 1, SH_DONE = 2 };

// one point's minimiser state (global memory; the launcher downloads the array and unpacks the results)
struct ShootState {
    int phase, status;       // SH_*; 0 converged, 1 budget (maxiter / maxfun), 2 abnormal line search, 3 non-finite cost at the start
    int iter, col, head;     // iterations; pairs stored; the oldest pair's slot
    int nls, pad0, pad1;     // trials the line search in progress has consumed
    long long nfev;
    double f, f_start, gmax; // cost and largest gradient entry at the iterate; cost at the start
    double stp, gdold, theta;
    LsState ls;
};

struct ShootGeo {
    PredictAdjGeo adj;       // the evaluation's geometry: plan_predict_adj(D, T, 1, NP, nstim)
    int n = 0, m = 0;        // variables per point, history pairs
    size_t lds_bytes = 0;    // adj.lds_bytes + 8 RW
    size_t point_doubles = 0;     // shoot_point_doubles(n, m)
    const char *why = "";
};

inline size_t shoot_point_doubles(int n, int m) { return 3 * (size_t)n + 2 * (size_t)m + 2 * (size_t)m * n; }

inline bool plan_shoot(int D, long T, int NP, int NPest, int nstim, int m, ShootGeo &g)
{
    g = ShootGeo();
    if (D < 1 || T < 1 || NP < 0 || NPest < 0 || NPest > NP || nstim < 0) { g.why = "bad sizes"; return false; }
    if (m < 1 || m > MAX_M) { g.why = "the history holds 1 to 32 pairs (MAX_M)"; return false; }
    if (D > SHOOT_MAX_D) { g.why = "the shooting kernel carries states of at most 512 columns (256 threads x 4 elements per lane)"; return false; }
    if (!plan_predict_adj(D, T, 1, NP, nstim, g.adj)) { g.why = g.adj.why; return false; }
    g.n = D + NPest; g.m = m;
    g.lds_bytes = g.adj.lds_bytes + sizeof(double) * (size_t)g.adj.RW;
    if (g.lds_bytes > PREDICT_ADJ_LDS_LIMIT) { g.why = "parameters, parameter partials and stage images do not fit 64 KiB of LDS"; return false; }
    g.point_doubles = shoot_point_doubles(g.n, m);
    return true;
}

// the options every entry checks (va_shoot, shoot_check): false with the reason in why[]
inline bool shoot_check_args(int m, long long maxiter, long long maxfun, int maxls, char *why, size_t len)
{
    if (m < 1 || m > MAX_M) { snprintf(why, len, "m must be 1 .. %d (MAX_M), got %d", MAX_M, m); return false; }
    if (maxfun < 1 || maxfun > SHOOT_MAX_FUN) { snprintf(why, len, "maxfun must be 1 .. %d, got %lld", SHOOT_MAX_FUN, maxfun); return false; }
    if (maxiter < 1) { snprintf(why, len, "maxiter must be at least 1, got %lld", maxiter); return false; }
    if (maxls < 1) { snprintf(why, len, "maxls must be at least 1, got %d", maxls); return false; }
    return true;
}

// va_shoot's device buffers per point, in doubles: the trial point x0, p; the observations (when every point has its own);
// gx0, gp, cost; the checkpoints of its slot; ShootState; the minimiser's vectors and history -- and, through
// predict_adj_chunk_trajs, the points of a chunk that stay under PREDICT_ADJ_WORKSPACE_BYTES
inline size_t shoot_state_doubles() { return (sizeof(ShootState) + sizeof(double) - 1) / sizeof(double); }
inline size_t shoot_traj_doubles(int D, int NP, int NPest, long long Q, int m, size_t y_doubles)
{
    return (size_t)D + NP + y_doubles + (size_t)D + NPest + 1 + (size_t)Q * D + shoot_state_doubles() + shoot_point_doubles(D + NPest, m);
}

// ---------------------------------------------------------------- the boxed shoot (k_shoot_box, va_shoot_box.h)
// The same workgroups, LDS and limits; what grows is the minimiser: one lane per point runs L-BFGS-B.  Its state is a struct
// of its own (ShootState stays as it is), and its per-point workspace in global memory holds, in doubles,
//   xk, gk, d, z, r, t, xp [n each]    the iterate, its gradient, the direction, the Cauchy / subspace point, the reduced
//                                      gradient, the breakpoints, the point saved for subsm's backtrack;  n = D + NPest
//   S [m][n], Y [m][n]                 the pairs, a ring of m columns
//   sy, ss, wt [m m each]              S'Y, S'S, the factor of T = theta S'S + L D^-1 L'
//   wn, wn1 [4 m m each]               the factored reduced middle matrix and its inner-product blocks, kept incrementally
//   wa [8 m]                           cauchy's p, c, wbp, v
// and behind them iwhere, index, iorder [n ints each], two ints to a double:
//   shoot_box_point_doubles(n, m) = 7 n + 2 m n + 11 m m + 8 m + (3 n + 1) / 2
// 14.6 KiB at D = 20, one parameter, m = 10; 218 KiB at D = 512, m = 10.
struct ShootBoxState {
    int phase, status;       // as ShootState
    int iter, col, head;     // iterations; pairs stored; the oldest pair's column, 1-based (the published code's ring)
    int itail, iupdat, updatd;     // the newest pair's column; pairs accepted since the memory was emptied; the last iteration stored one
    int nls, nfree, nenter, ileave;     // trials of the search in progress; free variables at the Cauchy point; entered / left (freev)
    int cnstnd, boxed, wnsync, pad0;    // any bound; every entry two-sided; wn1 holds every pair and the last free set
    long long nfev;
    double f, f_start, gmax; // cost at the iterate; cost of the projected start; projected-gradient norm sbgnrm at the iterate
    double stp, stpmx, gdold, theta, dtd;
    LsState ls;
};

inline size_t shoot_box_point_doubles(int n, int m)
{
    return 7 * (size_t)n + 2 * (size_t)m * n + 11 * (size_t)m * m + 8 * (size_t)m + (3 * (size_t)n + 1) / 2;
}

// plan_shoot's geometry with the larger workspace
inline bool plan_shoot_box(int D, long T, int NP, int NPest, int nstim, int m, ShootGeo &g)
{
    if (!plan_shoot(D, T, NP, NPest, nstim, m, g)) return false;
    g.point_doubles = shoot_box_point_doubles(g.n, m);
    return true;
}

// the box: `count` tables of n entries (1 when shared); -inf / +inf: no bound.  false with the first bad entry named
inline bool shoot_box_check_bounds(const double *lower, const double *upper, long count, int n, char *why, size_t len)
{
    for (long t = 0; t < count; ++t)
        for (int i = 0; i < n; ++i) {
            const double lo = lower[(size_t)t * n + i], hi = upper[(size_t)t * n + i];
            if (lo != lo || hi != hi) { snprintf(why, len, "bounds: entry %d of table %ld is NaN", i, t); return false; }
            if (lo > hi) { snprintf(why, len, "bounds: entry %d of table %ld has lower %.17g > upper %.17g", i, t, lo, hi); return false; }
        }
    return true;
}

// va_shoot_box's device buffers per point, as shoot_traj_doubles: the larger state and workspace, and the point's own box
// (box_doubles = 2 n when every point has one, 0 when all share one table)
inline size_t shoot_box_state_doubles() { return (sizeof(ShootBoxState) + sizeof(double) - 1) / sizeof(double); }
inline size_t shoot_box_traj_doubles(int D, int NP, int NPest, long long Q, int m, size_t y_doubles, size_t box_doubles)
{
    return (size_t)D + NP + y_doubles + box_doubles + (size_t)D + NPest + 1 + (size_t)Q * D + shoot_box_state_doubles()
           + shoot_box_point_doubles(D + NPest, m);
}

}  // namespace va
