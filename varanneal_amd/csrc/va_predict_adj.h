// va_predict_adj.h -- the adjoint of the RK4 predictor: the exact transpose of the map k_predict_tlm (va_predict_tlm.h)
// differentiates, i.e. of the derivative of the DISCRETE RK4 map, not a discretisation of the continuous adjoint equation.
//
// For T trajectories with ncot cotangent sets each, a workgroup integrates the nominal trajectory forward with
// va_predict.h's arithmetic (same stage times, stimulus interpolation, substeps and every), writes the state at the start of
// every RK4 step to a checkpoint buffer of its own in global memory, and walks the steps backward.  For a step with the
// cotangent l+ of its result it loads x_n (asked for a step ahead, like the stimulus rows), recomputes X2 = x + h/2 k1,
// X3 = x + h/2 k2, X4 = x + h k3 with the forward arithmetic -- the linearisation points are the forward pass's own bits -- and
//     k4~ = h/6 l+                 X4~ = J(X4)^T k4~    gp += pgrad(X4, k4~)
//     k3~ = h/3 l+ + h   X4~       X3~ = J(X3)^T k3~    gp += pgrad(X3, k3~)
//     k2~ = h/3 l+ + h/2 X3~       X2~ = J(X2)^T k2~    gp += pgrad(X2, k2~)
//     k1~ = h/6 l+ + h/2 X2~       X1~ = J(x)^T  k1~    gp += pgrad(x,  k1~)
//     l   = l+ + (((X4~ + X3~) + X2~) + X1~)
// with J^T s = RHS::vjp and (df/dp)^T s = RHS::pgrad, the terms the action's gradient uses.  At every output row l takes that
// row's cotangent before the step below it; row 0's is added to the result.  The cotangents are the caller's
// (G [T][ncot][n_out][D]), or, in misfit mode (ncot = 1), 2 w_l (x_l - y_l) at the observed columns, formed from the state
// the backward pass holds at the row; cost = sum w_l (x_l - y_l)^2 is then accumulated per column in row order during the
// forward pass and summed in column order at the end.
//
// Like va_predict_tlm.h the arithmetic is written once as __host__ __device__ phases of ONE LANE; k_predict_adj gives them
// their decomposition (va_predict_adj_geo.h), predict_adj_host drives them lane by lane on the CPU
// (tests/cpu_emul/predict_adj_check.cpp).  A lane owns E elements (slot, column): slot 0 of a trajectory is the nominal
// state, slots 1 .. chunk are cotangent sets.  State, l, the sum of the X~ and the value asked for ahead live in registers.
// LDS images, ONE synchronisation per phase:
//   xs [4]   the nominal's stage inputs X1 .. X4 of the step.  Stage k of the step with b = (Q - q) & 1 is image (b + k) & 3:
//            the next step's X1 is written (beside the last cotangent phase, which reads this step's X1) into the image that
//            held X2, whose readers are a synchronisation behind.  The forward pass uses images 0 and 1 as k_predict does.
//   cs [2]   the stage cotangents k~ of all cotangent slots, written and read in turn (va_predict.h says why one
//            synchronisation per phase is enough)
//   gps      the parameter partials per (slot, column), each added to by its own lane only, in time order; one lane per
//            (slot, estimated parameter) sums the columns in column order at the end.  No atomics: the same bits every call.
// A step backward is 7 phases (3 of recomputation, 4 of cotangents) after the 4 of the forward pass.
#pragma once
#include <vector>

#include "va_core.h"
#include "va_predict.h"
#include "va_predict_adj_geo.h"

namespace va {

struct PredictAdjArgs {
    const double *x0;        // [T][D]
    const double *p;         // [T][NP]
    const double *G;         // cotangent mode: [T][ncot][n_out][D]; NULL: misfit mode
    const double *Y;         // misfit mode: [T or 1][n_out][L], the observations of the columns Lidx
    const double *w;         // misfit mode: [L]
    const double *stim;      // NULL or [n_steps + 1][nstim], shared by the trajectories
    const int *Pidx;         // [NPest]: where an estimated parameter sits in the full vector
    const int *Lidx;         // misfit mode: [L], the observed columns
    double *out;             // [T][n_out][D]: the nominal trajectory
    double *gx0;             // [T][ncot][D]
    double *gp;              // [T][ncot][NPest]
    double *cost;            // misfit mode: [T]
    double *ckpt;            // [grid][RW][n_steps substeps][D]: the workgroups' checkpoints
    size_t y_stride;         // n_out L, or 0 when the trajectories share one Y
    int T, D, NP, NPest, ncot, L, nstim, n_steps, substeps, every, n_out;
    double t0, dt;
    PredictAdjGeo geo;
};

struct PredictAdjStep { double h, hh, h6, h3; };      // h, h / 2, h / 6, h / 3
VA_HD PredictAdjStep predict_adj_step_sizes(double dt, int substeps)
{
    const PredictStep s = predict_step_sizes(dt, substeps);
    PredictAdjStep r = {s.h, s.hh, s.h6, s.h / 3.0};
    return r;
}

// one element of a lane: kind 0 nobody's, 1 nominal, 2 cotangent
struct PredictAdjElem {
    int kind, col;
    int noff, coff, poff;    // the trajectory's place in a nominal image, the slot's in a cotangent image, the trajectory's parameters
    double *o;               // nominal: row 0 of the column in out (NULL: another chunk stores it); cotangent: the entry of gx0
    double *ck;              // nominal: the column's checkpoint of step 0
    const double *g;         // cotangent mode: row 0 of the column in G; misfit mode: row 0 of the column's observations (NULL: not observed)
    double w;                // misfit mode: the column's weight
};

template <int E> struct PredictAdjLane {
    double x[E], acc[E];     // state and k-accumulator / cotangent l and the sum of the X~
    double aux[E];           // asked for ahead: the nominal's checkpoint of the step below / the cotangent the row adds
    double cost[E];          // misfit mode, nominal: the column's share of the cost
    double g0, g1, gn;       // the lane's stimulus column at two neighbouring rows and the row asked for ahead
    PredictAdjElem el[E];
};

struct PredictAdjLds { double *xs, *cs, *ps, *gps, *sts; int imgn, imgc; };
VA_HD PredictAdjLds predict_adj_lds(const PredictAdjArgs &a, double *base)
{
    PredictAdjLds l;
    l.imgn = a.geo.RW * a.D; l.imgc = a.geo.RW * a.geo.chunk * a.D;
    l.xs = base; l.cs = l.xs + 4 * (size_t)l.imgn; l.ps = l.cs + 2 * (size_t)l.imgc; l.gps = l.ps + (size_t)a.geo.RW * a.NP;
    l.sts = l.gps + (size_t)l.imgc * a.geo.pitch;
    return l;
}

struct PredictAdjWork { long group; int ck; };
VA_HD PredictAdjWork predict_adj_work(const PredictAdjArgs &a, long wg)
{
    PredictAdjWork w;
    w.group = wg / a.geo.nchunks; w.ck = (int)(wg - w.group * a.geo.nchunks);
    return w;
}
VA_HD long long predict_adj_q(const PredictAdjArgs &a) { return (long long)a.n_steps * a.substeps; }

// phase 0: the lane's elements; x0 into the registers and the first stage input; the workgroup's parameters; zero partials;
// the lane's stimulus column at rows 0 and 1
template <int E>
VA_HD void predict_adj_load(const PredictAdjArgs &a, const PredictAdjLds &l, long wg, int tid, PredictAdjLane<E> &L)
{
    const PredictAdjGeo &g = a.geo;
    const PredictAdjWork w = predict_adj_work(a, wg);
    const int D = a.D;
    const size_t rowD = (size_t)a.n_out * D;
    const size_t Q = (size_t)predict_adj_q(a);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        PredictAdjElem &el = L.el[e];
        int r, s;
        predict_adj_elem(g, D, tid + e * g.threads, &r, &s, &el.col);
        const long traj = w.group * g.RW + r;
        const int dir = w.ck * g.chunk + s - 1;
        el.kind = (r < g.RW && traj < a.T) ? (s == 0 ? 1 : (dir < a.ncot ? 2 : 0)) : 0;
        el.noff = r * D; el.coff = (r * g.chunk + (s > 0 ? s - 1 : 0)) * D; el.poff = r * a.NP;
        el.o = nullptr; el.ck = nullptr; el.g = nullptr; el.w = 0.0;
        L.x[e] = 0.0; L.acc[e] = 0.0; L.aux[e] = 0.0; L.cost[e] = 0.0;
        if (el.kind && !a.G) {
            for (int k = 0; k < a.L; ++k)
                if (a.Lidx[k] == el.col) { el.g = a.Y + (size_t)traj * a.y_stride + k; el.w = a.w[k]; }
        }
        if (el.kind == 1) {
            L.x[e] = a.x0[(size_t)traj * D + el.col];
            el.ck = a.ckpt + ((size_t)wg * g.RW + r) * Q * D + el.col;
            if (w.ck == 0) el.o = a.out + (size_t)traj * rowD + el.col;       // (the other chunks recompute it and keep it to themselves)
            l.xs[el.noff + el.col] = L.x[e];
        } else if (el.kind == 2) {
            el.o = a.gx0 + ((size_t)traj * a.ncot + dir) * D + el.col;
            if (a.G) el.g = a.G + ((size_t)traj * a.ncot + dir) * rowD + el.col;
            double *acc = l.gps + (size_t)(el.coff + el.col) * g.pitch;
            for (int k = 0; k < g.pitch; ++k) acc[k] = 0.0;
        }
    }
    const long np = (long)g.RW * a.NP, first = w.group * np, all = (long)a.T * a.NP;
    for (long e = tid; e < np; e += g.threads) l.ps[e] = first + e < all ? a.p[first + e] : 0.0;
    L.g0 = 0.0; L.g1 = 0.0; L.gn = 0.0;
    if (tid < a.nstim) { L.g1 = a.stim[tid]; L.gn = a.stim[a.nstim + tid]; }
}

// forward, start of model step n: the stimulus column moves on one row (va_predict.h)
template <int E>
VA_HD void predict_adj_fstim_step(const PredictAdjArgs &a, int tid, int n, PredictAdjLane<E> &L)
{
    L.g0 = L.g1; L.g1 = L.gn;
    if (tid < a.nstim && n + 2 <= a.n_steps) L.gn = a.stim[(size_t)(n + 2) * a.nstim + tid];
}

template <int E, int STAGE>
VA_HD void predict_adj_fstim_stage(const PredictAdjArgs &a, const PredictAdjLds &l, int tid, int s, const PredictAdjLane<E> &L)
{
    constexpr int in = STAGE & 1;
    if (tid < a.nstim)
        l.sts[in * a.nstim + tid] = predict_interp(L.g0, L.g1, ((double)s + predict_c<STAGE>()) / (double)a.substeps);
}

// forward stage of the nominal elements: va_predict.h's predict_stage; stage 0 also leaves the step's checkpoint
template <class RHS, int E, int STAGE>
VA_HD void predict_adj_fstage(const PredictAdjArgs &a, const PredictAdjLds &l, long long q, const PredictAdjStep &hs, PredictAdjLane<E> &L)
{
    constexpr int in = STAGE & 1;
    const int D = a.D;
    const double *xin = l.xs + (size_t)in * l.imgn;
    double *xout = l.xs + (size_t)(in ^ 1) * l.imgn;
    const double *st = l.sts + in * a.nstim;
    const double t = predict_time(a.t0, q, predict_c<STAGE>(), hs.h);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const PredictAdjElem &el = L.el[e];
        if (el.kind == 1) {
            if (STAGE == 0) el.ck[(size_t)q * D] = L.x[e];
            const double k = predict_f<RHS>(xin + el.noff, el.col, D, l.ps + el.poff, t, st);
            double *xo = xout + el.noff + el.col;
            if (STAGE == 0) { L.acc[e] = k; *xo = L.x[e] + hs.hh * k; }
            else if (STAGE == 1) { L.acc[e] += 2.0 * k; *xo = L.x[e] + hs.hh * k; }
            else if (STAGE == 2) { L.acc[e] += 2.0 * k; *xo = L.x[e] + hs.h * k; }
            else { L.acc[e] += k; L.x[e] += hs.h6 * L.acc[e]; *xo = L.x[e]; }
        }
    }
}

// forward, output row `row` of the nominal: the state, and in misfit mode the column's share of the cost
template <int E>
VA_HD void predict_adj_row(const PredictAdjArgs &a, size_t row, PredictAdjLane<E> &L)
{
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const PredictAdjElem &el = L.el[e];
        if (el.kind == 1) {
            if (el.o) el.o[row * a.D] = L.x[e];
            if (el.g) {
                const double d = L.x[e] - el.g[row * a.L];
                L.cost[e] += el.w * (d * d);
            }
        }
    }
}

// the turn, after a synchronisation: the final state stands in image 0.  l starts as the last row's cotangent where the
// last step ends on a row, as zero otherwise; the nominal asks for the last checkpoint, the stimulus lane for row n_steps - 2
template <int E>
VA_HD void predict_adj_turn(const PredictAdjArgs &a, const PredictAdjLds &l, int tid, PredictAdjLane<E> &L)
{
    const size_t Q = (size_t)predict_adj_q(a);
    const bool last = a.n_steps % a.every == 0;
    const size_t row = (size_t)a.n_out - 1;
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const PredictAdjElem &el = L.el[e];
        if (el.kind == 1) L.aux[e] = el.ck[(Q - 1) * a.D];
        else if (el.kind == 2) {
            L.x[e] = 0.0; L.acc[e] = 0.0; L.aux[e] = 0.0;
            if (last && el.g) L.x[e] = a.G ? el.g[row * a.D] : 2.0 * el.w * (l.xs[el.noff + el.col] - el.g[row * a.L]);
        }
    }
    if (tid < a.nstim && a.n_steps >= 2) L.gn = a.stim[(size_t)(a.n_steps - 2) * a.nstim + tid];
}

// backward, start of model step n (descending): the stimulus column moves down one row; row n - 1 is asked for ahead
template <int E>
VA_HD void predict_adj_bstim_step(const PredictAdjArgs &a, int tid, int n, PredictAdjLane<E> &L)
{
    if (tid >= a.nstim) return;
    if (n < a.n_steps - 1) { L.g1 = L.g0; L.g0 = L.gn; }
    if (n >= 1 && n < a.n_steps - 1) L.gn = a.stim[(size_t)(n - 1) * a.nstim + tid];
}

VA_HD bool predict_adj_rowstep(const PredictAdjArgs &a, int n, int s) { return s == 0 && n % a.every == 0; }

// head of the backward step q = n substeps + s: the nominal takes its checkpoint, asks for the one below and writes X1; a
// cotangent element writes k4~ and, on a row in cotangent mode, asks for the row's cotangent; the stimulus at the three stage times
template <int E>
VA_HD void predict_adj_head(const PredictAdjArgs &a, const PredictAdjLds &l, int tid, int n, int s, long long q, const PredictAdjStep &hs,
                            PredictAdjLane<E> &L)
{
    const int b = (int)((predict_adj_q(a) - q) & 1);
    const bool rowstep = predict_adj_rowstep(a, n, s);
    const size_t row = (size_t)(n / a.every);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const PredictAdjElem &el = L.el[e];
        if (el.kind == 1) {
            L.x[e] = L.aux[e];
            if (q > 0) L.aux[e] = el.ck[(size_t)(q - 1) * a.D];
            l.xs[(size_t)b * l.imgn + el.noff + el.col] = L.x[e];
        } else if (el.kind == 2) {
            l.cs[el.coff + el.col] = hs.h6 * L.x[e];
            if (rowstep && a.G) L.aux[e] = el.g[row * a.D];
        }
    }
    if (tid < a.nstim) {
        double *st = l.sts + (size_t)b * 3 * a.nstim + tid;
        st[0] = predict_interp(L.g0, L.g1, ((double)s + 0.0) / (double)a.substeps);
        st[a.nstim] = predict_interp(L.g0, L.g1, ((double)s + 0.5) / (double)a.substeps);
        st[2 * a.nstim] = predict_interp(L.g0, L.g1, ((double)s + 1.0) / (double)a.substeps);
    }
}

template <int STAGE> VA_HD int predict_adj_st() { return STAGE == 0 ? 0 : (STAGE == 3 ? 2 : 1); }      // which of the three stimulus rows

// recomputation K = 0, 1, 2: the nominal's X_{K+2} from X_{K+1} with the forward arithmetic.  Beside K = 0, in misfit mode on
// a row: the cotangent element forms the row's cotangent from X1 = x_n
template <class RHS, int E, int K>
VA_HD void predict_adj_refwd(const PredictAdjArgs &a, const PredictAdjLds &l, int n, int s, long long q, const PredictAdjStep &hs,
                             PredictAdjLane<E> &L)
{
    const int b = (int)((predict_adj_q(a) - q) & 1), D = a.D;
    const double *xin = l.xs + (size_t)((b + K) & 3) * l.imgn;
    double *xout = l.xs + (size_t)((b + K + 1) & 3) * l.imgn;
    const double *st = l.sts + (size_t)(b * 3 + predict_adj_st<K>()) * a.nstim;
    const double t = predict_time(a.t0, q, predict_c<K>(), hs.h);
    const bool form = K == 0 && !a.G && predict_adj_rowstep(a, n, s);
    const size_t row = (size_t)(n / a.every);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const PredictAdjElem &el = L.el[e];
        if (el.kind == 1) {
            const double k = predict_f<RHS>(xin + el.noff, el.col, D, l.ps + el.poff, t, st);
            xout[el.noff + el.col] = L.x[e] + (K == 2 ? hs.h : hs.hh) * k;
        } else if (el.kind == 2 && form) {
            L.aux[e] = el.g ? 2.0 * el.w * (xin[el.noff + el.col] - el.g[row * a.L]) : 0.0;
        }
    }
}

// cotangent phase of stage STAGE = 3, 2, 1, 0: X~ = J(X_stage)^T k~ and the parameter partials; the next stage's k~ into the
// other image, or, after stage 0, the cotangent of the step's start, which takes the row's cotangent where x_n is a row
template <class RHS, int E, int STAGE>
VA_HD void predict_adj_bstage(const PredictAdjArgs &a, const PredictAdjLds &l, int n, int s, long long q, const PredictAdjStep &hs,
                              PredictAdjLane<E> &L)
{
    constexpr int in = (3 - STAGE) & 1;
    const int b = (int)((predict_adj_q(a) - q) & 1), D = a.D;
    const double *X = l.xs + (size_t)((b + STAGE) & 3) * l.imgn;
    const double *cin = l.cs + (size_t)in * l.imgc;
    double *cout = l.cs + (size_t)(in ^ 1) * l.imgc;
    const double *st = l.sts + (size_t)(b * 3 + predict_adj_st<STAGE>()) * a.nstim;
    const double t = predict_time(a.t0, q, predict_c<STAGE>(), hs.h);
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const PredictAdjElem &el = L.el[e];
        if (el.kind == 2) {
            const double *x = X + el.noff, *k = cin + el.coff, *p = l.ps + el.poff;
            const double v = RHS::vjp(x, k, el.col, D, p, t, st);
            RHS::pgrad(x, k, el.col, D, p, t, st, l.gps + (size_t)(el.coff + el.col) * a.geo.pitch);
            double *co = cout + el.coff + el.col;
            if (STAGE == 3) { L.acc[e] = v; *co = hs.h3 * L.x[e] + hs.h * v; }
            else if (STAGE == 2) { L.acc[e] += v; *co = hs.h3 * L.x[e] + hs.hh * v; }
            else if (STAGE == 1) { L.acc[e] += v; *co = hs.h6 * L.x[e] + hs.hh * v; }
            else {
                L.acc[e] += v; L.x[e] += L.acc[e];
                if (predict_adj_rowstep(a, n, s)) L.x[e] += L.aux[e];
            }
        }
    }
}

// the end: gx0; the nominal's cost shares into cotangent image 0 (whose last readers are two synchronisations behind)
template <int E>
VA_HD void predict_adj_finish_store(const PredictAdjArgs &a, const PredictAdjLds &l, const PredictAdjLane<E> &L)
{
#pragma unroll
    for (int e = 0; e < E; ++e) {
        const PredictAdjElem &el = L.el[e];
        if (el.kind == 2) el.o[0] = L.x[e];
        else if (el.kind == 1 && !a.G) l.cs[el.noff + el.col] = L.cost[e];
    }
}

// after a synchronisation: one lane per (slot, estimated parameter) sums the columns' partials in column order, one lane
// per trajectory the columns' cost shares
VA_HD void predict_adj_finish_sum(const PredictAdjArgs &a, const PredictAdjLds &l, long wg, int tid)
{
    const PredictAdjGeo &g = a.geo;
    const PredictAdjWork w = predict_adj_work(a, wg);
    for (int idx = tid; idx < g.RW * g.chunk * a.NPest; idx += g.threads) {
        const int rd = idx / a.NPest, k = idx - rd * a.NPest, r = rd / g.chunk, s1 = rd - r * g.chunk;
        const long traj = w.group * g.RW + r;
        const int dir = w.ck * g.chunk + s1;
        if (traj < a.T && dir < a.ncot) {
            const double *acc = l.gps + (size_t)rd * a.D * g.pitch + a.Pidx[k];
            double tot = 0.0;
            for (int i = 0; i < a.D; ++i) tot += acc[(size_t)i * g.pitch];
            a.gp[((size_t)traj * a.ncot + dir) * a.NPest + k] = tot;
        }
    }
    if (!a.G && w.ck == 0)
        for (int r = tid; r < g.RW; r += g.threads) {
            const long traj = w.group * g.RW + r;
            if (traj < a.T) {
                double tot = 0.0;
                for (int i = 0; i < a.D; ++i) tot += l.cs[r * a.D + i];
                a.cost[traj] = tot;
            }
        }
}

// ---------------------------------------------------------------- the same phases, lane by lane on the host
// (every pointer of `a` is host memory; a.geo from plan_predict_adj)
template <class RHS, int E>
inline void predict_adj_host_e(const PredictAdjArgs &a)
{
    const int nt = a.geo.threads;
    const PredictAdjStep hs = predict_adj_step_sizes(a.dt, a.substeps);
    std::vector<double> mem(predict_adj_lds_doubles(a.geo.RW, a.geo.chunk, a.D, a.NP, a.nstim) + 1, 0.0);
    std::vector<PredictAdjLane<E>> L(nt);
    const PredictAdjLds l = predict_adj_lds(a, mem.data());
#define VA_ADJ_ALL(call) for (int tid = 0; tid < nt; ++tid) call
    for (long wg = 0; wg < a.geo.grid; ++wg) {
        VA_ADJ_ALL((predict_adj_load<E>(a, l, wg, tid, L[tid])));
        VA_ADJ_ALL((predict_adj_row<E>(a, 0, L[tid])));
        long long q = 0;
        int until_out = a.every;
        size_t row = 1;
        for (int n = 0; n < a.n_steps; ++n) {
            if (a.nstim) VA_ADJ_ALL((predict_adj_fstim_step<E>(a, tid, n, L[tid])));
            for (int s = 0; s < a.substeps; ++s, ++q) {
                VA_ADJ_ALL((predict_adj_fstim_stage<E, 0>(a, l, tid, s, L[tid])));
                VA_ADJ_ALL((predict_adj_fstage<RHS, E, 0>(a, l, q, hs, L[tid])));
                VA_ADJ_ALL((predict_adj_fstim_stage<E, 1>(a, l, tid, s, L[tid])));
                VA_ADJ_ALL((predict_adj_fstage<RHS, E, 1>(a, l, q, hs, L[tid])));
                VA_ADJ_ALL((predict_adj_fstim_stage<E, 2>(a, l, tid, s, L[tid])));
                VA_ADJ_ALL((predict_adj_fstage<RHS, E, 2>(a, l, q, hs, L[tid])));
                VA_ADJ_ALL((predict_adj_fstim_stage<E, 3>(a, l, tid, s, L[tid])));
                VA_ADJ_ALL((predict_adj_fstage<RHS, E, 3>(a, l, q, hs, L[tid])));
            }
            if (--until_out == 0) {
                until_out = a.every;
                VA_ADJ_ALL((predict_adj_row<E>(a, row, L[tid])));
                ++row;
            }
        }
        VA_ADJ_ALL((predict_adj_turn<E>(a, l, tid, L[tid])));
        for (int n = a.n_steps - 1; n >= 0; --n) {
            if (a.nstim) VA_ADJ_ALL((predict_adj_bstim_step<E>(a, tid, n, L[tid])));
            for (int s = a.substeps - 1; s >= 0; --s) {
                q = (long long)n * a.substeps + s;
                VA_ADJ_ALL((predict_adj_head<E>(a, l, tid, n, s, q, hs, L[tid])));
                VA_ADJ_ALL((predict_adj_refwd<RHS, E, 0>(a, l, n, s, q, hs, L[tid])));
                VA_ADJ_ALL((predict_adj_refwd<RHS, E, 1>(a, l, n, s, q, hs, L[tid])));
                VA_ADJ_ALL((predict_adj_refwd<RHS, E, 2>(a, l, n, s, q, hs, L[tid])));
                VA_ADJ_ALL((predict_adj_bstage<RHS, E, 3>(a, l, n, s, q, hs, L[tid])));
                VA_ADJ_ALL((predict_adj_bstage<RHS, E, 2>(a, l, n, s, q, hs, L[tid])));
                VA_ADJ_ALL((predict_adj_bstage<RHS, E, 1>(a, l, n, s, q, hs, L[tid])));
                VA_ADJ_ALL((predict_adj_bstage<RHS, E, 0>(a, l, n, s, q, hs, L[tid])));
            }
        }
        VA_ADJ_ALL((predict_adj_finish_store<E>(a, l, L[tid])));
        VA_ADJ_ALL((predict_adj_finish_sum(a, l, wg, tid)));
    }
#undef VA_ADJ_ALL
}

template <class RHS>
inline void predict_adj_host(const PredictAdjArgs &a)
{
    switch (a.geo.E) {
    case 1: predict_adj_host_e<RHS, 1>(a); break;
    case 2: predict_adj_host_e<RHS, 2>(a); break;
    case 3: predict_adj_host_e<RHS, 3>(a); break;
    case 4: predict_adj_host_e<RHS, 4>(a); break;
    case 5: predict_adj_host_e<RHS, 5>(a); break;
    case 6: predict_adj_host_e<RHS, 6>(a); break;
    case 7: predict_adj_host_e<RHS, 7>(a); break;
    default: predict_adj_host_e<RHS, 8>(a); break;
    }
}

}  // namespace va

// ---------------------------------------------------------------- the kernel
#if defined(__HIPCC__)
#include "va_eval_flat.h"      // wave_sync_lds

namespace va {

template <class RHS, int E, bool WAVE>
__global__ __launch_bounds__(WAVE ? 64 : 256) void k_predict_adj(const PredictAdjArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double predict_adj_mem[];
    const PredictAdjLds l = predict_adj_lds(a, predict_adj_mem);
    const int tid = (int)threadIdx.x;
    const long wg = (long)blockIdx.x;
    const PredictAdjStep hs = predict_adj_step_sizes(a.dt, a.substeps);
    PredictAdjLane<E> L;
    predict_adj_load<E>(a, l, wg, tid, L);
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

// launch the instantiation a.geo names.  DC > 0: the model's D is a constant (a generated module): only the instantiations
// that D can run are compiled (E depends on the number of cotangent sets of the call as well)
template <class RHS, int E, int DC>
inline hipError_t launch_predict_adj_e(const PredictAdjArgs &a, hipStream_t s)
{
    constexpr bool can = DC == 0 || (DC > 32 && 2 * DC <= 256 * E && (DC <= 512 ? E <= PREDICT_MAX_E : 2 * DC > 256 * (E - 1)));
    if constexpr (can) {
        hipLaunchKernelGGL((k_predict_adj<RHS, E, false>), dim3((unsigned)a.geo.grid), dim3((unsigned)a.geo.threads), a.geo.lds_bytes, s, a);
        return hipGetLastError();
    }
    return hipErrorInvalidValue;      // (a geometry plan_predict_adj does not make for this D)
}

template <class RHS, int DC>
inline hipError_t launch_predict_adj(const PredictAdjArgs &a, hipStream_t s)
{
    if (DC > 0 && a.D != DC) return hipErrorInvalidValue;
    if (a.geo.wave != (2 * a.D <= 64 ? 1 : 0) || a.geo.E < 1 || a.geo.E > PREDICT_ADJ_MAX_E) return hipErrorInvalidValue;
    if (a.geo.lds_bytes > PREDICT_ADJ_LDS_LIMIT || !a.ckpt) return hipErrorInvalidValue;
    if (a.geo.wave) {
        if constexpr (DC == 0 || 2 * DC <= 64) {
            if (a.geo.E != 1 || a.geo.threads != 64) return hipErrorInvalidValue;
            hipLaunchKernelGGL((k_predict_adj<RHS, 1, true>), dim3((unsigned)a.geo.grid), dim3(64), a.geo.lds_bytes, s, a);
            return hipGetLastError();
        }
        return hipErrorInvalidValue;
    }
    switch (a.geo.E) {
    case 1: return launch_predict_adj_e<RHS, 1, DC>(a, s);
    case 2: return launch_predict_adj_e<RHS, 2, DC>(a, s);
    case 3: return launch_predict_adj_e<RHS, 3, DC>(a, s);
    case 4: return launch_predict_adj_e<RHS, 4, DC>(a, s);
    case 5: return launch_predict_adj_e<RHS, 5, DC>(a, s);
    case 6: return launch_predict_adj_e<RHS, 6, DC>(a, s);
    case 7: return launch_predict_adj_e<RHS, 7, DC>(a, s);
    default: return launch_predict_adj_e<RHS, 8, DC>(a, s);
    }
}

}  // namespace va
#endif
