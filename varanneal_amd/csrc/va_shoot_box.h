// va_shoot_box.h -- strong-constraint shooting INSIDE A BOX on the device: k_shoot's launch (va_shoot.h), with L-BFGS-B in
// the place of the unbounded L-BFGS step.  For T points (x0, p) the whole minimisation of the misfit of the model's RK4
// trajectory subject to lower <= (x0, p_est) <= upper, in ONE launch.
//
// A workgroup carries the points plan_shoot_box gives it (va_shoot_geo.h: plan_shoot's geometry) and loops as k_shoot does:
//   a. evaluate   shoot_eval, exactly as k_shoot calls it: va_predict_adj.h's phases, called and not copied.
//   b. step       lane r owns point r and runs the published algorithm (Byrd, Lu, Nocedal & Zhu 1995; Algorithm 778 in its
//                 3.0 form with Morales & Nocedal's projection step, the one SciPy runs) between evaluations:
//                   start     the start is projected onto the box BEFORE the first evaluation (as SciPy clips x0):
//                             cost_start is the cost of the PROJECTED start.  The projected-gradient norm sbgnrm takes
//                             max|g|'s place in the gtol test, and is what grad_max returns, at the returned point.
//                   matupd / formt   S'Y, S'S and the factor of T = theta S'S + L D^-1 L', per point
//                   cauchy    the generalised Cauchy point; breakpoints in increasing order from the serial heap, equal
//                             breakpoints by index, so the order is fixed
//                   formk / cmprlb   the reduced middle matrix over the free set.  WN1's inner-product blocks are kept
//                             incrementally as the Fortran keeps them: an accepted pair adds one row and column, variables
//                             that enter or leave the free set add and subtract their terms.  They are formed over all n
//                             only when an iteration had to skip formk (nothing free) while a pair or a change of the free
//                             set was pending: the Fortran leaves WN1 stale there.
//                   subsm     subspace minimisation with the 3.0 projection / backtrack step; skipped when nothing is
//                             free at the Cauchy point
//                   a singular factor empties the memory and forms the direction once more; status 2 if it was empty
//                             already (shoot_begin_search's two-pass rule)
//                   lnsrlb    d = z - x; stpmx from the bounds along d (1 at iteration 0 of a problem with any bound);
//                             first step min(1 / |d|, stpmx) at iteration 0 unless every entry has a two-sided box, else
//                             1; dcsrch (va_core.h) with shoot_step's constants 1e-3, 0.9, 0.1 and the upper limit stpmx;
//                             the trial at step 1 is z itself, any other trial is clamped to the box entry by entry, so
//                             every point that is ever evaluated or returned satisfies lower <= x <= upper exactly
//                   the pair is kept when dr > epsmch ddum
//                 maxiter, maxfun, maxls, ftol, the trip bound maxfun + 2, freezing and status 3 work as in shoot_step /
//                 shoot_final.  A finite, feasible iterate comes back in every case.
//                 Every sum runs over the n = D + NPest variables (or over the free / active index lists, which are in
//                 index order) on the point's own lane: no atomics, the same bits every call and whoever shares the launch.
//   c. end        as k_shoot.
// The two things va_shoot.h lists as different from SciPy's driver hold here too: the budget test inside a line search
// (nfev <= maxfun + 1), and a non-finite cost ending a search as a failed one (status 3 at the first evaluation).
//
// Bounds: lower, upper of n entries, D state columns then the estimated parameters in Pidx order; -inf / +inf: none; one
// table for all points (box_shared) or one per point.  The dense 2m x 2m algebra indexes the point's workspace in global
// memory (shoot_box_point_doubles): no local array is sized by m.
//
// shoot_box_host drives the same phases lane by lane on the CPU (tests/cpu_emul/shoot_box_check.cpp).
#pragma once
#include <math.h>

#include "va_shoot.h"

namespace va {

struct ShootBoxArgs {
    ShootArgs sh;                  // as k_shoot's, but sh.st is not used (NULL)
    ShootBoxState *st;             // [T]
    const double *lower, *upper;   // [n], or [T][n] when every point has its own box
    int box_shared;
};

// one point's workspace (va_shoot_geo.h) and box
struct SbCtx {
    double *w;
    const double *lo, *hi;
    int n, m;
    VA_HD double *xk() const { return w; }
    VA_HD double *gk() const { return w + n; }
    VA_HD double *d() const { return w + 2 * (size_t)n; }
    VA_HD double *z() const { return w + 3 * (size_t)n; }
    VA_HD double *r() const { return w + 4 * (size_t)n; }
    VA_HD double *t() const { return w + 5 * (size_t)n; }
    VA_HD double *xp() const { return w + 6 * (size_t)n; }
    VA_HD double *ws() const { return w + 7 * (size_t)n; }
    VA_HD double *wy() const { return ws() + (size_t)m * n; }
    VA_HD double *sy() const { return wy() + (size_t)m * n; }
    VA_HD double *ss() const { return sy() + (size_t)m * m; }
    VA_HD double *wt() const { return ss() + (size_t)m * m; }
    VA_HD double *wn() const { return wt() + (size_t)m * m; }
    VA_HD double *wn1() const { return wn() + 4 * (size_t)m * m; }
    VA_HD double *wa() const { return wn1() + 4 * (size_t)m * m; }
    VA_HD int *iwhere() const { return reinterpret_cast<int *>(wa() + 8 * (size_t)m); }
    VA_HD int *index() const { return iwhere() + n; }
    VA_HD int *indx2() const { return iwhere() + 2 * (size_t)n; }      // cauchy's iorder; freev's entering / leaving lists
};
VA_HD SbCtx shoot_box_ctx(const ShootBoxArgs &ba, long traj)
{
    SbCtx c;
    c.n = ba.sh.adj.D + ba.sh.adj.NPest; c.m = ba.sh.m;
    c.w = ba.sh.work + (size_t)traj * ba.sh.point_doubles;
    const size_t off = ba.box_shared ? 0 : (size_t)traj * c.n;
    c.lo = ba.lower + off; c.hi = ba.upper + off;
    return c;
}

// 1-based, column-major, as the published code (and oracle/va_lbfgsb.inc.c) index them
#define SB_WS(i, j) c.ws()[((j) - 1) * (size_t)c.n + ((i) - 1)]
#define SB_WY(i, j) c.wy()[((j) - 1) * (size_t)c.n + ((i) - 1)]
#define SB_SY(i, j) c.sy()[((j) - 1) * c.m + ((i) - 1)]
#define SB_SS(i, j) c.ss()[((j) - 1) * c.m + ((i) - 1)]
#define SB_WT(i, j) c.wt()[((j) - 1) * c.m + ((i) - 1)]
#define SB_WN(i, j) c.wn()[((j) - 1) * (2 * c.m) + ((i) - 1)]
#define SB_WN1(i, j) c.wn1()[((j) - 1) * (2 * c.m) + ((i) - 1)]

// 0 none, 1 lower, 2 both, 3 upper
VA_HD int sb_nbd(double l, double u) { return l > -HUGE_VAL ? (u < HUGE_VAL ? 2 : 1) : (u < HUGE_VAL ? 3 : 0); }
VA_HD double sb_clamp(double v, double l, double u) { return fmin(fmax(v, l), u); }

// LINPACK dpofa / dtrsl on the small matrices
VA_HD int sb_dpofa(double *a, int lda, int n)
{
#define A_(i, j) a[((j) - 1) * lda + ((i) - 1)]
    for (int j = 1; j <= n; ++j) {
        double s = 0.0;
        for (int k = 1; k <= j - 1; ++k) {
            double t = A_(k, j);
            for (int q = 1; q <= k - 1; ++q) t -= A_(q, k) * A_(q, j);
            t = t / A_(k, k);
            A_(k, j) = t;
            s += t * t;
        }
        s = A_(j, j) - s;
        if (!(s > 0.0)) return j;
        A_(j, j) = sqrt(s);
    }
    return 0;
#undef A_
}
VA_HD int sb_dtrsl(const double *t, int ldt, int n, double *b, int job)
{
#define T_(i, j) t[((j) - 1) * ldt + ((i) - 1)]
    for (int j = 1; j <= n; ++j)
        if (T_(j, j) == 0.0) return j;
    if (job == 1) {
        b[n - 1] = b[n - 1] / T_(n, n);
        for (int jj = 2; jj <= n; ++jj) {
            const int j = n - jj + 1;
            const double temp = -b[j];
            for (int q = 1; q <= j; ++q) b[q - 1] += temp * T_(q, j + 1);
            b[j - 1] = b[j - 1] / T_(j, j);
        }
    } else {
        b[0] = b[0] / T_(1, 1);
        for (int j = 2; j <= n; ++j) {
            double s = 0.0;
            for (int q = 1; q <= j - 1; ++q) s += T_(q, j) * b[q - 1];
            b[j - 1] = (b[j - 1] - s) / T_(j, j);
        }
    }
    return 0;
#undef T_
}

// the 2 col x 2 col middle matrix of the compact formula times v
VA_HD int sb_bmv(const SbCtx &c, int col, const double *v, double *p)
{
    if (col == 0) return 0;
    p[col] = v[col];
    for (int i = 2; i <= col; ++i) {
        double sum = 0.0;
        for (int k = 1; k <= i - 1; ++k) sum += SB_SY(i, k) * v[k - 1] / SB_SY(k, k);
        p[col + i - 1] = v[col + i - 1] + sum;
    }
    if (sb_dtrsl(c.wt(), c.m, col, p + col, 11)) return 1;
    for (int i = 1; i <= col; ++i) p[i - 1] = v[i - 1] / sqrt(SB_SY(i, i));
    if (sb_dtrsl(c.wt(), c.m, col, p + col, 1)) return 1;
    for (int i = 1; i <= col; ++i) p[i - 1] = -p[i - 1] / sqrt(SB_SY(i, i));
    for (int i = 1; i <= col; ++i) {
        double sum = 0.0;
        for (int k = i + 1; k <= col; ++k) sum += SB_SY(k, i) * p[col + k - 1] / SB_SY(i, i);
        p[i - 1] += sum;
    }
    return 0;
}

VA_HD int sb_formt(const SbCtx &c, int col, double theta)
{
    for (int j = 1; j <= col; ++j) SB_WT(1, j) = theta * SB_SS(1, j);
    for (int i = 2; i <= col; ++i)
        for (int j = i; j <= col; ++j) {
            const int k1 = (i < j ? i : j) - 1;
            double ddum = 0.0;
            for (int k = 1; k <= k1; ++k) ddum += SB_SY(i, k) * SB_SY(j, k) / SB_SY(k, k);
            SB_WT(i, j) = ddum + theta * SB_SS(i, j);
        }
    return sb_dpofa(c.wt(), c.m, col) ? -3 : 0;
}

// the projected-gradient norm at (x, g); NaN passes through
VA_HD double sb_projgr(const SbCtx &c, const double *x, const double *g)
{
    double sbgnrm = 0.0;
    for (int i = 0; i < c.n; ++i) {
        double gi = g[i];
        const int nb = sb_nbd(c.lo[i], c.hi[i]);
        if (nb != 0) {
            if (gi < 0.0) { if (nb >= 2) gi = fmax(x[i] - c.hi[i], gi); }
            else { if (nb <= 2) gi = fmin(x[i] - c.lo[i], gi); }
        }
        sbgnrm = shoot_absmax(sbgnrm, gi);
    }
    return sbgnrm;
}

// the breakpoint heap: the least member to t[n-1], the rest re-heaped in t[0 .. n-2].  Equal breakpoints: the smaller index first
VA_HD bool sb_less(double ta, int ia, double tb, int ib) { return ta < tb || (ta == tb && ia < ib); }
VA_HD void sb_hpsolb(int n, double *t, int *iorder, int iheap)
{
    if (iheap == 0) {
        for (int k = 2; k <= n; ++k) {
            const double ddum = t[k - 1];
            const int indxin = iorder[k - 1];
            int i = k;
            while (i > 1) {
                const int j = i / 2;
                if (sb_less(ddum, indxin, t[j - 1], iorder[j - 1])) { t[i - 1] = t[j - 1]; iorder[i - 1] = iorder[j - 1]; i = j; }
                else break;
            }
            t[i - 1] = ddum; iorder[i - 1] = indxin;
        }
    }
    if (n > 1) {
        int i = 1;
        const double out = t[0], ddum = t[n - 1];
        const int indxou = iorder[0], indxin = iorder[n - 1];
        for (;;) {
            int j = i + i;
            if (j <= n - 1) {
                if (sb_less(t[j], iorder[j], t[j - 1], iorder[j - 1])) j = j + 1;
                if (sb_less(t[j - 1], iorder[j - 1], ddum, indxin)) { t[i - 1] = t[j - 1]; iorder[i - 1] = iorder[j - 1]; i = j; }
                else break;
            } else break;
        }
        t[i - 1] = ddum; iorder[i - 1] = indxin;
        t[n - 1] = out; iorder[n - 1] = indxou;
    }
}

// the generalised Cauchy point z from the iterate (xk, gk).  p, cc, wbp, v: the four quarters of wa
VA_HD int sb_cauchy(const SbCtx &c, const ShootBoxState &s, double sbgnrm)
{
    const double epsmch = 2.220446049250313e-16;
    const int n = c.n, m = c.m, col = s.col, head = s.head, col2 = 2 * col;
    const double theta = s.theta;
    const double *x = c.xk(), *g = c.gk();
    double *xcp = c.z(), *d = c.d(), *t = c.t();
    double *p = c.wa(), *cc = p + 2 * m, *wbp = p + 4 * m, *v = p + 6 * m;
    int *iwhere = c.iwhere(), *iorder = c.indx2();
    if (sbgnrm <= 0.0) { for (int i = 0; i < n; ++i) xcp[i] = x[i]; return 0; }
    int bnded = 1, nfree = n + 1, nbreak = 0, ibkmin = 0;
    double bkmin = 0.0, f1 = 0.0;
    for (int i = 0; i < col2; ++i) p[i] = 0.0;
    for (int i = 1; i <= n; ++i) {
        const double neggi = -g[i - 1], l = c.lo[i - 1], u = c.hi[i - 1];
        const int nb = sb_nbd(l, u);
        double tl = 0.0, tu = 0.0;
        int iw = iwhere[i - 1];
        if (iw != 3 && iw != -1) {
            if (nb <= 2) tl = x[i - 1] - l;
            if (nb >= 2) tu = u - x[i - 1];
            const bool xlower = nb <= 2 && tl <= 0.0, xupper = nb >= 2 && tu <= 0.0;
            iw = 0;
            if (xlower) { if (neggi <= 0.0) iw = 1; }
            else if (xupper) { if (neggi >= 0.0) iw = 2; }
            else { if (fabs(neggi) <= 0.0) iw = -3; }
            iwhere[i - 1] = iw;
        }
        xcp[i - 1] = x[i - 1];
        if (iw != 0 && iw != -1) { d[i - 1] = 0.0; continue; }
        d[i - 1] = neggi;
        f1 -= neggi * neggi;
        int pointr = head;
        for (int j = 1; j <= col; ++j) {
            p[j - 1] += SB_WY(i, pointr) * neggi;
            p[col + j - 1] += SB_WS(i, pointr) * neggi;
            pointr = pointr % m + 1;
        }
        if (nb <= 2 && nb != 0 && neggi < 0.0) {
            nbreak++; iorder[nbreak - 1] = i; t[nbreak - 1] = tl / (-neggi);
            if (nbreak == 1 || t[nbreak - 1] < bkmin) { bkmin = t[nbreak - 1]; ibkmin = nbreak; }
        } else if (nb >= 2 && neggi > 0.0) {
            nbreak++; iorder[nbreak - 1] = i; t[nbreak - 1] = tu / neggi;
            if (nbreak == 1 || t[nbreak - 1] < bkmin) { bkmin = t[nbreak - 1]; ibkmin = nbreak; }
        } else {
            nfree--; iorder[nfree - 1] = i;
            if (fabs(neggi) > 0.0) bnded = 0;
        }
    }
    if (theta != 1.0) for (int j = 0; j < col; ++j) p[col + j] *= theta;
    if (nbreak == 0 && nfree == n + 1) return 0;
    for (int j = 0; j < col2; ++j) cc[j] = 0.0;
    double f2 = -theta * f1;
    const double f2_org = f2;
    if (col > 0) {
        if (sb_bmv(c, col, p, v)) return 1;
        double dd = 0.0;
        for (int j = 0; j < col2; ++j) dd += v[j] * p[j];
        f2 -= dd;
    }
    double dtm = -f1 / f2, tsum = 0.0;
    bool all_hit = false;
    if (nbreak > 0) {
        int nleft = nbreak, iter = 1, ibp = 0;
        double tj = 0.0;
        for (;;) {
            const double tj0 = tj;
            if (iter == 1) { tj = bkmin; ibp = iorder[ibkmin - 1]; }
            else {
                if (iter == 2 && ibkmin != nbreak) { t[ibkmin - 1] = t[nbreak - 1]; iorder[ibkmin - 1] = iorder[nbreak - 1]; }
                sb_hpsolb(nleft, t, iorder, iter - 2);
                tj = t[nleft - 1]; ibp = iorder[nleft - 1];
            }
            const double dt = tj - tj0;
            if (dtm < dt) break;                               // the minimiser is inside this interval
            tsum += dt; nleft--; iter++;
            const double dibp = d[ibp - 1];
            double zibp;
            d[ibp - 1] = 0.0;
            if (dibp > 0.0) { zibp = c.hi[ibp - 1] - x[ibp - 1]; xcp[ibp - 1] = c.hi[ibp - 1]; iwhere[ibp - 1] = 2; }
            else { zibp = c.lo[ibp - 1] - x[ibp - 1]; xcp[ibp - 1] = c.lo[ibp - 1]; iwhere[ibp - 1] = 1; }
            if (nleft == 0 && nbreak == n) { dtm = dt; all_hit = true; break; }
            const double dibp2 = dibp * dibp;
            f1 = f1 + dt * f2 + dibp2 - theta * dibp * zibp;
            f2 = f2 - theta * dibp2;
            if (col > 0) {
                for (int j = 0; j < col2; ++j) cc[j] += dt * p[j];
                int pointr = head;
                for (int j = 1; j <= col; ++j) {
                    wbp[j - 1] = SB_WY(ibp, pointr);
                    wbp[col + j - 1] = theta * SB_WS(ibp, pointr);
                    pointr = pointr % m + 1;
                }
                if (sb_bmv(c, col, wbp, v)) return 1;
                double wmc = 0.0, wmp = 0.0, wmw = 0.0;
                for (int j = 0; j < col2; ++j) { wmc += cc[j] * v[j]; wmp += p[j] * v[j]; wmw += wbp[j] * v[j]; }
                for (int j = 0; j < col2; ++j) p[j] -= dibp * wbp[j];
                f1 += dibp * wmc;
                f2 += 2.0 * dibp * wmp - dibp2 * wmw;
            }
            f2 = fmax(epsmch * f2_org, f2);
            if (nleft > 0) { dtm = -f1 / f2; continue; }
            else if (bnded) { f1 = 0.0; f2 = 0.0; dtm = 0.0; }
            else dtm = -f1 / f2;
            break;
        }
    }
    if (!all_hit) {
        if (!(dtm > 0.0)) dtm = 0.0;
        tsum += dtm;
        // (a moving entry stays short of its breakpoint but for rounding: the clamp keeps z in the box to the last bit)
        for (int i = 0; i < n; ++i)
            if (d[i] != 0.0) xcp[i] = sb_clamp(xcp[i] + tsum * d[i], c.lo[i], c.hi[i]);
    }
    if (col > 0) for (int j = 0; j < col2; ++j) cc[j] += dtm * p[j];
    return 0;
}

// the free and the active variables at the Cauchy point (index: free first, in index order), who entered and who left
VA_HD bool sb_freev(const SbCtx &c, ShootBoxState &s)
{
    const int n = c.n;
    int *index = c.index(), *indx2 = c.indx2();
    const int *iwhere = c.iwhere();
    int nenter = 0, ileave = n + 1;
    if (s.iter > 0 && s.cnstnd) {
        for (int i = 1; i <= s.nfree; ++i) { const int k = index[i - 1]; if (iwhere[k - 1] > 0) { ileave--; indx2[ileave - 1] = k; } }
        for (int i = 1 + s.nfree; i <= n; ++i) { const int k = index[i - 1]; if (iwhere[k - 1] <= 0) { nenter++; indx2[nenter - 1] = k; } }
    }
    const bool wrk = ileave < n + 1 || nenter > 0 || s.updatd;
    int nfree = 0, iact = n + 1;
    for (int i = 1; i <= n; ++i) {
        if (iwhere[i - 1] <= 0) { nfree++; index[nfree - 1] = i; }
        else { iact--; index[iact - 1] = i; }
    }
    s.nfree = nfree; s.nenter = nenter; s.ileave = ileave;
    return wrk;
}

// LEL' factorisation of the reduced middle matrix.  WN1 = [Y'ZZ'Y  L_a' + R_z'; L_a + R_z  S'AA'S] (lower triangle) is
// brought up to date first: one new row and column for an accepted pair, the terms of entering and leaving variables
VA_HD int sb_formk(const SbCtx &c, ShootBoxState &s)
{
    const int n = c.n, m = c.m, m2 = 2 * m, col = s.col, head = s.head, nsub = s.nfree;
    const double theta = s.theta;
    const int *ind = c.index(), *indx2 = c.indx2();
    if (!s.wnsync) {
        // every block over all n (an earlier iteration skipped this routine with work pending)
        int ipntr = head;
        for (int iy = 1; iy <= col; ++iy) {
            const int is = m + iy;
            int jpntr = head;
            for (int jy = 1; jy <= iy; ++jy) {
                double temp1 = 0.0, temp2 = 0.0;
                for (int k = 1; k <= nsub; ++k) { const int k1 = ind[k - 1]; temp1 += SB_WY(k1, ipntr) * SB_WY(k1, jpntr); }
                for (int k = nsub + 1; k <= n; ++k) { const int k1 = ind[k - 1]; temp2 += SB_WS(k1, ipntr) * SB_WS(k1, jpntr); }
                SB_WN1(iy, jy) = temp1; SB_WN1(is, m + jy) = temp2;
                jpntr = jpntr % m + 1;
            }
            jpntr = head;
            for (int jy = 1; jy <= col; ++jy) {
                double temp = 0.0;
                if (iy <= jy) for (int k = 1; k <= nsub; ++k) { const int k1 = ind[k - 1]; temp += SB_WS(k1, ipntr) * SB_WY(k1, jpntr); }
                else for (int k = nsub + 1; k <= n; ++k) { const int k1 = ind[k - 1]; temp += SB_WS(k1, ipntr) * SB_WY(k1, jpntr); }
                SB_WN1(is, jy) = temp;
                jpntr = jpntr % m + 1;
            }
            ipntr = ipntr % m + 1;
        }
        s.wnsync = 1;
    } else {
        int upcl = col;
        if (s.updatd) {
            if (s.iupdat > m) {                                // the oldest pair left: shift the old part of WN1
                for (int jy = 1; jy <= m - 1; ++jy) {
                    const int js = m + jy;
                    for (int q = 0; q < m - jy; ++q) {
                        SB_WN1(jy + q, jy) = SB_WN1(jy + 1 + q, jy + 1);
                        SB_WN1(js + q, js) = SB_WN1(js + 1 + q, js + 1);
                    }
                    for (int q = 0; q < m - 1; ++q) SB_WN1(m + 1 + q, jy) = SB_WN1(m + 2 + q, jy + 1);
                }
            }
            // the new row of blocks (1,1), (2,1) and (2,2)
            int ipntr = head + col - 1;
            if (ipntr > m) ipntr -= m;
            int jpntr = head;
            for (int jy = 1; jy <= col; ++jy) {
                double temp1 = 0.0, temp2 = 0.0, temp3 = 0.0;
                for (int k = 1; k <= nsub; ++k) { const int k1 = ind[k - 1]; temp1 += SB_WY(k1, ipntr) * SB_WY(k1, jpntr); }
                for (int k = nsub + 1; k <= n; ++k) {
                    const int k1 = ind[k - 1];
                    temp2 += SB_WS(k1, ipntr) * SB_WS(k1, jpntr);
                    temp3 += SB_WS(k1, ipntr) * SB_WY(k1, jpntr);
                }
                SB_WN1(col, jy) = temp1; SB_WN1(m + col, m + jy) = temp2; SB_WN1(m + col, jy) = temp3;
                jpntr = jpntr % m + 1;
            }
            // the new column of block (2,1)
            jpntr = ipntr;
            ipntr = head;
            for (int i = 1; i <= col; ++i) {
                double temp3 = 0.0;
                for (int k = 1; k <= nsub; ++k) { const int k1 = ind[k - 1]; temp3 += SB_WS(k1, ipntr) * SB_WY(k1, jpntr); }
                ipntr = ipntr % m + 1;
                SB_WN1(m + i, col) = temp3;
            }
            upcl = col - 1;
        }
        if (s.nenter > 0 || s.ileave < n + 1) {
            // the old parts, for the variables that entered (indx2[0 .. nenter)) or left (indx2[ileave - 1 .. n)) the free set
            int ipntr = head;
            for (int iy = 1; iy <= upcl; ++iy) {
                const int is = m + iy;
                int jpntr = head;
                for (int jy = 1; jy <= iy; ++jy) {
                    double temp1 = 0.0, temp2 = 0.0, temp3 = 0.0, temp4 = 0.0;
                    for (int k = 1; k <= s.nenter; ++k) {
                        const int k1 = indx2[k - 1];
                        temp1 += SB_WY(k1, ipntr) * SB_WY(k1, jpntr);
                        temp2 += SB_WS(k1, ipntr) * SB_WS(k1, jpntr);
                    }
                    for (int k = s.ileave; k <= n; ++k) {
                        const int k1 = indx2[k - 1];
                        temp3 += SB_WY(k1, ipntr) * SB_WY(k1, jpntr);
                        temp4 += SB_WS(k1, ipntr) * SB_WS(k1, jpntr);
                    }
                    SB_WN1(iy, jy) = SB_WN1(iy, jy) + temp1 - temp3;
                    SB_WN1(is, m + jy) = SB_WN1(is, m + jy) - temp2 + temp4;
                    jpntr = jpntr % m + 1;
                }
                ipntr = ipntr % m + 1;
            }
            ipntr = head;
            for (int is = m + 1; is <= m + upcl; ++is) {
                int jpntr = head;
                for (int jy = 1; jy <= upcl; ++jy) {
                    double temp1 = 0.0, temp3 = 0.0;
                    for (int k = 1; k <= s.nenter; ++k) { const int k1 = indx2[k - 1]; temp1 += SB_WS(k1, ipntr) * SB_WY(k1, jpntr); }
                    for (int k = s.ileave; k <= n; ++k) { const int k1 = indx2[k - 1]; temp3 += SB_WS(k1, ipntr) * SB_WY(k1, jpntr); }
                    if (is <= jy + m) SB_WN1(is, jy) = SB_WN1(is, jy) + temp1 - temp3;
                    else SB_WN1(is, jy) = SB_WN1(is, jy) - temp1 + temp3;
                    jpntr = jpntr % m + 1;
                }
                ipntr = ipntr % m + 1;
            }
        }
    }
    // the upper triangle of WN = [D + Y'ZZ'Y / theta  -L_a' + R_z'; -L_a + R_z  S'AA'S theta], then its factor
    for (int iy = 1; iy <= col; ++iy) {
        const int is = col + iy, is1 = m + iy;
        for (int jy = 1; jy <= iy; ++jy) {
            SB_WN(jy, iy) = SB_WN1(iy, jy) / theta;
            SB_WN(col + jy, is) = SB_WN1(is1, m + jy) * theta;
        }
        for (int jy = 1; jy <= iy - 1; ++jy) SB_WN(jy, is) = -SB_WN1(is1, jy);
        for (int jy = iy; jy <= col; ++jy) SB_WN(jy, is) = SB_WN1(is1, jy);
        SB_WN(iy, iy) += SB_SY(iy, iy);
    }
    if (sb_dpofa(c.wn(), m2, col)) return -1;
    const int col2 = 2 * col;
    for (int js = col + 1; js <= col2; ++js)
        if (sb_dtrsl(c.wn(), m2, col, &SB_WN(1, js), 11)) return -1;
    for (int is = col + 1; is <= col2; ++is)
        for (int js = is; js <= col2; ++js) {
            double sm = 0.0;
            for (int q = 1; q <= col; ++q) sm += SB_WN(q, is) * SB_WN(q, js);
            SB_WN(is, js) += sm;
        }
    if (sb_dpofa(&SB_WN(col + 1, col + 1), m2, col)) return -2;
    return 0;
}

// r = -Z'B(xcp - xk) - Z'g, on the free variables (r[i] belongs to variable index[i])
VA_HD int sb_cmprlb(const SbCtx &c, const ShootBoxState &s)
{
    const int n = c.n, m = c.m, col = s.col, nfree = s.nfree;
    const double theta = s.theta;
    const double *x = c.xk(), *g = c.gk(), *z = c.z();
    double *r = c.r(), *wa = c.wa();
    const int *index = c.index();
    if (!s.cnstnd && col > 0) { for (int i = 0; i < n; ++i) r[i] = -g[i]; return 0; }
    for (int i = 1; i <= nfree; ++i) { const int k = index[i - 1]; r[i - 1] = -theta * (z[k - 1] - x[k - 1]) - g[k - 1]; }
    if (sb_bmv(c, col, wa + 2 * m, wa)) return -8;
    int pointr = s.head;
    for (int j = 1; j <= col; ++j) {
        const double a1 = wa[j - 1], a2 = theta * wa[col + j - 1];
        for (int i = 1; i <= nfree; ++i) { const int k = index[i - 1]; r[i - 1] += SB_WY(k, pointr) * a1 + SB_WS(k, pointr) * a2; }
        pointr = pointr % m + 1;
    }
    return 0;
}

// subspace minimisation over the free variables from the Cauchy point z, then L-BFGS-B 3.0's projection / backtrack
VA_HD int sb_subsm(const SbCtx &c, const ShootBoxState &s)
{
    const int n = c.n, m = c.m, m2 = 2 * m, col = s.col, col2 = 2 * col, nsub = s.nfree;
    const double theta = s.theta;
    const int *ind = c.index();
    double *x = c.z(), *d = c.r(), *xp = c.xp(), *wv = c.wa();
    const double *xx = c.xk(), *gg = c.gk();
    if (nsub <= 0) return 0;
    int pointr = s.head;
    for (int i = 1; i <= col; ++i) {
        double temp1 = 0.0, temp2 = 0.0;
        for (int j = 1; j <= nsub; ++j) { const int k = ind[j - 1]; temp1 += SB_WY(k, pointr) * d[j - 1]; temp2 += SB_WS(k, pointr) * d[j - 1]; }
        wv[i - 1] = temp1; wv[col + i - 1] = theta * temp2;
        pointr = pointr % m + 1;
    }
    if (sb_dtrsl(c.wn(), m2, col2, wv, 11)) return 1;
    for (int i = 0; i < col; ++i) wv[i] = -wv[i];
    if (sb_dtrsl(c.wn(), m2, col2, wv, 1)) return 1;
    pointr = s.head;
    for (int jy = 1; jy <= col; ++jy) {
        const int js = col + jy;
        for (int i = 1; i <= nsub; ++i) { const int k = ind[i - 1]; d[i - 1] += SB_WY(k, pointr) * wv[jy - 1] / theta + SB_WS(k, pointr) * wv[js - 1]; }
        pointr = pointr % m + 1;
    }
    for (int i = 0; i < nsub; ++i) d[i] *= 1.0 / theta;
    int iword = 0;
    for (int i = 0; i < n; ++i) xp[i] = x[i];
    for (int i = 1; i <= nsub; ++i) {
        const int k = ind[i - 1];
        const double dk = d[i - 1], xk = x[k - 1], l = c.lo[k - 1], u = c.hi[k - 1];
        const int nb = sb_nbd(l, u);
        double xn = xk + dk;
        if (nb == 1) { xn = fmax(l, xn); if (xn == l) iword = 1; }
        else if (nb == 2) { xn = fmin(u, fmax(l, xn)); if (xn == l || xn == u) iword = 1; }
        else if (nb == 3) { xn = fmin(u, xn); if (xn == u) iword = 1; }
        x[k - 1] = xn;
    }
    if (iword == 0) return 0;
    double dd_p = 0.0;
    for (int i = 0; i < n; ++i) dd_p += (x[i] - xx[i]) * gg[i];
    if (dd_p > 0.0) {
        // the projected point does not descend: back to the Cauchy point, and a truncated step along d
        for (int i = 0; i < n; ++i) x[i] = xp[i];
        double alpha = 1.0, temp1 = alpha;
        int ibd = 0;
        for (int i = 1; i <= nsub; ++i) {
            const int k = ind[i - 1];
            const double dk = d[i - 1], l = c.lo[k - 1], u = c.hi[k - 1];
            const int nb = sb_nbd(l, u);
            if (nb != 0) {
                if (dk < 0.0 && nb <= 2) {
                    const double temp2 = l - x[k - 1];
                    if (temp2 >= 0.0) temp1 = 0.0; else if (dk * alpha < temp2) temp1 = temp2 / dk;
                } else if (dk > 0.0 && nb >= 2) {
                    const double temp2 = u - x[k - 1];
                    if (temp2 <= 0.0) temp1 = 0.0; else if (dk * alpha > temp2) temp1 = temp2 / dk;
                }
                if (temp1 < alpha) { alpha = temp1; ibd = i; }
            }
        }
        if (alpha < 1.0) {
            const double dk = d[ibd - 1];
            const int k = ind[ibd - 1];
            if (dk > 0.0) { x[k - 1] = c.hi[k - 1]; d[ibd - 1] = 0.0; }
            else if (dk < 0.0) { x[k - 1] = c.lo[k - 1]; d[ibd - 1] = 0.0; }
        }
        for (int i = 1; i <= nsub; ++i) { const int k = ind[i - 1]; x[k - 1] = sb_clamp(x[k - 1] + alpha * d[i - 1], c.lo[k - 1], c.hi[k - 1]); }
    }
    return 0;
}

// the accepted pair (S = stp d, Y = r) enters the ring, S'Y and S'S
VA_HD void sb_matupd(const SbCtx &c, ShootBoxState &s, double rr, double dr, double stp)
{
    const int n = c.n, m = c.m;
    s.iupdat += 1;
    if (s.iupdat <= m) { s.col = s.iupdat; s.itail = (s.head + s.iupdat - 2) % m + 1; }
    else { s.itail = s.itail % m + 1; s.head = s.head % m + 1; }
    const double *d = c.d(), *r = c.r();
    for (int i = 1; i <= n; ++i) { SB_WS(i, s.itail) = stp * d[i - 1]; SB_WY(i, s.itail) = r[i - 1]; }
    s.theta = rr / dr;
    const int col = s.col;
    if (s.iupdat > m) {
        for (int j = 1; j <= col - 1; ++j) {
            for (int q = 1; q <= j; ++q) SB_SS(q, j) = SB_SS(q + 1, j + 1);
            for (int q = 0; q < col - j; ++q) SB_SY(j + q, j) = SB_SY(j + 1 + q, j + 1);
        }
    }
    int pointr = s.head;
    for (int j = 1; j <= col - 1; ++j) {
        double a = 0.0, b = 0.0;
        for (int i = 1; i <= n; ++i) { const double sn = SB_WS(i, s.itail); a += sn * SB_WY(i, pointr); b += SB_WS(i, pointr) * sn; }
        SB_SY(col, j) = a; SB_SS(j, col) = b;
        pointr = pointr % m + 1;
    }
    SB_SS(col, col) = stp == 1.0 ? s.dtd : stp * stp * s.dtd;
    SB_SY(col, col) = dr;
}

VA_HD void sb_reset(ShootBoxState &s) { s.col = 0; s.head = 1; s.itail = 0; s.theta = 1.0; s.iupdat = 0; s.updatd = 0; s.wnsync = 1; }

// z, the point the line search aims at: the Cauchy point, moved on by the subspace step.  != 0: a singular factor
VA_HD int sb_direction(const SbCtx &c, ShootBoxState &s)
{
    bool wrk;
    if (!s.cnstnd && s.col > 0) {
        const double *x = c.xk();
        double *z = c.z();
        for (int i = 0; i < c.n; ++i) z[i] = x[i];
        wrk = s.updatd != 0;
    } else {
        if (sb_cauchy(c, s, s.gmax)) return 1;
        wrk = sb_freev(c, s);
    }
    if (s.nfree != 0 && s.col != 0) {
        if (wrk || !s.wnsync) { if (sb_formk(c, s)) return 2; }
        if (sb_cmprlb(c, s)) return 3;
        return sb_subsm(c, s) ? 4 : 0;
    }
    if (s.col != 0 && wrk) s.wnsync = 0;       // formk was due and did not run: WN1 misses this iteration's changes
    return 0;
}

VA_HD void shoot_box_finish(ShootBoxState &s, double *done, int r, int status) { s.status = status; s.phase = SH_DONE; done[r] = 1.0; }
VA_HD void shoot_box_restore(const ShootBoxArgs &ba, const SbCtx &c, long traj)
{
    const double *xk = c.xk();
    for (int i = 0; i < c.n; ++i) *shoot_xp(ba.sh, traj, i) = xk[i];
}

// a new search from the iterate: z, d = z - x, stpmx, the first step, dcsrch's start, the first trial into (x0, p)
VA_HD void shoot_box_begin_search(const ShootBoxArgs &ba, ShootBoxState &s, const SbCtx &c, long traj, double *done, int r)
{
    const int n = c.n;
    for (int pass = 0; pass < 2; ++pass) {
        if (sb_direction(c, s) == 0) {
            const double *x = c.xk(), *g = c.gk(), *z = c.z();
            double *d = c.d();
            double dtd = 0.0, gd = 0.0, stpmx = 1e10;
            for (int i = 0; i < n; ++i) {
                const double di = z[i] - x[i];
                d[i] = di;
                dtd += di * di; gd += g[i] * di;
                if (s.cnstnd && s.iter != 0) {
                    const double l = c.lo[i], u = c.hi[i];
                    const int nb = sb_nbd(l, u);
                    if (nb != 0) {
                        if (di < 0.0 && nb <= 2) { const double a2 = l - x[i]; if (a2 >= 0.0) stpmx = 0.0; else if (di * stpmx < a2) stpmx = a2 / di; }
                        else if (di > 0.0 && nb >= 2) { const double a2 = u - x[i]; if (a2 <= 0.0) stpmx = 0.0; else if (di * stpmx > a2) stpmx = a2 / di; }
                    }
                }
            }
            if (s.cnstnd && s.iter == 0) stpmx = 1.0;
            double stp = (s.iter == 0 && !s.boxed) ? fmin(1.0 / sqrt(dtd), stpmx) : 1.0;
            LsState ls = LsState();
            int task = LS_ERROR;
            if (gd < 0.0) task = dcsrch(s.f, gd, stp, 1e-3, 0.9, 0.1, 0.0, stpmx, LS_START, ls);
            if (task != LS_ERROR) {
                s.gdold = gd; s.stp = stp; s.stpmx = stpmx; s.dtd = dtd; s.ls = ls; s.nls = 0; s.phase = SH_LS;
                for (int i = 0; i < n; ++i)
                    *shoot_xp(ba.sh, traj, i) = stp == 1.0 ? z[i] : sb_clamp(trial(x[i], stp, d[i]), c.lo[i], c.hi[i]);
                return;
            }
        }
        if (s.col == 0) break;
        sb_reset(s);
    }
    shoot_box_restore(ba, c, traj);
    shoot_box_finish(s, done, r, 2);
}

// before the first evaluation: lane r arms point r and projects its start onto the box, or marks an idle slot as done
VA_HD void shoot_box_init(const ShootBoxArgs &ba, double *done, long wg, int tid)
{
    const PredictAdjArgs &a = ba.sh.adj;
    if (tid >= a.geo.RW) return;
    const long traj = predict_adj_work(a, wg).group * a.geo.RW + tid;
    if (traj >= a.T) { done[tid] = 1.0; return; }
    ShootBoxState s = ShootBoxState();
    s.phase = SH_START;
    sb_reset(s);
    ba.st[traj] = s;
    const SbCtx c = shoot_box_ctx(ba, traj);
    for (int i = 0; i < c.n; ++i) {
        double *x = shoot_xp(ba.sh, traj, i);
        const double v = *x;
        if (v < c.lo[i]) *x = c.lo[i];
        else if (v > c.hi[i]) *x = c.hi[i];
    }
    done[tid] = 0.0;
}

// the step: lane r consumes the evaluation of point r's trial
VA_HD void shoot_box_step(const ShootBoxArgs &ba, double *done, long wg, int tid)
{
    const ShootArgs &sa = ba.sh;
    const PredictAdjArgs &a = sa.adj;
    if (tid >= a.geo.RW) return;
    const long traj = predict_adj_work(a, wg).group * a.geo.RW + tid;
    if (traj >= a.T) return;
    ShootBoxState &s = ba.st[traj];
    if (s.phase == SH_DONE) return;
    const double epsmch = 2.220446049250313e-16;
    const SbCtx c = shoot_box_ctx(ba, traj);
    const int n = c.n;
    double *xk = c.xk(), *gk = c.gk();
    const double ft = a.cost[traj];
    if (s.phase == SH_START) {
        s.f = ft; s.f_start = ft; s.nfev = 1;
        int *iwhere = c.iwhere();
        int cnstnd = 0, boxed = 1;
        for (int i = 0; i < n; ++i) {
            gk[i] = shoot_g(a, traj, i); xk[i] = *shoot_xp(sa, traj, i);
            const int nb = sb_nbd(c.lo[i], c.hi[i]);
            if (nb != 2) boxed = 0;
            if (nb == 0) iwhere[i] = -1;
            else { cnstnd = 1; iwhere[i] = (nb == 2 && c.hi[i] - c.lo[i] <= 0.0) ? 3 : 0; }
        }
        s.cnstnd = cnstnd; s.boxed = boxed; s.nfree = n;
        s.gmax = sb_projgr(c, xk, gk);
        if (!shoot_finite(ft)) { shoot_box_finish(s, done, tid, 3); return; }
        if (s.gmax <= sa.gtol) { shoot_box_finish(s, done, tid, 0); return; }
        shoot_box_begin_search(ba, s, c, traj, done, tid);
        return;
    }
    s.nfev += 1;
    const double *d = c.d();
    double gd = 0.0;
    for (int i = 0; i < n; ++i) gd += shoot_g(a, traj, i) * d[i];
    const double stp_eval = s.stp;
    bool fail = !shoot_finite(ft) || !shoot_finite(gd);
    if (!fail) {
        LsState ls = s.ls;
        double stp = stp_eval;
        const int task = dcsrch(ft, gd, stp, 1e-3, 0.9, 0.1, 0.0, s.stpmx, LS_FG, ls);
        if (task == LS_FG) {
            s.nls += 1;
            if (s.nls >= sa.maxls) fail = true;
            else if (s.nfev > sa.maxfun) { shoot_box_restore(ba, c, traj); shoot_box_finish(s, done, tid, 1); return; }
            else {
                s.ls = ls; s.stp = stp;
                const double *z = c.z();
                for (int i = 0; i < n; ++i)
                    *shoot_xp(sa, traj, i) = stp == 1.0 ? z[i] : sb_clamp(trial(xk[i], stp, d[i]), c.lo[i], c.hi[i]);
                return;
            }
        }
    }
    if (fail) {
        if (s.col == 0) { shoot_box_restore(ba, c, traj); shoot_box_finish(s, done, tid, 2); return; }
        sb_reset(s);                                       // (the iterate, its gradient and cost were not touched)
        shoot_box_begin_search(ba, s, c, traj, done, tid);
        return;
    }
    // the trial is the new iterate; r = its gradient's change
    const double fold = s.f;
    s.f = ft; s.iter += 1;
    double *r = c.r();
    double rr = 0.0;
    for (int i = 0; i < n; ++i) {
        const double g = shoot_g(a, traj, i), y = g - gk[i];
        r[i] = y; rr += y * y;
        gk[i] = g; xk[i] = *shoot_xp(sa, traj, i);
    }
    s.gmax = sb_projgr(c, xk, gk);
    if (s.iter >= sa.maxiter || s.nfev > sa.maxfun) { shoot_box_finish(s, done, tid, 1); return; }
    if (s.gmax <= sa.gtol) { shoot_box_finish(s, done, tid, 0); return; }
    if (fold - ft <= sa.ftol * fmax(fmax(fabs(fold), fabs(ft)), 1.0)) { shoot_box_finish(s, done, tid, 0); return; }
    const double dr = (gd - s.gdold) * stp_eval, ddum = -s.gdold * stp_eval;
    if (dr > epsmch * ddum) {
        s.updatd = 1;
        sb_matupd(c, s, rr, dr, stp_eval);
        if (sb_formt(c, s.col, s.theta)) sb_reset(s);
    } else s.updatd = 0;
    shoot_box_begin_search(ba, s, c, traj, done, tid);
}

// behind the loop: a point the trip bound stopped returns its iterate with status 1
VA_HD void shoot_box_final(const ShootBoxArgs &ba, double *done, long wg, int tid)
{
    const PredictAdjArgs &a = ba.sh.adj;
    if (tid >= a.geo.RW) return;
    const long traj = predict_adj_work(a, wg).group * a.geo.RW + tid;
    if (traj >= a.T) return;
    ShootBoxState &s = ba.st[traj];
    if (s.phase == SH_DONE) return;
    if (s.phase == SH_LS) shoot_box_restore(ba, shoot_box_ctx(ba, traj), traj);
    shoot_box_finish(s, done, tid, 1);
}

#undef SB_WS
#undef SB_WY
#undef SB_SY
#undef SB_SS
#undef SB_WT
#undef SB_WN
#undef SB_WN1

// ---------------------------------------------------------------- the same phases, lane by lane on the host
// (every pointer of `ba` is host memory)
template <class RHS, int E>
inline void shoot_box_host_e(const ShootBoxArgs &ba)
{
    const PredictAdjArgs &a = ba.sh.adj;
    const int nt = a.geo.threads;
    std::vector<double> mem(predict_adj_lds_doubles(a.geo.RW, a.geo.chunk, a.D, a.NP, a.nstim) + a.geo.RW + 1, 0.0);
    std::vector<PredictAdjLane<E>> L(nt);
    const PredictAdjLds l = predict_adj_lds(a, mem.data());
    double *done = shoot_done_flags(a, l);
    for (long wg = 0; wg < a.geo.grid; ++wg) {
        for (int tid = 0; tid < nt; ++tid) shoot_box_init(ba, done, wg, tid);
        for (int trip = 0; trip < shoot_trips(ba.sh); ++trip) {
            shoot_eval_host<RHS, E>(a, l, wg, L);
            for (int tid = 0; tid < nt; ++tid) shoot_box_step(ba, done, wg, tid);
            if (shoot_all_done(a, done)) break;
        }
        for (int tid = 0; tid < nt; ++tid) shoot_box_final(ba, done, wg, tid);
    }
}

template <class RHS>
inline void shoot_box_host(const ShootBoxArgs &ba)
{
    switch (ba.sh.adj.geo.E) {
    case 1: shoot_box_host_e<RHS, 1>(ba); break;
    case 2: shoot_box_host_e<RHS, 2>(ba); break;
    case 3: shoot_box_host_e<RHS, 3>(ba); break;
    default: shoot_box_host_e<RHS, 4>(ba); break;
    }
}

}  // namespace va

// ---------------------------------------------------------------- the kernel
#if defined(__HIPCC__)

namespace va {

// k_shoot's loop; the barriers around the step order global memory as they do there
template <class RHS, int E, bool WAVE>
__global__ __launch_bounds__(WAVE ? 64 : 256) void k_shoot_box(const ShootBoxArgs ba)
{
    extern __shared__ __attribute__((aligned(16))) double shoot_box_mem[];
    const PredictAdjArgs &a = ba.sh.adj;
    const PredictAdjLds l = predict_adj_lds(a, shoot_box_mem);
    double *done = shoot_done_flags(a, l);
    const int tid = (int)threadIdx.x;
    const long wg = (long)blockIdx.x;
    const PredictAdjStep hs = predict_adj_step_sizes(a.dt, a.substeps);
    shoot_box_init(ba, done, wg, tid);
    __syncthreads();
    const int trips = shoot_trips(ba.sh);
    for (int trip = 0; trip < trips; ++trip) {
        shoot_eval<RHS, E, WAVE>(a, l, wg, tid, hs);
        __syncthreads();
        shoot_box_step(ba, done, wg, tid);
        __syncthreads();
        if (shoot_all_done(a, done)) break;      // (the same LDS words for every lane: uniform)
    }
    shoot_box_final(ba, done, wg, tid);
}

template <class RHS, int E, int DC>
inline hipError_t launch_shoot_box_e(const ShootBoxArgs &ba, size_t lds_bytes, hipStream_t s)
{
    constexpr bool can = DC == 0 || (DC > 32 && DC <= SHOOT_MAX_D && shoot_e_of(DC) == E);
    if constexpr (can) {
        hipLaunchKernelGGL((k_shoot_box<RHS, E, false>), dim3((unsigned)ba.sh.adj.geo.grid), dim3((unsigned)ba.sh.adj.geo.threads), lds_bytes, s, ba);
        return hipGetLastError();
    }
    return hipErrorInvalidValue;      // (a geometry plan_shoot_box does not make for this D)
}

// launch the instantiation ba.sh.adj.geo names; DC as in launch_shoot
template <class RHS, int DC>
inline hipError_t launch_shoot_box(const ShootBoxArgs &ba, hipStream_t s)
{
    const ShootArgs &sa = ba.sh;
    const PredictAdjArgs &a = sa.adj;
    const PredictAdjGeo &g = a.geo;
    if (DC > 0 && a.D != DC) return hipErrorInvalidValue;
    if (a.D < 1 || a.D > SHOOT_MAX_D || a.ncot != 1 || a.G || !a.Y || g.nchunks != 1 || g.chunk != 1) return hipErrorInvalidValue;
    if (g.wave != (2 * a.D <= 64 ? 1 : 0) || g.E < 1 || g.E > PREDICT_MAX_E || g.RW < 1 || g.RW > g.threads) return hipErrorInvalidValue;
    if (sa.m < 1 || sa.m > MAX_M || sa.maxfun < 1 || sa.maxfun > SHOOT_MAX_FUN) return hipErrorInvalidValue;
    if (sa.point_doubles < shoot_box_point_doubles(a.D + a.NPest, sa.m)) return hipErrorInvalidValue;
    const size_t lds_bytes = g.lds_bytes + sizeof(double) * (size_t)g.RW;
    if (lds_bytes > PREDICT_ADJ_LDS_LIMIT || !a.ckpt || !sa.x || !ba.st || !sa.work || !ba.lower || !ba.upper) return hipErrorInvalidValue;
    if (g.wave) {
        if constexpr (DC == 0 || 2 * DC <= 64) {
            if (g.E != 1 || g.threads != 64) return hipErrorInvalidValue;
            hipLaunchKernelGGL((k_shoot_box<RHS, 1, true>), dim3((unsigned)g.grid), dim3(64), lds_bytes, s, ba);
            return hipGetLastError();
        }
        return hipErrorInvalidValue;
    }
    switch (g.E) {
    case 1: return launch_shoot_box_e<RHS, 1, DC>(ba, lds_bytes, s);
    case 2: return launch_shoot_box_e<RHS, 2, DC>(ba, lds_bytes, s);
    case 3: return launch_shoot_box_e<RHS, 3, DC>(ba, lds_bytes, s);
    default: return launch_shoot_box_e<RHS, 4, DC>(ba, lds_bytes, s);
    }
}

}  // namespace va
#endif
