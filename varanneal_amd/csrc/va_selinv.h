// va_selinv.h -- selected inverse and log-determinant of a block-tridiagonal matrix with a dense border (an "arrow"): the
// Hessian of the action in [X | p_est], time rows grouped into K blocks of width W (va_selinv_geo.h).
//
//     forward, k = 0 .. K-1     C_k = chol(S),  R = P_k - F_{k-1} E_{k-1}^T,  F_k = R C_k^-T,
//                               E_k = B_k C_k^-T,  S = D_{k+1} - E_k E_k^T                        (S = D_0 at k = 0)
//     parameters                S_p = H_pp - sum_k F_k F_k^T,  C_p = chol(S_p),  Sigma_pp = S_p^-1
//                               logdet = 2 sum log diag(C_k) + 2 sum log diag(C_p)
//     backward, k = K-1 .. 0    Ge = E_k C_k^-1,  Gf = F_k C_k^-1                                 (Takahashi's recurrence on the
//                               Sigma_{k+1,k} = -(Sigma_{k+1,k+1} Ge + Sigma_{p,k+1}^T Gf)         factor's own pattern)
//                               Sigma_{p,k}   = -(Sigma_{p,k+1} Ge + Sigma_pp Gf)
//                               Sigma_kk      = C_k^-T C_k^-1 - Sigma_{k+1,k}^T Ge - Sigma_{p,k}^T Gf
// The blocks of the inverse that lie on the pattern come out exactly as the dense inverse has them; nothing else is formed.
//
// One workgroup owns one point.  The current blocks live in LDS, the factor (C_k, E_k, F_k) streams to the point's
// workspace in global memory on the way forward, with the pivots it took the roots of, and is read back on the way down.
// selinv_point is written ONCE, over an executor: ex.par(f) runs f(tid, nt) for every thread and then joins them -- on the device each thread calls f and meets
// the others at a barrier, on the host (selinv_host; tests/cpu_emul/selinv_check.cpp) the threads run one after the other.
// Nothing is carried in registers from one par to the next, and every sum runs in index order in ONE thread: the same
// inputs give the same bits on every call, on either side.
//
// A pivot that is <= 0 or NaN ends the point: status k + 1 (path block k) or -1 (the parameters' Schur complement), every
// requested output of the point NaN.  status 0: fine.
//
// k_hblocks cuts D_k, B_k, P_k, H_pp from the coloured Hessian-vector products k_hvp leaves on the device (index map:
// va_selinv_geo.h hblocks_src), k_hcolour writes those directions, k_laplace_unpack takes the padding out again.
#pragma once
#include <math.h>

#include <vector>

#include "va_core.h"
#include "va_selinv_geo.h"

namespace va {

struct SelinvArgs {
    SelinvGeo g;
    const double *Dk, *Bk, *Pk, *Hpp;      // [npts][K][W][W], [npts][K-1][W][W] (B_k = H_{k+1,k}), [npts][K][NPe][W], [npts][NPe][NPe]
    double *Skk, *Snk, *Spk, *Spp;         // the same shapes; any of them NULL: not written
    double *logdet;                        // [npts]
    int *status;                           // [npts]
    double *ws;                            // [npts][g.ws_doubles]
    int npts;
};

static_assert(SELINV_THREADS == 256, "the trailing update of the in-block Cholesky maps the threads 16 x 16");

// ---------------------------------------------------------------- phases (one thread's share each)
// global [rows][cols] dense <-> an LDS image at row pitch `pitch`
VA_HD void blk_load(double *dst, int pitch, const double *src, int rows, int cols, int tid, int nt)
{
    const int tot = rows * cols;
    for (int e = tid; e < tot; e += nt) { const int i = e / cols, j = e - i * cols; dst[i * pitch + j] = src[e]; }
}
VA_HD void blk_store(double *dst, const double *src, int pitch, int rows, int cols, int tid, int nt)
{
    const int tot = rows * cols;
    for (int e = tid; e < tot; e += nt) { const int i = e / cols, j = e - i * cols; dst[e] = src[i * pitch + j]; }
}
VA_HD void blk_identity(double *dst, int pitch, int n, int tid, int nt)
{
    const int tot = n * n;
    for (int e = tid; e < tot; e += nt) { const int i = e / n, j = e - i * n; dst[i * pitch + j] = (i == j) ? 1.0 : 0.0; }
}
VA_HD void fill_value(double *dst, long n, double v, int tid, int nt)
{
    if (!dst) return;
    for (long e = tid; e < n; e += nt) dst[e] = v;
}

// in-block Cholesky, column j, first half: the column under the pivot p = S[j][j] (read by every thread before this par)
VA_HD void chol_scale(double *S, int pitch, int n, int j, double c, int tid, int nt)
{
    for (int i = j + 1 + tid; i < n; i += nt) S[i * pitch + j] = S[i * pitch + j] / c;
}
// second half: the pivot itself, its share of the log-determinant, and the trailing lower triangle S[i][l] -= S[i][j] S[l][j]
VA_HD void chol_update(double *S, int pitch, int n, int j, double p, double c, double *piv, double *ld, int tid)
{
    if (tid == 0) { S[j * pitch + j] = c; piv[j] = p; *ld += 2.0 * log(c); }
    const int ty = tid >> 4, tx = tid & 15;
    for (int i = j + 1 + ty; i < n; i += 16) {
        const double sij = S[i * pitch + j];
        for (int l = j + 1 + tx; l <= i; l += 16) S[i * pitch + l] -= sij * S[l * pitch + j];
    }
}
// row r of X := X C^-T in place (C lower, pitch cp): X[r][j] = (X[r][j] - sum_{i<j} X[r][i] C[j][i]) / C[j][j]
VA_HD void row_solve_ct(double *x, const double *C, int cp, int n)
{
    for (int j = 0; j < n; ++j) {
        double v = x[j];
        for (int i = 0; i < j; ++i) v -= x[i] * C[j * cp + i];
        x[j] = v / C[j * cp + j];
    }
}
// row r of C^-1, in place on a row of the identity: X[r][j] = ((r == j) - sum_{j<i<=r} X[r][i] C[i][j]) / C[j][j], j = r .. 0
VA_HD void row_inverse(double *x, const double *C, int cp, int r)
{
    for (int j = r; j >= 0; --j) {
        double v = x[j];
        for (int i = j + 1; i <= r; ++i) v -= x[i] * C[i * cp + j];
        x[j] = v / C[j * cp + j];
    }
}
// row r of X := X Ci in place (Ci lower, pitch cp): X[r][j] = sum_{i>=j} X[r][i] Ci[i][j], j ascending (entry j is not read again)
VA_HD void row_times_lower(double *x, const double *Ci, int cp, int n)
{
    for (int j = 0; j < n; ++j) {
        double v = 0.0;
        for (int i = j; i < n; ++i) v += x[i] * Ci[i * cp + j];
        x[j] = v;
    }
}
// (Ci^T Ci)[i][j] = sum_{l >= max(i, j)} Ci[l][i] Ci[l][j], Ci = C^-1.  On the diagonal the first term is Ci[i][i]^2 =
// 1 / c_i^2 = 1 / p_i with p_i the pivot the Cholesky took its root of: it is formed from the pivot itself (one rounding)
// and not as the square of a reciprocal root (three)
VA_HD double lower_gram(const double *Ci, int cp, int n, const double *piv, int i, int j)
{
    const int m = i > j ? i : j;
    double v = (i == j) ? 1.0 / piv[i] : Ci[m * cp + i] * Ci[m * cp + j];
    for (int l = m + 1; l < n; ++l) v += Ci[l * cp + i] * Ci[l * cp + j];
    return v;
}

// ---------------------------------------------------------------- executors
struct SelinvHostExec {
    int nt;
    template <class F> void par(F f) const { for (int t = 0; t < nt; ++t) f(t, nt); }
};
#if defined(__HIPCC__)
struct SelinvDevExec {
    template <class F> __host__ __device__ void par(F f) const
    {
#if defined(__HIP_DEVICE_COMPILE__)
        f((int)threadIdx.x, SELINV_THREADS);
        __syncthreads();
#endif
    }
};
#endif

// a failed point: every requested output NaN, the status says where it stopped
template <class X> VA_HD void selinv_fail(const SelinvArgs &a, long pt, int code, const X &ex)
{
    const SelinvGeo &g = a.g;
    const long ww = (long)g.W * g.W, pw = (long)g.NPe * g.W;
    const double nan = NAN;
    ex.par([&](int tid, int nt) {
        fill_value(a.Skk ? a.Skk + pt * g.K * ww : nullptr, g.K * ww, nan, tid, nt);
        fill_value(a.Snk ? a.Snk + pt * (g.K - 1) * ww : nullptr, (g.K - 1) * ww, nan, tid, nt);
        fill_value(a.Spk ? a.Spk + pt * g.K * pw : nullptr, g.K * pw, nan, tid, nt);
        fill_value(a.Spp ? a.Spp + pt * g.NPe * g.NPe : nullptr, (long)g.NPe * g.NPe, nan, tid, nt);
        if (tid == 0) { a.logdet[pt] = nan; a.status[pt] = code; }
    });
}

// Cholesky of the n x n image S in place (lower triangle), the pivots kept in piv[n]; false at the first pivot that is <= 0 or NaN
template <class X> VA_HD bool selinv_chol(double *S, int pitch, int n, double *piv, double *ld, const X &ex)
{
    for (int j = 0; j < n; ++j) {
        const double p = S[j * pitch + j];            // (written before the last join; the same value in every thread)
        if (!(p > 0.0)) return false;
        const double c = sqrt(p);
        ex.par([&](int tid, int nt) { chol_scale(S, pitch, n, j, c, tid, nt); });
        ex.par([&](int tid, int nt) { chol_update(S, pitch, n, j, p, c, piv, ld, tid); });
    }
    return true;
}

// ---------------------------------------------------------------- one point
template <class X> VA_HD void selinv_point(const SelinvArgs &a, long pt, double *mem, const X &ex)
{
    const SelinvGeo &g = a.g;
    const int W = g.W, K = g.K, NPe = g.NPe, Wp = g.Wp, NPp = g.NPp;
    const long ww = (long)W * W, pw = (long)NPe * W;
    const double *Dk = a.Dk + pt * K * ww, *Bk = a.Bk + pt * (K - 1) * ww, *Pk = a.Pk + pt * K * pw, *Hpp = a.Hpp + pt * NPe * NPe;
    double *wsC = a.ws + (size_t)pt * g.ws_doubles, *wsE = wsC + K * ww, *wsF = wsE + (K - 1) * ww, *wsPiv = wsF + K * pw,
           *wsSnk = wsPiv + (long)K * W;
    double *ld = mem, *piv = mem + SELINV_HDR;
    double *big0 = piv + g.piv, *big1 = big0 + g.big, *big2 = big1 + g.big;
    double *brd0 = big2 + g.big + (g.snk_global ? 0 : g.big), *brd1 = brd0 + g.brd, *brd2 = brd1 + g.brd, *spp = brd2 + g.brd;
    double *snk = g.snk_global ? wsSnk : big2 + g.big;
    const int snp = g.snk_global ? W : Wp;

    // ---- forward
    double *S = big0, *E = big1, *Fa = brd0, *Fb = brd1;
    ex.par([&](int tid, int nt) {
        blk_load(S, Wp, Dk, W, W, tid, nt);
        blk_load(spp, NPp, Hpp, NPe, NPe, tid, nt);
        if (tid == 0) *ld = 0.0;
    });
    for (int k = 0; k < K; ++k) {
        // R = P_k - F_{k-1} E_{k-1}^T
        ex.par([&](int tid, int nt) {
            const double *P = Pk + k * pw;
            for (int e = tid; e < NPe * W; e += nt) {
                const int r = e / W, i = e - r * W;
                double v = P[e];
                if (k > 0)
                    for (int j = 0; j < W; ++j) v -= Fa[r * Wp + j] * E[i * Wp + j];
                Fb[r * Wp + i] = v;
            }
        });
        if (!selinv_chol(S, Wp, W, piv, ld, ex)) { selinv_fail(a, pt, k + 1, ex); return; }
        if (k < K - 1) ex.par([&](int tid, int nt) { blk_load(E, Wp, Bk + k * ww, W, W, tid, nt); });
        // E_k = B_k C^-T, F_k = R C^-T: a row per thread
        ex.par([&](int tid, int nt) {
            for (int r = tid; r < W + NPe; r += nt) {
                if (r < W) { if (k < K - 1) row_solve_ct(E + r * Wp, S, Wp, W); }
                else row_solve_ct(Fb + (r - W) * Wp, S, Wp, W);
            }
        });
        // the factor goes out; S_p -= F_k F_k^T
        ex.par([&](int tid, int nt) {
            blk_store(wsC + k * ww, S, Wp, W, W, tid, nt);
            if (k < K - 1) blk_store(wsE + k * ww, E, Wp, W, W, tid, nt);
            blk_store(wsF + k * pw, Fb, Wp, NPe, W, tid, nt);
            for (int e = tid; e < W; e += nt) wsPiv[(long)k * W + e] = piv[e];
            for (int e = tid; e < NPe * NPe; e += nt) {
                const int r = e / NPe, c = e - r * NPe;
                double v = 0.0;
                for (int j = 0; j < W; ++j) v += Fb[r * Wp + j] * Fb[c * Wp + j];
                spp[r * NPp + c] -= v;
            }
        });
        // S = D_{k+1} - E_k E_k^T (lower triangle)
        if (k < K - 1)
            ex.par([&](int tid, int nt) {
                const double *Dn = Dk + (k + 1) * ww;
                for (int e = tid; e < W * W; e += nt) {
                    const int i = e / W, l = e - i * W;
                    if (l > i) continue;
                    double v = 0.0;
                    for (int j = 0; j < W; ++j) v += E[i * Wp + j] * E[l * Wp + j];
                    S[i * Wp + l] = Dn[e] - v;
                }
            });
        double *t = Fa; Fa = Fb; Fb = t;
    }

    // ---- the parameters: C_p = chol(S_p), Sigma_pp = C_p^-T C_p^-1
    if (!selinv_chol(spp, NPp, NPe, piv, ld, ex)) { selinv_fail(a, pt, -1, ex); return; }
    ex.par([&](int tid, int nt) {
        blk_identity(big2, NPp, NPe, tid, nt);
        if (tid == 0) { a.logdet[pt] = *ld; a.status[pt] = 0; }
    });
    ex.par([&](int tid, int nt) { for (int r = tid; r < NPe; r += nt) row_inverse(big2 + r * NPp, spp, NPp, r); });
    ex.par([&](int tid, int nt) {
        for (int e = tid; e < NPe * NPe; e += nt) {
            const int r = e / NPe, c = e - r * NPe;
            const double v = lower_gram(big2, NPp, NPe, piv, r, c);
            spp[r * NPp + c] = v;
            if (a.Spp) a.Spp[pt * NPe * NPe + e] = v;
        }
    });

    // ---- backward
    double *Sn = big0, *Cb = big1, *Ci = big2, *Spn = brd0, *Gf = brd1, *Spk = brd2;
    for (int k = K - 1; k >= 0; --k) {
        const bool sub = k < K - 1;
        ex.par([&](int tid, int nt) {
            blk_load(Cb, Wp, wsC + k * ww, W, W, tid, nt);
            blk_identity(Ci, Wp, W, tid, nt);
            blk_load(Gf, Wp, wsF + k * pw, NPe, W, tid, nt);
            for (int e = tid; e < W; e += nt) piv[e] = wsPiv[(long)k * W + e];
        });
        ex.par([&](int tid, int nt) { for (int r = tid; r < W; r += nt) row_inverse(Ci + r * Wp, Cb, Wp, r); });
        if (sub) ex.par([&](int tid, int nt) { blk_load(Cb, Wp, wsE + k * ww, W, W, tid, nt); });
        // Ge = E_k C^-1 (in Cb), Gf = F_k C^-1: a row per thread
        ex.par([&](int tid, int nt) {
            for (int r = tid; r < W + NPe; r += nt) {
                if (r < W) { if (sub) row_times_lower(Cb + r * Wp, Ci, Wp, W); }
                else row_times_lower(Gf + (r - W) * Wp, Ci, Wp, W);
            }
        });
        const double *Ge = Cb;
        // Sigma_{k+1,k} and Sigma_{p,k}
        ex.par([&](int tid, int nt) {
            if (sub)
                for (int e = tid; e < W * W; e += nt) {
                    const int i = e / W, j = e - i * W;
                    double v = 0.0;
                    for (int l = 0; l < W; ++l) v += Sn[i * Wp + l] * Ge[l * Wp + j];
                    for (int p = 0; p < NPe; ++p) v += Spn[p * Wp + i] * Gf[p * Wp + j];
                    snk[i * snp + j] = -v;
                    if (a.Snk) a.Snk[(pt * (K - 1) + k) * ww + e] = -v;
                }
            for (int e = tid; e < NPe * W; e += nt) {
                const int r = e / W, j = e - r * W;
                double v = 0.0;
                if (sub)
                    for (int l = 0; l < W; ++l) v += Spn[r * Wp + l] * Ge[l * Wp + j];
                for (int p = 0; p < NPe; ++p) v += spp[r * NPp + p] * Gf[p * Wp + j];
                Spk[r * Wp + j] = -v;
                if (a.Spk) a.Spk[(pt * K + k) * pw + e] = -v;
            }
        });
        // Sigma_kk, over Sigma_{k+1,k+1} (not read in this par)
        ex.par([&](int tid, int nt) {
            for (int e = tid; e < W * W; e += nt) {
                const int i = e / W, j = e - i * W;
                double v = lower_gram(Ci, Wp, W, piv, i, j);
                if (sub)
                    for (int l = 0; l < W; ++l) v -= snk[l * snp + i] * Ge[l * Wp + j];
                for (int p = 0; p < NPe; ++p) v -= Spk[p * Wp + i] * Gf[p * Wp + j];
                Sn[i * Wp + j] = v;
                if (a.Skk) a.Skk[(pt * K + k) * ww + e] = v;
            }
        });
        double *t = Spn; Spn = Spk; Spk = t;
    }
}

// the same phases, thread by thread on the host (every pointer of `a` is host memory)
inline void selinv_host(const SelinvArgs &a)
{
    std::vector<double> mem(a.g.lds_doubles, 0.0);
    const SelinvHostExec ex{SELINV_THREADS};
    for (long pt = 0; pt < a.npts; ++pt) selinv_point(a, pt, mem.data(), ex);
}

// ---------------------------------------------------------------- blocks from the coloured products, and back to time rows
struct HblocksArgs {
    HblocksGeo h;
    const double *HV;                      // [npts][nvec][ld]
    double *Dk, *Bk, *Pk, *Hpp;            // as SelinvArgs
    int npts;
};
VA_HD long hblocks_per_point(const HblocksGeo &h)
{
    const long W = hblocks_W(h), K = hblocks_K(h);
    return (2 * K - 1) * W * W + K * h.NPe * W + (long)h.NPe * h.NPe;
}
VA_HD double hblocks_fetch(const double *hv, long src) { return src == HB_ZERO ? 0.0 : (src == HB_ONE ? 1.0 : hv[src]); }
// entry e of point pt's blocks, in the order D | B | P | H_pp
VA_HD void hblocks_one(const HblocksArgs &a, long pt, long e)
{
    const HblocksGeo &h = a.h;
    const long W = hblocks_W(h), K = hblocks_K(h), ww = W * W, pw = (long)h.NPe * W;
    const double *hv = a.HV + (size_t)pt * hblocks_nvec(h) * h.ld;
    if (e < K * ww) {
        const long k = e / ww, r = (e - k * ww) / W, c = e - k * ww - r * W;
        a.Dk[pt * K * ww + e] = hblocks_fetch(hv, hblocks_src(h, k * W + r, k * W + c));
        return;
    }
    e -= K * ww;
    if (e < (K - 1) * ww) {
        const long k = e / ww, r = (e - k * ww) / W, c = e - k * ww - r * W;
        a.Bk[pt * (K - 1) * ww + e] = hblocks_fetch(hv, hblocks_src(h, (k + 1) * W + r, k * W + c));
        return;
    }
    e -= (K - 1) * ww;
    if (e < K * pw) {
        const long k = e / pw, p = (e - k * pw) / W, c = e - k * pw - p * W;
        a.Pk[pt * K * pw + e] = hblocks_fetch(hv, hblocks_src_border(h, (int)p, k * W + c));
        return;
    }
    e -= K * pw;
    const int p = (int)(e / h.NPe), q = (int)(e - (long)p * h.NPe);
    a.Hpp[pt * h.NPe * h.NPe + e] = 0.5 * (hv[hblocks_src_pp(h, p, q)] + hv[hblocks_src_pp(h, q, p)]);
}
inline void hblocks_host(const HblocksArgs &a)
{
    const long per = hblocks_per_point(a.h);
    for (long pt = 0; pt < a.npts; ++pt)
        for (long e = 0; e < per; ++e) hblocks_one(a, pt, e);
}

// entry (c, i) of the coloured directions, the same for every point
VA_HD double hcolour_entry(const HblocksGeo &h, long c, long i)
{
    const long ND = (long)h.N * h.D, nc = 2 * h.hb + 1;
    if (c >= nc * h.D) return i == ND + (c - nc * h.D) ? 1.0 : 0.0;
    if (i >= ND) return 0.0;
    const long n = i / h.D;
    return (n % nc) * h.D + (i - n * h.D) == c ? 1.0 : 0.0;
}

struct UnpackArgs {
    HblocksGeo h;
    const double *Skk, *Spk;               // [npts][K][W][W], [npts][K][NPe][W]
    double *var_x, *cov_xx, *cov_px;       // [npts][N D], [npts][N][D][D] or NULL, [npts][NPe][N D] or NULL
    int npts;
};
VA_HD long unpack_per_point(const HblocksGeo &h) { return (long)h.N * h.D * (1 + h.D + h.NPe); }
// entry e of point pt's results, in the order var_x | cov_xx | cov_px
VA_HD void unpack_one(const UnpackArgs &a, long pt, long e)
{
    const HblocksGeo &h = a.h;
    const long D = h.D, ND = (long)h.N * D, W = hblocks_W(h), K = hblocks_K(h), ww = W * W;
    const double *Skk = a.Skk + pt * K * ww, *Spk = a.Spk + pt * K * h.NPe * W;
    if (e < ND) {
        const long k = e / W, r = e - k * W;
        a.var_x[pt * ND + e] = Skk[k * ww + r * W + r];
        return;
    }
    e -= ND;
    if (e < ND * D) {
        if (!a.cov_xx) return;
        const long i = e / D, b = e - i * D, k = i / W, r = i - k * W, c = (r / D) * D + b;      // the D x D block of i's own time row
        a.cov_xx[pt * ND * D + e] = Skk[k * ww + r * W + c];
        return;
    }
    e -= ND * D;
    if (!a.cov_px) return;
    const long p = e / ND, i = e - p * ND, k = i / W, r = i - k * W;
    a.cov_px[pt * h.NPe * ND + e] = Spk[(k * h.NPe + p) * W + r];
}

}  // namespace va

// ---------------------------------------------------------------- the kernels
#if defined(__HIPCC__)
#include "va_device.h"      // the LDS opt-in's sizes

namespace va {

__global__ __launch_bounds__(SELINV_THREADS) void k_selinv(const SelinvArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double selinv_mem[];
    selinv_point(a, (long)blockIdx.x, selinv_mem, SelinvDevExec());
}

__global__ __launch_bounds__(256) void k_hblocks(const HblocksArgs a)
{
    const long per = hblocks_per_point(a.h), tot = per * a.npts;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < tot; idx += (long)gridDim.x * 256) {
        const long pt = idx / per;
        hblocks_one(a, pt, idx - pt * per);
    }
}

// V [npts][nvec][ld]
__global__ __launch_bounds__(256) void k_hcolour(const HblocksGeo h, double *V, int npts)
{
    const long per = (long)hblocks_nvec(h) * h.ld, tot = per * npts;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < tot; idx += (long)gridDim.x * 256) {
        const long e = idx % per, c = e / h.ld;
        V[idx] = hcolour_entry(h, c, e - c * h.ld);
    }
}

__global__ __launch_bounds__(256) void k_laplace_unpack(const UnpackArgs a)
{
    const long per = unpack_per_point(a.h), tot = per * a.npts;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < tot; idx += (long)gridDim.x * 256) {
        const long pt = idx / per;
        unpack_one(a, pt, idx - pt * per);
    }
}

inline unsigned selinv_flat_grid(long tot)
{
    const long blocks = (tot + 255) / 256;
    return (unsigned)(blocks < 1 ? 1 : (blocks > 65535 ? 65535 : blocks));
}

inline hipError_t launch_selinv(const SelinvArgs &a, hipStream_t s)
{
    if (a.g.lds_bytes > LDS_DEFAULT_BYTES) {
        const hipError_t e = hipFuncSetAttribute((const void *)k_selinv, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_OPTIN_BYTES);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_selinv, dim3((unsigned)a.npts), dim3(SELINV_THREADS), a.g.lds_bytes, s, a);
    return hipGetLastError();
}
inline hipError_t launch_hblocks(const HblocksArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(k_hblocks, dim3(selinv_flat_grid(hblocks_per_point(a.h) * a.npts)), dim3(256), 0, s, a);
    return hipGetLastError();
}
inline hipError_t launch_hcolour(const HblocksGeo &h, double *V, int npts, hipStream_t s)
{
    hipLaunchKernelGGL(k_hcolour, dim3(selinv_flat_grid((long)hblocks_nvec(h) * h.ld * npts)), dim3(256), 0, s, h, V, npts);
    return hipGetLastError();
}
inline hipError_t launch_laplace_unpack(const UnpackArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(k_laplace_unpack, dim3(selinv_flat_grid(unpack_per_point(a.h) * a.npts)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace va
#endif
