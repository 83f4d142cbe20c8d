// va_hvp.h -- Hessian-vector products of the action: (d^2 A / d[X | p_est]^2) . v for a batch of points and directions.
//
// The gradient of va_core.h is a chain of LINEAR phases around the model function:
//     q = c w r(x, f(x, p))          tile_q        (r: the discretisation's residual, linear in x and f)
//     (direct, s) = lin(q)           disc_direct_s
//     g_m = direct_m + J(x_m)^T s_m  tile_g        g_p = sum_m (df/dp)^T s_m
// Differentiated along v = [v_x | v_p] the same phases run on tangent inputs, and one new term per row appears:
//     fdot_m = J(x_m) v_m + (df/dp) v_p                                    RHS::jvp      (tile_fdot)
//     qdot   = tile_q on (v, fdot)   sdot, directdot = disc_direct_s(qdot)
//     (Hv)_m = directdot_m + J(x_m)^T sdot_m + K_m + 2 cme w v_m [observed entries]       (tile_hv)
//     K_m,j  = sum_i s_m,i d/dx_j (fdot_m,i)                                RHS::vjp2
//     (Hv)_p = sum_m (df/dp)^T sdot_m + sum_m sum_i s_m,i d/dp (fdot_m,i)   RHS::pgrad, RHS::pgrad2
// Without K and pgrad2 this is the Gauss-Newton Hessian 2 J_r^T W J_r of the residual list.  The reference has no
// analytic second derivatives; it exposes adolc.hessian of a taped action (varanneal/_autodiffmin.py).
//
// Decomposition (va_hvp_geo.h): one workgroup = one (point, direction, tile of T time rows).  It stages the rows of x and of
// v with the halos of Halo<DISC>, and runs tile_f / tile_q / tile_s of va_core.h on two TileCtx: one on the images of x,
// one on the images of v.  The parameter rows are per-tile partial sums, added in tile order by k_hvp_finish: no
// floating-point atomics, the same bits whenever the geometry is the same.  (Simpson-Hermite tiles of an odd number of rows
// stage two more rows behind, form q for one more, and keep a zero row in front: va_hvp_geo.h hvp_extra_rows.)  hvp_host drives the same phases thread by thread
// on the CPU (tests/cpu_emul/hvp_check.cpp).
#pragma once
#include <vector>

#include "va_core.h"
#include "va_hvp_geo.h"

namespace va {

struct HvpArgs {
    Dims dm;                 // D, N, ND = N D, NP, NPest, T, ntiles, nskip, L, dt, cme, rm, rf0; tdp = 0, NPt = NP
    ProblemPtrs pp;          // lmap, rm_arr, rf0_arr, Pidx, tmodel, stim of the handle; Pfull: the call's own [npts][NP];
                             // rf0_full, rm_full, lo, hi: NULL (refused / ignored by va_hess_vec)
    const double *X;         // [npts][ld]         [X | p_est]
    const double *V;         // [npts][nvec][ld]   directions, the same packing
    double *HV;              // [npts][nvec][ld]
    double *part;            // [npts][nvec][ntiles][NP]: the tiles' shares of the parameter rows
    long ld;
    int npts, nvec;
    int gn;                  // 1: Gauss-Newton (no K, no pgrad2)
    int rm_ld;               // row pitch of pp.rm_arr
    double c;                // 2 rf_scale cfe
};

struct HvpWork { long pt, pd; int tile; };      // point, point x direction, tile
VA_HD HvpWork hvp_work(const HvpArgs &a, long wg)
{
    HvpWork w;
    w.pd = wg / a.dm.ntiles; w.tile = (int)(wg - w.pd * a.dm.ntiles);
    w.pt = w.pd / a.nvec;
    return w;
}

template <class RHS> struct HvpNP { static constexpr int value = RHS::NP > 0 ? RHS::NP : 1; };

// the two contexts of a workgroup and the full-length parameter tangent qp (zero where a parameter is not estimated)
template <class RHS, int DISC>
VA_HD void hvp_ctx(const HvpArgs &a, const HvpWork &w, double *mem, TileCtx &cx, TileCtx &cv, double *qp)
{
    const Dims &dm = a.dm;
    // an image: `front` rows held at zero (hvp_front_rows), then the R staged rows the phases see
    const int front = hvp_front_rows(DISC, dm.T), R = dm.T + hvp_halo(DISC, dm.T) - front, RD = (R + front) * dm.D;
    mem += front * dm.D;
    cx.n0 = cv.n0 = w.tile * dm.T; cx.R = cv.R = R; cx.use_d = cv.use_d = 0;
    cx.stp = cv.stp = 0.0; cx.c = cv.c = a.c;
    cx.xs = mem; cx.fs = mem + RD; cx.qs = mem + 2 * RD;
    cv.xs = mem + 3 * RD; cv.fs = mem + 4 * RD; cv.qs = mem + 5 * RD;
    cx.xg = a.X + (size_t)w.pt * a.ld; cv.xg = a.V + (size_t)w.pd * a.ld;
    cx.dg = cv.dg = nullptr; cx.gtg = cv.gtg = a.HV + (size_t)w.pd * a.ld;
    cx.tmodel = cv.tmodel = a.pp.tmodel; cx.stim = cv.stim = a.pp.stim; cx.nstim = cv.nstim = a.pp.nstim;
    cx.ps = cv.ps = nullptr;
    tile_params<RHS>(dm, a.pp, (int)w.pt, cx);
#pragma unroll
    for (int k = 0; k < HvpNP<RHS>::value; ++k) qp[k] = 0.0;
    for (int e = 0; e < dm.NPest; ++e) {
        const double v = cv.xg[dm.ND + e];
        const int dst = a.pp.Pidx[e];
#pragma unroll
        for (int k = 0; k < HvpNP<RHS>::value; ++k) qp[k] = (dst == k) ? v : qp[k];      // (no runtime-indexed array)
    }
}

// the front rows of the images tile_q reads one row back from (x, f, v, fdot), zeroed once per workgroup
template <int DISC>
VA_HD void hvp_zero_front(const Dims &dm, const TileCtx &cx, const TileCtx &cv, int tid, int nt)
{
    const int tot = hvp_front_rows(DISC, dm.T) * dm.D;
    for (int e = tid; e < tot; e += nt) { cx.xs[e - tot] = 0.0; cx.fs[e - tot] = 0.0; cv.xs[e - tot] = 0.0; cv.fs[e - tot] = 0.0; }
}

// what tile_q is handed: q for the rows [n0 - HL, n0 + T), and one more row where the tile staged extra rows
template <int DISC> VA_HD Dims hvp_q_dims(const Dims &dm)
{
    Dims dq = dm;
    if (hvp_back_rows(DISC, dm.T)) dq.T = dm.T + 1;
    return dq;
}

// tangent of phase 2: fdot = J(x) v + (df/dp) v_p at every staged row that exists (into the tangent context's fs)
template <class RHS, int DISC>
VA_HD void tile_fdot(const Dims &dm, const TileCtx &cx, TileCtx &cv, const double *qp, int tid, int nt)
{
    const int D = dm.D, tot = cx.R * D;
    int lr = tid / D, i = tid - lr * D;
    const int dlr = nt / D, di = nt - dlr * D;
    for (int e = tid; e < tot; e += nt) {
        const int row = cx.n0 - Halo<DISC>::HL + lr;
        cv.fs[e] = (row >= 0 && row < dm.N)
                       ? RHS::jvp(cx.xs + lr * D, cv.xs + lr * D, qp, i, D, cx.p, cx.tmodel ? cx.tmodel[row] : 0.0,
                                  cx.stim + (size_t)row * cx.nstim)
                       : 0.0;
        lr += dlr; i += di;
        if (i >= D) { i -= D; ++lr; }
    }
}

// the owned rows of H v, and the thread's share of the parameter rows (accp[RHS::NP]).  cx.fs holds s, cv.fs holds sdot.
template <class RHS, int DISC>
VA_HD void tile_hv(const HvpArgs &a, const TileCtx &cx, const TileCtx &cv, const double *qp, double *accp, int tid, int nt)
{
    constexpr int HL = Halo<DISC>::HL;
    const Dims &dm = a.dm;
    const int D = dm.D, tot = dm.T * D;
    int lt = tid / D, j = tid - lt * D;
    const int dlr = nt / D, dj = nt - dlr * D;
    for (int e = tid; e < tot; e += nt) {
        const int lr = lt + HL, m = cx.n0 + lt;
        if (m < dm.N) {
            double direct, sdummy;
            disc_direct_s<DISC>(cv.qs + lr * D + j, D, m, dm.dt, direct, sdummy);
            const double *xr = cx.xs + lr * D, *sr = cx.fs + lr * D, *vr = cv.xs + lr * D, *sdr = cv.fs + lr * D;
            const double tm = cx.tmodel ? cx.tmodel[m] : 0.0;
            const double *st = cx.stim + (size_t)m * cx.nstim;
            double hv = direct + RHS::vjp(xr, sdr, j, D, cx.p, tm, st);
            RHS::pgrad(xr, sdr, j, D, cx.p, tm, st, accp);
            if (!a.gn) {
                hv += RHS::vjp2(xr, sr, vr, qp, j, D, cx.p, tm, st);
                RHS::pgrad2(xr, sr, vr, qp, j, D, cx.p, tm, st, accp);
            }
            const int l = a.pp.lmap[j];
            if (l >= 0 && (m % dm.nskip) == 0) {
                const double w = a.pp.rm_arr ? a.pp.rm_arr[(size_t)(m / dm.nskip) * a.rm_ld + l] : dm.rm;
                hv += 2.0 * dm.cme * w * vr[j];
            }
            cx.gtg[(long)m * D + j] = hv;
        }
        lt += dlr; j += dj;
        if (j >= D) { j -= D; ++lt; }
    }
}

// finishing pass: parameter row e of (point, direction) pd = the tiles' shares added in tile order
VA_HD void hvp_finish_one(const HvpArgs &a, long pd, int e)
{
    const int NP = a.dm.NP, k = a.pp.Pidx[e];
    const double *row = a.part + (size_t)pd * a.dm.ntiles * NP + k;
    double tot = 0.0;
    for (int t = 0; t < a.dm.ntiles; ++t) tot += row[(size_t)t * NP];
    a.HV[(size_t)pd * a.ld + a.dm.ND + e] = tot;
}

// ---------------------------------------------------------------- the same phases, thread by thread on the host
// (every pointer of `a` is host memory)
template <class RHS, int DISC>
inline void hvp_host_disc(const HvpArgs &a)
{
    const Dims &dm = a.dm;
    const int nt = HVP_THREADS;
    constexpr int NPA = HvpNP<RHS>::value;
    std::vector<double> mem(hvp_lds_doubles(dm.T, dm.D, DISC, dm.NP), 0.0);
    const long nwork = (long)a.npts * a.nvec * dm.ntiles;
    const Dims dq = hvp_q_dims<DISC>(dm);
    for (long wg = 0; wg < nwork; ++wg) {
        const HvpWork w = hvp_work(a, wg);
        TileCtx cx, cv;
        double qp[NPA];
        hvp_ctx<RHS, DISC>(a, w, mem.data(), cx, cv, qp);
        ThreadAccT<2> none;
        none.clear();
        for (int tid = 0; tid < nt; ++tid) { hvp_zero_front<DISC>(dm, cx, cv, tid, nt); tile_load<DISC>(dm, a.pp, cx, tid, nt); tile_load<DISC>(dm, a.pp, cv, tid, nt); }
        for (int tid = 0; tid < nt; ++tid) { tile_f<RHS, DISC>(dm, cx, tid, nt); tile_fdot<RHS, DISC>(dm, cx, cv, qp, tid, nt); }
        for (int tid = 0; tid < nt; ++tid) { tile_q<DISC>(dq, a.pp, cx, none, tid, nt); tile_q<DISC>(dq, a.pp, cv, none, tid, nt); }
        for (int tid = 0; tid < nt; ++tid) { tile_s<DISC>(dm, cx, tid, nt); tile_s<DISC>(dm, cv, tid, nt); }
        double tot[NPA];
        for (int k = 0; k < NPA; ++k) tot[k] = 0.0;
        for (int tid = 0; tid < nt; ++tid) {
            double accp[NPA];
            for (int k = 0; k < NPA; ++k) accp[k] = 0.0;
            tile_hv<RHS, DISC>(a, cx, cv, qp, accp, tid, nt);
            for (int k = 0; k < NPA; ++k) tot[k] += accp[k];
        }
        for (int k = 0; k < dm.NP; ++k) a.part[((size_t)w.pd * dm.ntiles + w.tile) * dm.NP + k] = tot[k];
    }
    for (long pd = 0; pd < (long)a.npts * a.nvec; ++pd)
        for (int e = 0; e < dm.NPest; ++e) hvp_finish_one(a, pd, e);
}

template <class RHS>
inline void hvp_host(const HvpArgs &a)
{
    switch (a.dm.disc) {
    case DISC_EULER: hvp_host_disc<RHS, DISC_EULER>(a); break;
    case DISC_TRAPEZOID: hvp_host_disc<RHS, DISC_TRAPEZOID>(a); break;
    case DISC_SH: hvp_host_disc<RHS, DISC_SH>(a); break;
    default: hvp_host_disc<RHS, DISC_FWDMAP>(a); break;
    }
}

}  // namespace va

// ---------------------------------------------------------------- the kernels
#if defined(__HIPCC__)
#include "va_eval_flat.h"      // wave_sum, with_disc, the LDS opt-in's sizes

namespace va {

template <class RHS, int DISC>
__global__ __launch_bounds__(HVP_THREADS) void k_hvp(const HvpArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double hvp_mem[];
    constexpr int NPA = HvpNP<RHS>::value;
    const Dims &dm = a.dm;
    const HvpWork w = hvp_work(a, (long)blockIdx.x);
    const int tid = threadIdx.x, nt = HVP_THREADS;
    TileCtx cx, cv;
    double qp[NPA], accp[NPA];
    hvp_ctx<RHS, DISC>(a, w, hvp_mem, cx, cv, qp);
    ThreadAccT<2> none;
    none.clear();
#pragma unroll
    for (int k = 0; k < NPA; ++k) accp[k] = 0.0;

    hvp_zero_front<DISC>(dm, cx, cv, tid, nt);
    tile_load<DISC>(dm, a.pp, cx, tid, nt);
    tile_load<DISC>(dm, a.pp, cv, tid, nt);
    __syncthreads();
    tile_f<RHS, DISC>(dm, cx, tid, nt);
    tile_fdot<RHS, DISC>(dm, cx, cv, qp, tid, nt);
    __syncthreads();
    {
        const Dims dq = hvp_q_dims<DISC>(dm);
        tile_q<DISC>(dq, a.pp, cx, none, tid, nt);
        tile_q<DISC>(dq, a.pp, cv, none, tid, nt);
    }
    __syncthreads();
    tile_s<DISC>(dm, cx, tid, nt);
    tile_s<DISC>(dm, cv, tid, nt);
    __syncthreads();
    tile_hv<RHS, DISC>(a, cx, cv, qp, accp, tid, nt);

    if (RHS::NP == 0) return;
    // the workgroup's share of the parameter rows: wave sums, then the four waves in order
    double *red = hvp_mem + 6 * (size_t)(dm.T + hvp_halo(DISC, dm.T)) * dm.D;
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int k = 0; k < NPA; ++k) {
        const double v = wave_sum(accp[k]);
        if (lane == 0) red[wave * NPA + k] = v;
    }
    __syncthreads();
    if (tid < RHS::NP) {
        double v = red[tid];
        for (int ww = 1; ww < HVP_THREADS / 64; ++ww) v += red[ww * NPA + tid];
        a.part[((size_t)w.pd * dm.ntiles + w.tile) * RHS::NP + tid] = v;
    }
}

template <class RHS>
__global__ __launch_bounds__(256) void k_hvp_finish(const HvpArgs a)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x, n = (long)a.npts * a.nvec * a.dm.NPest;
    if (idx >= n) return;
    const long pd = idx / a.dm.NPest;
    hvp_finish_one(a, pd, (int)(idx - pd * a.dm.NPest));
}

// prepare (the opt-in to the large LDS, once per process and device is enough but it is cheap: every call) and launch
template <class RHS>
inline hipError_t launch_hvp(const HvpArgs &a, size_t lds_bytes, hipStream_t s)
{
    static_assert(RHS::NP <= HVP_THREADS, "one thread per parameter writes the workgroup's share");
    if (a.dm.NP != RHS::NP) return hipErrorInvalidValue;
    hipError_t err = hipSuccess;
    const long grid = (long)a.npts * a.nvec * a.dm.ntiles;
    with_disc(a.dm.disc, [&](auto disc) {
        auto kern = k_hvp<RHS, decltype(disc)::value>;
        if (lds_bytes > LDS_DEFAULT_BYTES)
            err = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_OPTIN_BYTES);
        if (err == hipSuccess) hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(HVP_THREADS), lds_bytes, s, a);
    });
    if (err != hipSuccess) return err;
    if ((err = hipGetLastError()) != hipSuccess) return err;
    const long nfin = (long)a.npts * a.nvec * a.dm.NPest;
    if (nfin > 0) hipLaunchKernelGGL(k_hvp_finish<RHS>, dim3((unsigned)((nfin + 255) / 256)), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace va
#endif
