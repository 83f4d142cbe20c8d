// va_hmc.hip -- the sampler's kernels: thin executors over the phases of va_hmc.h on the geometry of va_hmc_geo.h.
// Memory-bound element-wise passes (begin: 2 vectors read, 4 written; mid: 3 read, 2 written; the box sampler's one vector
// more each way and three shared tables); a translation unit of its own, so the evaluation kernels are not rebuilt with it.
#include "va_hmc.h"
#include "va_hmc_box.h"

namespace va {

// the lanes' sums by a binary tree over the lane index, in LDS (hmc_tree_host is its transcription); the total in red[0]
__device__ __forceinline__ void hmc_tree(double *red, int tid, double v)
{
#pragma clang fp contract(off)
    red[tid] = v;
    __syncthreads();
    for (int s = HMC_THREADS / 2; s >= 1; s >>= 1) {
        if (tid < s) red[tid] = red[tid] + red[tid + s];
        __syncthreads();
    }
}

template <int PHASE>
__global__ __launch_bounds__(HMC_THREADS) void k_hmc(const HmcArgs a)
{
    __shared__ double red[HMC_THREADS];
    __shared__ double dec[2];
    __shared__ int acc_s;
    const long wg = (long)blockIdx.x;
    const int tid = (int)threadIdx.x;
    if (wg >= a.geo.grid) return;
    if (PHASE == HMC_BEGIN || PHASE == HMC_END) {
        const double v = PHASE == HMC_BEGIN ? hmc_begin_lane(a, wg, tid) : hmc_end_lane(a, wg, tid);
        hmc_tree(red, tid, v);
        if (tid == 0) a.part[(PHASE == HMC_END ? (size_t)a.geo.grid : 0) + wg] = red[0];
    } else if (PHASE == HMC_MID) {
        hmc_mid_lane(a, wg, tid);
    } else {
        if (tid == 0) {
            double dH, A_new;
            acc_s = hmc_decide(a, (int)(wg / a.geo.nwg), dH, A_new) ? 1 : 0;
            dec[0] = dH; dec[1] = A_new;
        }
        __syncthreads();
        hmc_commit_lane(a, wg, tid, acc_s != 0, dec[0], dec[1]);
    }
}

hipError_t launch_hmc(const HmcArgs &a, int phase, hipStream_t s)
{
    if (a.geo.grid < 1 || a.geo.grid > 2147483647L || a.geo.threads != HMC_THREADS) return hipErrorInvalidValue;
    const dim3 grid((unsigned)a.geo.grid), block(HMC_THREADS);
    switch (phase) {
    case HMC_BEGIN: hipLaunchKernelGGL(k_hmc<HMC_BEGIN>, grid, block, 0, s, a); break;
    case HMC_MID: hipLaunchKernelGGL(k_hmc<HMC_MID>, grid, block, 0, s, a); break;
    case HMC_END: hipLaunchKernelGGL(k_hmc<HMC_END>, grid, block, 0, s, a); break;
    case HMC_COMMIT: hipLaunchKernelGGL(k_hmc<HMC_COMMIT>, grid, block, 0, s, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------- the box sampler (va_hmc_box.h): the same executors over
// its phases, a second reduction buffer for the log-Jacobian share
template <int PHASE>
__global__ __launch_bounds__(HMC_THREADS) void k_hmc_box(const HmcBoxArgs a)
{
    __shared__ double red[HMC_THREADS];
    __shared__ double redl[HMC_THREADS];
    __shared__ double dec[2];
    __shared__ int acc_s;
    const long wg = (long)blockIdx.x;
    const int tid = (int)threadIdx.x;
    if (wg >= a.h.geo.grid) return;
    if (PHASE == HMC_BEGIN || PHASE == HMC_END) {
        double ls;
        const double v = PHASE == HMC_BEGIN ? hmc_box_begin_lane(a, wg, tid, &ls) : hmc_box_end_lane(a, wg, tid, &ls);
        hmc_tree(red, tid, v);
        hmc_tree(redl, tid, ls);
        if (tid == 0) {
            const size_t o = (PHASE == HMC_END ? (size_t)a.h.geo.grid : 0) + wg;
            a.h.part[o] = red[0]; a.lpart[o] = redl[0];
        }
    } else if (PHASE == HMC_MID) {
        hmc_box_mid_lane(a, wg, tid);
    } else {
        if (tid == 0) {
            double dH, A_new;
            acc_s = hmc_box_decide(a, (int)(wg / a.h.geo.nwg), dH, A_new) ? 1 : 0;
            dec[0] = dH; dec[1] = A_new;
        }
        __syncthreads();
        hmc_box_commit_lane(a, wg, tid, acc_s != 0, dec[0], dec[1]);
    }
}

hipError_t launch_hmc_box(const HmcBoxArgs &a, int phase, hipStream_t s)
{
    if (a.h.geo.grid < 1 || a.h.geo.grid > 2147483647L || a.h.geo.threads != HMC_THREADS) return hipErrorInvalidValue;
    const dim3 grid((unsigned)a.h.geo.grid), block(HMC_THREADS);
    switch (phase) {
    case HMC_BEGIN: hipLaunchKernelGGL(k_hmc_box<HMC_BEGIN>, grid, block, 0, s, a); break;
    case HMC_MID: hipLaunchKernelGGL(k_hmc_box<HMC_MID>, grid, block, 0, s, a); break;
    case HMC_END: hipLaunchKernelGGL(k_hmc_box<HMC_END>, grid, block, 0, s, a); break;
    case HMC_COMMIT: hipLaunchKernelGGL(k_hmc_box<HMC_COMMIT>, grid, block, 0, s, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void k_hmc_box_map(long n, const int32_t *kind, const double *lo, const double *hi, const double *z,
                                                     double *x, double *dx, double *dlj, double *lj)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double xv, dv, dl, l;
    hmc_box_map(kind[i], lo[i], hi[i], z[i], &xv, &dv, &dl, &l);
    x[i] = xv; dx[i] = dv; dlj[i] = dl; lj[i] = l;
}

hipError_t launch_hmc_box_map(long n, const int32_t *kind, const double *lo, const double *hi, const double *z, double *x, double *dx,
                              double *dlj, double *lj, hipStream_t s)
{
    if (n < 1 || (n + 255) / 256 > 2147483647L) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_hmc_box_map, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, kind, lo, hi, z, x, dx, dlj, lj);
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void k_hmc_noise(uint32_t k0, uint32_t k1, uint32_t chain, uint32_t it, long n, uint32_t *words,
                                                   double *normals, double *uniforms)
{
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i > n) return;
    uint32_t w[4];
    if (i < n) {
        hmc_philox(k0, k1, chain, it, (uint32_t)i, 0u, w);
        if (normals) normals[i] = hmc_box_muller(w[0], w[1]);
    } else {
        hmc_philox(k0, k1, chain, it, 0u, 1u, w);
        if (uniforms) { uniforms[0] = hmc_u01(w[0]); uniforms[1] = hmc_u01(w[1]); }
    }
    if (words)
        for (int k = 0; k < 4; ++k) words[4 * i + k] = w[k];
}

hipError_t launch_hmc_noise(uint32_t k0, uint32_t k1, uint32_t chain, uint32_t it, long n, uint32_t *words, double *normals,
                            double *uniforms, hipStream_t s)
{
    if (n < 0 || (n + 256) / 256 > 2147483647L) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_hmc_noise, dim3((unsigned)((n + 256) / 256)), dim3(256), 0, s, k0, k1, chain, it, n, words, normals, uniforms);
    return hipGetLastError();
}

}  // namespace va
