// va_hmc_geo.h -- launch geometry and argument checks of the Hamiltonian Monte Carlo sampler (va_hmc.h).  Plain C++: the
// host (va_capi.hip), the kernels and a CPU test (tests/cpu_emul/hmc_check.cpp) call the same functions.
//
// Every element-wise kernel of the sampler runs on ONE geometry: a chain's n_var variables are cut into chunks of
// HMC_CHUNK consecutive elements, one workgroup of HMC_THREADS lanes per chunk, lane t of chunk w taking the elements
// w * HMC_CHUNK + t + e * HMC_THREADS, e = 0 .. HMC_EPT - 1 (coalesced).  Workgroup index = chain * nwg + chunk.  The
// energy sums follow the same cut: a lane adds its elements in the order of e, the lanes are added by a binary tree over
// the lane index, the chunks of a chain in chunk order -- a fixed order, whatever the hardware does.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>

namespace va {

constexpr int HMC_THREADS = 256;
constexpr int HMC_EPT = 4;                              // elements per lane
constexpr int HMC_CHUNK = HMC_THREADS * HMC_EPT;        // elements per workgroup

struct HmcGeo {
    int threads;          // HMC_THREADS
    long nwg;             // workgroups (chunks) per chain: ceil(n_var / HMC_CHUNK); the last one may be ragged
    long grid;            // B * nwg
};

// false (`why`, nwhy bytes, says why: it stays with the host, the geometry goes to the kernels by value): nothing to do, or
// a grid past what one launch takes
inline bool plan_hmc(long n_var, long B, HmcGeo &g, char *why, size_t nwhy)
{
    g.threads = HMC_THREADS; g.nwg = 0; g.grid = 0;
    if (nwhy) why[0] = 0;
    if (n_var < 1 || B < 1) { snprintf(why, nwhy, "n_var=%ld and B=%ld must be at least 1", n_var, B); return false; }
    g.nwg = (n_var + HMC_CHUNK - 1) / HMC_CHUNK;
    if (g.nwg > 2147483647L / B) { snprintf(why, nwhy, "%ld chains x %ld workgroups do not fit one grid", B, g.nwg); return false; }
    g.grid = B * g.nwg;
    return true;
}

// the element lane `tid` of chunk `w` takes as its e-th, or -1 past the chain's end (constexpr: host and device call it)
constexpr long hmc_element(long n_var, long w, int tid, int e)
{
    return w * HMC_CHUNK + tid + (long)e * HMC_THREADS < n_var ? w * HMC_CHUNK + tid + (long)e * HMC_THREADS : -1;
}

// What va_hmc rejects with VA_EINVAL before it touches the device; 0, or 1 with the reason in `why`.
// minv: NULL, or minv_n = n_var (shared) or B * n_var values; keep_idx: n_keep indices into [0, n_var)
inline int hmc_check_args(long n_var, long B, int n_iter, int n_leap, int thin, const double *eps, double jitter, const double *minv,
                          long minv_n, const int64_t *keep_idx, long n_keep, char *why, size_t nwhy)
{
    if (n_iter < 1 || n_leap < 1 || thin < 1) {
        snprintf(why, nwhy, "n_iter, n_leap and thin must be at least 1 (n_iter=%d n_leap=%d thin=%d)", n_iter, n_leap, thin);
        return 1;
    }
    if (!eps) { snprintf(why, nwhy, "eps is NULL"); return 1; }
    for (long b = 0; b < B; ++b)
        if (!(eps[b] > 0.0) || !std::isfinite(eps[b])) { snprintf(why, nwhy, "eps[%ld] = %g is not positive and finite", b, eps[b]); return 1; }
    if (!(jitter >= 0.0 && jitter < 1.0)) { snprintf(why, nwhy, "jitter = %g outside [0, 1)", jitter); return 1; }
    if (minv) {
        if (minv_n != n_var && minv_n != B * n_var) {
            snprintf(why, nwhy, "minv holds %ld values: n_var = %ld (shared) or B * n_var = %ld", minv_n, n_var, B * n_var);
            return 1;
        }
        for (long i = 0; i < minv_n; ++i)
            if (!(minv[i] > 0.0) || !std::isfinite(minv[i])) { snprintf(why, nwhy, "minv[%ld] = %g is not positive and finite", i, minv[i]); return 1; }
    }
    if (n_keep < 0 || (n_keep > 0 && !keep_idx)) { snprintf(why, nwhy, "keep_idx is NULL or n_keep_idx negative"); return 1; }
    for (long k = 0; k < n_keep; ++k)
        if (keep_idx[k] < 0 || keep_idx[k] >= n_var) { snprintf(why, nwhy, "keep_idx[%ld] = %lld outside [0, n_var = %ld)", k, (long long)keep_idx[k], n_var); return 1; }
    return 0;
}

// ---------------------------------------------------------------- the box sampler's own checks (va_hmc_box.h)
// kind[i] of every entry from its bounds (-/+HUGE_VAL: none): 0 free, 1 lower only, 2 upper only, 3 both.  Returns the
// number of bounded entries (0: `why` says that nothing is bounded), or -1 with the reason in `why` (a lower bound that is
// not below its upper bound, or a NaN).
inline long hmc_box_kinds(long n_var, const double *lo, const double *hi, int32_t *kind, char *why, size_t nwhy)
{
    long nb = 0;
    for (long i = 0; i < n_var; ++i) {
        if (!(lo[i] < hi[i])) { snprintf(why, nwhy, "lower[%ld] = %g >= upper[%ld] = %g (or NaN)", i, lo[i], i, hi[i]); return -1; }
        kind[i] = (lo[i] > -HUGE_VAL ? 1 : 0) + (hi[i] < HUGE_VAL ? 2 : 0);
        if (kind[i]) ++nb;
    }
    if (nb == 0) snprintf(why, nwhy, "no bounds: every entry of lower / upper is infinite (va_hmc samples unbounded problems)");
    return nb;
}

// a start X [B][ld] must lie strictly inside its box (T^-1 is infinite on a bound); 0, or 1 with the entry in `why`
inline int hmc_box_check_start(long n_var, long B, long ld, const double *X, const double *lo, const double *hi, char *why, size_t nwhy)
{
    for (long b = 0; b < B; ++b)
        for (long i = 0; i < n_var; ++i) {
            const double v = X[b * ld + i];
            if (!(v > lo[i] && v < hi[i]) || !std::isfinite(v)) {
                snprintf(why, nwhy, "start XP[%ld][%ld] = %.17g is not strictly inside its box (%g, %g)", b, i, v, lo[i], hi[i]);
                return 1;
            }
        }
    return 0;
}

// a start given in z must be finite; 0, or 1 with the entry in `why`
inline int hmc_box_check_z(long n_var, long B, long ld, const double *Z, char *why, size_t nwhy)
{
    for (long b = 0; b < B; ++b)
        for (long i = 0; i < n_var; ++i)
            if (!std::isfinite(Z[b * ld + i])) { snprintf(why, nwhy, "Z0[%ld][%ld] = %g is not finite", b, i, Z[b * ld + i]); return 1; }
    return 0;
}

}  // namespace va
