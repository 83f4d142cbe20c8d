// va_enkf_geo.h -- launch geometry, LDS layout and argument checks of the ensemble Kalman filter kernel k_enkf (va_enkf.h) and
// the chunking of va_enkf's device workspace, as plain host C++: shared by the launcher, by the host emulation of the
// kernel (enkf_host) and by the CPU check (tests/cpu_emul/enkf_check.cpp, tests/test_enkf_cpu.py).
//
// A workgroup carries ONE point, always: its M members are the SLOTS of va_lyap_geo.h, D columns each at pitch D made odd,
// because the analysis walks a column across the members as k_lyap's QR walks one across the tangents.  One point to a
// workgroup even where several would fit a wave: a point's bits then cannot depend on what shares its launch.  The
// workgroup's elements (member, column) are numbered slot-major, element q = m D + i, and lane tid owns the elements tid,
// tid + threads, ..., E of them.
//   M D <= 64      one wave, no workgroup barrier
//   wider          min(256, elements rounded up to 64) threads, E <= 8 elements per lane: M D <= 2048, which is 102 members
//                  at D = 20 and 32 at D = 64
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdio.h>

#include "va_core.h"

namespace va {

constexpr int ENKF_MAX_E = 8;
constexpr int ENKF_MAX_THREADS = 256;
constexpr int ENKF_MAX_ELEMS = ENKF_MAX_THREADS * ENKF_MAX_E;      // M D of one point
constexpr size_t ENKF_LDS_LIMIT = 64 * 1024;
constexpr size_t ENKF_WORKSPACE_BYTES = (size_t)1 << 30;           // the device buffers of one chunk of points stay under this

struct EnkfGeo {
    int threads = 0;        // per workgroup: 64 (one wave), or min(256, elements rounded up to 64)
    int E = 0;              // elements per lane
    int wave = 0;           // 1: one wave per workgroup, ordered by the wave's own LDS order; 0: workgroup barriers
    int pitch = 0;          // doubles from one member's slot of an image to the next: D | 1
    size_t lds_bytes = 0;   // enkf_lds_doubles
    long grid = 0;          // workgroups: T
    const char *why = "";   // the refusal, when plan_enkf returns false
};

VA_HD int enkf_pitch(int D) { return D | 1; }

// images [2][M][pitch], parameters [M][NP], stimulus [2][nstim], the tables of the D + NQ augmented variables (mean,
// standard deviation, gain) [3][D + NQ], and hbar, y - hbar, alpha, status
inline size_t enkf_lds_doubles(int M, int D, int NP, int NQ, int nstim)
{
    return 2 * (size_t)M * enkf_pitch(D) + (size_t)M * NP + 2 * (size_t)nstim + 3 * (size_t)(D + NQ) + 4;
}

inline bool plan_enkf(int D, long T, int M, int NP, int NQ, int nstim, EnkfGeo &g)
{
    g = EnkfGeo();
    if (D < 1 || T < 1 || NP < 0 || NQ < 0 || NQ > NP || nstim < 0) { g.why = "bad sizes"; return false; }
    if (M < 2) { g.why = "an ensemble has at least 2 members (the sample variance divides by M - 1)"; return false; }
    if ((long)M * D > ENKF_MAX_ELEMS) {
        g.why = "M D is more than 2048: a workgroup of 256 threads x 8 elements per lane holds all members of a point";
        return false;
    }
    const int elems = M * D;
    g.pitch = enkf_pitch(D);
    if (elems <= 64) { g.wave = 1; g.threads = 64; g.E = 1; }
    else {
        const int up = ((elems + 63) / 64) * 64;
        g.wave = 0;
        g.threads = up < ENKF_MAX_THREADS ? up : ENKF_MAX_THREADS;
        g.E = (elems + g.threads - 1) / g.threads;
    }
    if (nstim > g.threads) { g.why = "more stimulus columns than threads of a workgroup"; return false; }      // (a lane keeps one column's rows)
    g.lds_bytes = sizeof(double) * enkf_lds_doubles(M, D, NP, NQ, nstim);
    if (g.lds_bytes > ENKF_LDS_LIMIT) { g.why = "members, their parameters and the stimulus do not fit 64 KiB of LDS"; return false; }
    if (T > 2147483647L) { g.why = "too many points for one launch"; return false; }
    g.grid = T;
    return true;
}

// what va_enkf checks before it touches the device (est, obs_var: host memory).  false: `why` says which
inline bool enkf_check_args(long T, int M, int NP, int NQ, int L, int n_obs, int obs_every, int substeps, const int *est,
                            const double *obs_var, double inflation, char *why, size_t nwhy)
{
    if (T < 1 || M < 1 || n_obs < 1 || obs_every < 1 || substeps < 1) {
        snprintf(why, nwhy, "T, M, n_obs, obs_every and substeps must be at least 1 (T=%ld M=%d n_obs=%d obs_every=%d substeps=%d)", T, M,
                 n_obs, obs_every, substeps);
        return false;
    }
    if (NQ < 0 || NQ > NP) { snprintf(why, nwhy, "NQ=%d outside 0 .. NP=%d", NQ, NP); return false; }
    if (NQ > 0 && !est) { snprintf(why, nwhy, "NQ=%d but est is NULL", NQ); return false; }
    for (int q = 0; q < NQ; ++q) {
        if (est[q] < 0 || est[q] >= NP) { snprintf(why, nwhy, "est[%d]=%d outside 0 .. NP-1=%d", q, est[q], NP - 1); return false; }
        for (int r = 0; r < q; ++r)
            if (est[r] == est[q]) { snprintf(why, nwhy, "est[%d] and est[%d] both name parameter %d: repeated", r, q, est[q]); return false; }
    }
    if (L > 0 && !obs_var) { snprintf(why, nwhy, "obs_var is NULL"); return false; }
    for (int j = 0; j < L; ++j)
        if (!(obs_var[j] > 0.0) || !isfinite(obs_var[j])) {
            snprintf(why, nwhy, "obs_var[%d]=%g: observation variances are finite and positive", j, obs_var[j]);
            return false;
        }
    if (!(inflation >= 1.0) || !isfinite(inflation)) { snprintf(why, nwhy, "inflation=%g: finite and at least 1", inflation); return false; }
    return true;
}

// va_enkf's device buffers per point (x0, p, Y, the four statistics, x_end, p_end, status), and the points of a chunk that
// stay under ENKF_WORKSPACE_BYTES (0: not even one)
inline size_t enkf_point_doubles(int D, int NP, int NQ, int L, int M, int n_obs)
{
    return 2 * (size_t)M * D + 2 * (size_t)M * NP + (size_t)n_obs * L + 4 * (size_t)n_obs * (D + NQ) + 1;
}
inline long enkf_chunk_points(size_t point_doubles, long T)
{
    const size_t fit = ENKF_WORKSPACE_BYTES / (sizeof(double) * point_doubles);
    return (long)(fit < (size_t)T ? fit : (size_t)T);
}

}  // namespace va
