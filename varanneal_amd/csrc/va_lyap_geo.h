// va_lyap_geo.h -- launch geometry, LDS layout and argument checks of the Lyapunov-spectrum kernel k_lyap (va_lyap.h) and
// the chunking of va_lyapunov's device workspace, as plain host C++: shared by the launcher, by the host emulation of the
// kernel (lyap_host) and by the CPU check (tests/cpu_emul/lyap_check.cpp, tests/test_lyap_cpu.py).
//
// A workgroup carries RW whole trajectories: each takes K + 1 SLOTS of D columns, slot 0 the nominal state, slots 1 .. K
// the tangents -- all K of them, because the QR re-orthonormalises them together.  A slot starts every `pitch` doubles of
// an LDS image, pitch = D made odd: the QR's dot products run one lane per slot along the columns, so at a time the lanes
// of a wave read one column of up to 64 slots, addresses `pitch` doubles apart; an odd pitch spreads the 32 lanes of a
// half-wave (the group a 64-bit LDS read is banked by) over all 64 banks, where the even pitches D = 32 and 64 would put
// them on one.  The workgroup's elements (slot, column) are numbered slot-major, element q = (r (K + 1) + s) D + i, and lane
// tid owns the elements tid, tid + threads, ..., E of them.
//   (K + 1) D <= 64      one wave, RW = 64 / ((K + 1) D) trajectories side by side, no workgroup barrier
//   wider                one trajectory, min(256, elements rounded up to 64) threads, E <= 8 elements per lane:
//                        (K + 1) D <= 2048, which is every full spectrum to D = 44 and 31 exponents at D = 64
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdio.h>

#include "va_core.h"

namespace va {

constexpr int LYAP_MAX_D = 64;
constexpr int LYAP_MAX_E = 8;
constexpr int LYAP_MAX_THREADS = 256;
constexpr int LYAP_MAX_ELEMS = LYAP_MAX_THREADS * LYAP_MAX_E;      // (K + 1) D of one trajectory
constexpr size_t LYAP_LDS_LIMIT = 64 * 1024;
constexpr size_t LYAP_WORKSPACE_BYTES = (size_t)1 << 30;           // the device buffers of one chunk of trajectories stay under this

struct LyapGeo {
    int RW = 0;             // trajectories side by side in one workgroup (more than 1 only in one wave)
    int threads = 0;        // per workgroup: 64 (one wave), or min(256, elements rounded up to 64)
    int E = 0;              // elements per lane
    int wave = 0;           // 1: one wave per workgroup, ordered by the wave's own LDS order; 0: workgroup barriers
    int pitch = 0;          // doubles from one slot of an image to the next: D | 1
    size_t lds_bytes = 0;   // lyap_lds_doubles
    long grid = 0;          // workgroups: ceil(T / RW)
    const char *why = "";   // the refusal, when plan_lyap returns false
};

VA_HD int lyap_pitch(int D) { return D | 1; }

// images [2][RW][K + 1][pitch], parameters [RW][NP], ONE zero parameter tangent [NP], gains [RW][D], stimulus [2][nstim],
// the QR's coefficients and squared norms [2][RW][K], status [RW]
inline size_t lyap_lds_doubles(int RW, int K, int D, int NP, int nstim)
{
    return (size_t)RW * (2 * (size_t)(K + 1) * lyap_pitch(D) + NP + D + 2 * (size_t)K + 1) + NP + 2 * (size_t)nstim;
}

// element q of a workgroup -> (trajectory slot r, slot s, column i); r >= RW: nobody's (the lane idles there)
VA_HD void lyap_elem(int K, int D, int q, int *r, int *s, int *i)
{
    const int slot = q / D;
    *i = q - slot * D;
    *r = slot / (K + 1);
    *s = slot - *r * (K + 1);
}

inline bool plan_lyap(int D, long T, int K, int NP, int nstim, LyapGeo &g)
{
    g = LyapGeo();
    if (D < 1 || T < 1 || K < 1 || NP < 0 || nstim < 0) { g.why = "bad sizes"; return false; }
    if (K > D) { g.why = "more exponents than state columns"; return false; }
    if (D > LYAP_MAX_D) { g.why = "k_lyap carries states of at most 64 columns"; return false; }
    const int elems = (K + 1) * D;
    if (elems > LYAP_MAX_ELEMS) {
        g.why = "(K + 1) D is more than 2048: a workgroup of 256 threads x 8 elements per lane holds a trajectory and all its tangents";
        return false;
    }
    g.pitch = lyap_pitch(D);
    if (elems <= 64) { g.wave = 1; g.threads = 64; g.E = 1; g.RW = 64 / elems; }
    else {
        const int up = ((elems + 63) / 64) * 64;
        g.wave = 0; g.RW = 1;
        g.threads = up < LYAP_MAX_THREADS ? up : LYAP_MAX_THREADS;
        g.E = (elems + g.threads - 1) / g.threads;
    }
    if (nstim > g.threads) { g.why = "more stimulus columns than threads of a workgroup"; return false; }      // (a lane keeps one column's rows)
    g.lds_bytes = sizeof(double) * lyap_lds_doubles(g.RW, K, D, NP, nstim);
    if (g.lds_bytes > LYAP_LDS_LIMIT) { g.why = "parameters, stimulus and stage inputs do not fit 64 KiB of LDS"; return false; }
    const long groups = (T + g.RW - 1) / g.RW;
    if (groups > 2147483647L) { g.why = "too many trajectories for one launch"; return false; }
    g.grid = groups;
    return true;
}

// what va_lyapunov checks before it touches the device (coupling: host memory, [T][D] or NULL).  false: `why` says which
inline bool lyap_check_args(long T, int D, int K, int n_steps, int substeps, int qr_every, int n_skip, const double *coupling,
                            char *why, size_t nwhy)
{
    if (T < 1 || n_steps < 1 || substeps < 1 || qr_every < 1) {
        snprintf(why, nwhy, "T, n_steps, substeps and qr_every must be at least 1 (T=%ld n_steps=%d substeps=%d qr_every=%d)", T, n_steps,
                 substeps, qr_every);
        return false;
    }
    if (K < 1 || K > D) { snprintf(why, nwhy, "K=%d outside 1 .. D=%d", K, D); return false; }
    if (n_steps % qr_every) { snprintf(why, nwhy, "n_steps=%d is not a multiple of qr_every=%d", n_steps, qr_every); return false; }
    const int n_qr = n_steps / qr_every;
    if (n_skip < 0 || n_skip >= n_qr) { snprintf(why, nwhy, "n_skip=%d outside 0 .. n_qr - 1 = %d", n_skip, n_qr - 1); return false; }
    if (coupling)
        for (size_t e = 0; e < (size_t)T * D; ++e)
            if (!(coupling[e] >= 0.0) || !isfinite(coupling[e])) {
                snprintf(why, nwhy, "coupling[%zu][%zu]=%g: gains are finite and not negative", e / D, e % D, coupling[e]);
                return false;
            }
    return true;
}

// va_lyapunov's device buffers per trajectory (x0, p, Q0, coupling, logsum, x_end, Q_end, trace, status), and the
// trajectories of a chunk that stay under LYAP_WORKSPACE_BYTES (0: not even one)
inline size_t lyap_traj_doubles(int D, int NP, int K, int n_qr, bool trace)
{
    return 3 * (size_t)D + NP + 2 * (size_t)K * D + K + (trace ? (size_t)n_qr * K : 0) + 1;
}
inline long lyap_chunk_trajs(size_t traj_doubles, long T)
{
    const size_t fit = LYAP_WORKSPACE_BYTES / (sizeof(double) * traj_doubles);
    return (long)(fit < (size_t)T ? fit : (size_t)T);
}

}  // namespace va
