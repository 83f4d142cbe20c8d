// va_predict_adj_geo.h -- launch geometry of the adjoint RK4 predictor k_predict_adj (va_predict_adj.h) and the chunking of
// va_predict_adjoint's device workspace, as plain host C++: shared by the launcher, by the host emulation of the kernel
// (predict_adj_host) and by the CPU check (tests/cpu_emul/predict_adj_check.cpp, tests/test_predict_adj_cpu.py).
//
// The slots are va_predict_tlm_geo.h's: a workgroup carries RW trajectories, each of them chunk + 1 SLOTS of D columns:
// slot 0 is the nominal trajectory (every workgroup that needs it integrates it and keeps checkpoints of its own: workgroups
// stay independent), slots 1 .. chunk are `chunk` consecutive cotangent sets.  Element q = (r (chunk + 1) + s) D + i, lane
// tid owns the elements tid, tid + threads, ..., E of them.
//   (ncot + 1) D <= 64      one wave, all cotangent sets, RW = 64 / ((ncot + 1) D) trajectories side by side
//   2 D <= 64               one wave, one trajectory, chunk = 64 / D - 1 cotangent sets of it
//   wider                   one trajectory, up to 256 threads with E <= 4 elements per lane: chunk = 1024 / D - 1 sets, spread
//                           evenly over the chunks; past D = 512 one set beside the nominal, E = 5 .. 8
// LDS (doubles): the nominal's four stage inputs [4][RW][D], the stage cotangents [2][RW][chunk][D], parameters [RW][NP],
// the parameter partials per (slot, column) [RW][chunk][D][pitch] with pitch = NP made odd (lanes of neighbouring columns
// then hit different banks), and the stimulus at the stage times [2][3][nstim].
#pragma once
#include <stddef.h>

#include "va_core.h"
#include "va_predict_geo.h"

namespace va {

constexpr int PREDICT_ADJ_MAX_E = 8;       // 4 wherever a cotangent set fits beside the nominal with it (D <= 512)
constexpr size_t PREDICT_ADJ_LDS_LIMIT = 64 * 1024;
constexpr size_t PREDICT_ADJ_WORKSPACE_BYTES = (size_t)1 << 30;      // the device buffers of one chunk of trajectories stay under this

struct PredictAdjGeo {
    int RW = 0;             // trajectories side by side in one workgroup (more than 1 only when all sets fit one wave)
    int chunk = 0;          // cotangent sets per workgroup (slots 1 .. chunk)
    int nchunks = 0;        // workgroups per trajectory group: ceil(ncot / chunk)
    int threads = 0;        // per workgroup: 64 (one wave), or min(256, elements rounded up to 64)
    int E = 0;              // elements per lane
    int wave = 0;           // 1: one wave per workgroup, ordered by the wave's own LDS order; 0: workgroup barriers
    int pitch = 0;          // doubles between the parameter partials of two columns: NP, made odd
    size_t lds_bytes = 0;
    long grid = 0;          // workgroups: ceil(T / RW) nchunks
    const char *why = "";   // the refusal, when plan_predict_adj returns false
};

VA_HD int predict_adj_pitch(int NP) { return NP | 1; }

inline size_t predict_adj_lds_doubles(int RW, int chunk, int D, int NP, int nstim)
{
    return (size_t)RW * (4 * (size_t)D + 2 * (size_t)chunk * D + NP + (size_t)chunk * D * predict_adj_pitch(NP)) + 6 * (size_t)nstim;
}

// element q of a workgroup -> (trajectory slot r, cotangent slot s, column i); r >= RW: nobody's (the lane idles there)
VA_HD void predict_adj_elem(const PredictAdjGeo &g, int D, int q, int *r, int *s, int *i)
{
    const int slot = q / D;
    *i = q - slot * D;
    *r = slot / (g.chunk + 1);
    *s = slot - *r * (g.chunk + 1);
}

inline bool plan_predict_adj(int D, long T, int ncot, int NP, int nstim, PredictAdjGeo &g)
{
    g = PredictAdjGeo();
    if (D < 1 || T < 1 || ncot < 1 || NP < 0 || nstim < 0) { g.why = "bad sizes"; return false; }
    if (D > PREDICT_MAX_D) { g.why = "the predictor carries states of at most 1024 columns (256 threads x 4 columns per lane)"; return false; }
    if (2 * D <= 64) {
        const int slots = 64 / D;
        g.wave = 1; g.threads = 64; g.E = 1;
        if (ncot + 1 <= slots) { g.chunk = ncot; g.RW = slots / (ncot + 1); }
        else { g.chunk = slots - 1; g.RW = 1; }
        // (trajectories side by side share the LDS: fewer of them before fewer sets)
        while (g.RW > 1 && sizeof(double) * predict_adj_lds_doubles(g.RW, g.chunk, D, NP, nstim) > PREDICT_ADJ_LDS_LIMIT) --g.RW;
    } else {
        g.wave = 0; g.RW = 1;
        const int most = D <= 512 ? 256 * PREDICT_MAX_E / D - 1 : 1;      // cotangent sets beside the nominal
        g.chunk = ncot < most ? ncot : most;
    }
    // (a set's parameter partials share the LDS with the stage images: fewer sets per workgroup where the parameters are many)
    while (g.chunk > 1 && sizeof(double) * predict_adj_lds_doubles(g.RW, g.chunk, D, NP, nstim) > PREDICT_ADJ_LDS_LIMIT) --g.chunk;
    g.nchunks = (ncot + g.chunk - 1) / g.chunk;
    if (g.RW == 1) g.chunk = (ncot + g.nchunks - 1) / g.nchunks;          // even chunks: the same number of workgroups, fewer idle slots
    if (!g.wave) {
        const int elems = (g.chunk + 1) * D, up = ((elems + 63) / 64) * 64;
        g.threads = up < 256 ? up : 256;
        g.E = (elems + g.threads - 1) / g.threads;
    }
    g.pitch = predict_adj_pitch(NP);
    if (nstim > g.threads) { g.why = "more stimulus columns than threads of a workgroup"; return false; }      // (a lane keeps one column's rows)
    g.lds_bytes = sizeof(double) * predict_adj_lds_doubles(g.RW, g.chunk, D, NP, nstim);
    if (g.lds_bytes > PREDICT_ADJ_LDS_LIMIT) { g.why = "parameters, parameter partials and stage images do not fit 64 KiB of LDS"; return false; }
    const long groups = (T + g.RW - 1) / g.RW;
    if (groups > 2147483647L / g.nchunks) { g.why = "too many trajectories and cotangent sets for one launch"; return false; }
    g.grid = groups * g.nchunks;
    return true;
}

// checkpoints of one launch: the state at the start of every RK4 step, per workgroup and trajectory slot [grid][RW][Q][D]
inline size_t predict_adj_ckpt_doubles(const PredictAdjGeo &g, int D, long long Q) { return (size_t)g.grid * g.RW * (size_t)Q * D; }

// va_predict_adjoint's device buffers per trajectory: x0, p, the cotangents G (or the observations, when every trajectory has
// its own), out, gx0, gp, cost and the checkpoints of every workgroup that integrates the trajectory -- and the
// trajectories of a chunk that stay under PREDICT_ADJ_WORKSPACE_BYTES (0: not even one).  (One more group of RW slots of
// checkpoints is set aside per launch for the part-filled last workgroup: `spare`.)
inline size_t predict_adj_traj_doubles(int D, int NP, int NPest, int ncot, int n_out, long long Q, int nchunks, size_t cot_doubles)
{
    return (size_t)D + NP + cot_doubles + (size_t)n_out * D + (size_t)ncot * (D + NPest) + 1 + (size_t)nchunks * (size_t)Q * D;
}
inline long predict_adj_chunk_trajs(size_t traj_doubles, size_t spare_doubles, long T)
{
    const size_t room = PREDICT_ADJ_WORKSPACE_BYTES / sizeof(double);
    if (spare_doubles >= room) return 0;
    const size_t fit = (room - spare_doubles) / traj_doubles;
    return (long)(fit < (size_t)T ? fit : (size_t)T);
}

}  // namespace va
