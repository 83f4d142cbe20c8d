// va_predict_tlm_geo.h -- launch geometry of the tangent-linear RK4 predictor k_predict_tlm (va_predict_tlm.h) and the
// chunking of va_predict_tangent's device workspace, as plain host C++: shared by the launcher, by the host emulation of
// the kernel (predict_tlm_host) and by the CPU check (tests/cpu_emul/predict_tlm_check.cpp, tests/test_predict_tlm_cpu.py).
//
// A workgroup carries RW trajectories; each of them takes chunk + 1 SLOTS of D columns: slot 0 is the nominal trajectory
// (recomputed by every workgroup that needs it: workgroups stay independent), slots 1 .. chunk are `chunk` consecutive
// tangent directions.  The workgroup's elements (slot, column) are numbered slot-major, element q = (r (chunk + 1) + s) D + i,
// and lane tid owns the elements tid, tid + threads, ..., E of them.
//   (nvec + 1) D <= 64      one wave, all directions, RW = 64 / ((nvec + 1) D) trajectories side by side
//   2 D <= 64               one wave, one trajectory, chunk = 64 / D - 1 directions of it
//   wider                   one trajectory, up to 256 threads with E <= 4 elements per lane: chunk = 1024 / D - 1 directions,
//                           spread evenly over the chunks; past D = 512 one direction beside the nominal, E = 5 .. 8
#pragma once
#include <stddef.h>

#include "va_core.h"
#include "va_predict_geo.h"

namespace va {

constexpr int PREDICT_TLM_MAX_E = 8;       // 4 wherever a direction fits beside the nominal with it (D <= 512)
constexpr size_t PREDICT_TLM_LDS_LIMIT = 64 * 1024;
constexpr size_t PREDICT_TLM_WORKSPACE_BYTES = (size_t)1 << 30;      // the device buffers of one chunk of trajectories stay under this

struct PredictTlmGeo {
    int RW = 0;             // trajectories side by side in one workgroup (more than 1 only when all directions fit one wave)
    int chunk = 0;          // directions per workgroup (slots 1 .. chunk)
    int nchunks = 0;        // workgroups per trajectory group: ceil(nvec / chunk)
    int threads = 0;        // per workgroup: 64 (one wave), or min(256, elements rounded up to 64)
    int E = 0;              // elements per lane
    int wave = 0;           // 1: one wave per workgroup, ordered by the wave's own LDS order; 0: workgroup barriers
    size_t lds_bytes = 0;   // stage inputs [2][RW][chunk + 1][D], parameters [RW][NP], parameter tangents [RW][chunk][NP], stimulus [2][nstim]
    long grid = 0;          // workgroups: ceil(T / RW) nchunks
    const char *why = "";   // the refusal, when plan_predict_tlm returns false
};

inline size_t predict_tlm_lds_doubles(int RW, int chunk, int D, int NP, int nstim)
{
    return (size_t)RW * (2 * (size_t)(chunk + 1) * D + (size_t)(chunk + 1) * NP) + 2 * (size_t)nstim;
}

// element q of a workgroup -> (trajectory slot r, direction slot s, column i); r >= RW: nobody's (the lane idles there)
VA_HD void predict_tlm_elem(const PredictTlmGeo &g, int D, int q, int *r, int *s, int *i)
{
    const int slot = q / D;
    *i = q - slot * D;
    *r = slot / (g.chunk + 1);
    *s = slot - *r * (g.chunk + 1);
}

inline bool plan_predict_tlm(int D, long T, int nvec, int NP, int nstim, PredictTlmGeo &g)
{
    g = PredictTlmGeo();
    if (D < 1 || T < 1 || nvec < 1 || NP < 0 || nstim < 0) { g.why = "bad sizes"; return false; }
    if (D > PREDICT_MAX_D) { g.why = "the predictor carries states of at most 1024 columns (256 threads x 4 columns per lane)"; return false; }
    if (2 * D <= 64) {
        const int slots = 64 / D;
        g.wave = 1; g.threads = 64; g.E = 1;
        if (nvec + 1 <= slots) { g.chunk = nvec; g.RW = slots / (nvec + 1); }
        else { g.chunk = slots - 1; g.RW = 1; }
    } else {
        g.wave = 0; g.RW = 1;
        const int most = D <= 512 ? 256 * PREDICT_MAX_E / D - 1 : 1;      // directions beside the nominal
        g.chunk = nvec < most ? nvec : most;
    }
    // (a chunk's parameter tangents share the LDS with the stage inputs: fewer directions per workgroup where they are long)
    while (g.chunk > 1 && sizeof(double) * predict_tlm_lds_doubles(g.RW, g.chunk, D, NP, nstim) > PREDICT_TLM_LDS_LIMIT) --g.chunk;
    g.nchunks = (nvec + g.chunk - 1) / g.chunk;
    if (g.RW == 1) g.chunk = (nvec + g.nchunks - 1) / g.nchunks;          // even chunks: the same number of workgroups, fewer idle slots
    if (!g.wave) {
        const int elems = (g.chunk + 1) * D, up = ((elems + 63) / 64) * 64;
        g.threads = up < 256 ? up : 256;
        g.E = (elems + g.threads - 1) / g.threads;
    }
    if (nstim > g.threads) { g.why = "more stimulus columns than threads of a workgroup"; return false; }      // (a lane keeps one column's rows)
    g.lds_bytes = sizeof(double) * predict_tlm_lds_doubles(g.RW, g.chunk, D, NP, nstim);
    if (g.lds_bytes > PREDICT_TLM_LDS_LIMIT) { g.why = "parameters, parameter tangents and stage inputs do not fit 64 KiB of LDS"; return false; }
    const long groups = (T + g.RW - 1) / g.RW;
    if (groups > 2147483647L / g.nchunks) { g.why = "too many trajectories and directions for one launch"; return false; }
    g.grid = groups * g.nchunks;
    return true;
}

// va_predict_tangent's device buffers per trajectory (x0, p, V0, out, dX, var, cov when asked for), and the trajectories of
// a chunk that stay under PREDICT_TLM_WORKSPACE_BYTES (0: not even one)
inline size_t predict_tlm_traj_doubles(int D, int NP, int NPest, int nvec, int n_out, bool cov)
{
    const size_t row = (size_t)n_out * D;
    return (size_t)D + NP + (size_t)nvec * (D + NPest) + 2 * row + (size_t)nvec * row + (cov ? row * D : 0);
}
inline long predict_tlm_chunk_trajs(size_t traj_doubles, long T)
{
    const size_t fit = PREDICT_TLM_WORKSPACE_BYTES / (sizeof(double) * traj_doubles);
    return (long)(fit < (size_t)T ? fit : (size_t)T);
}

}  // namespace va
