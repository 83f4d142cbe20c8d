// va_predict_geo.h -- launch geometry of the batched RK4 predictor k_predict (va_predict.h), as plain host C++: shared by
// the launcher, by the host emulation of the kernel (predict_host) and by the CPU check that records it
// (tests/cpu_emul/predict_check.cpp, tests/test_predict_cpu.py).
#pragma once
#include <stddef.h>

#include "va_core.h"

namespace va {

constexpr int PREDICT_MAX_D = 1024;        // widest state: 256 threads x 4 columns per lane
constexpr int PREDICT_MAX_E = 4;

struct PredictGeo {
    int RW = 0;             // trajectories side by side in one workgroup (D <= 64: 64 / D, one wave; wider states: 1)
    int threads = 0;        // per workgroup: 64 (one wave), or min(256, D rounded up to 64)
    int E = 0;              // state columns per lane: lane tid owns columns tid, tid + threads, ...
    int wave = 0;           // 1: one wave per workgroup, ordered by the wave's own LDS order; 0: workgroup barriers
    size_t lds_bytes = 0;   // stage inputs [2][RW][D], parameters [RW][NP], interpolated stimulus [2][nstim]
    long grid = 0;          // workgroups: ceil(T / RW)
    const char *why = "";   // the refusal, when plan_predict returns false
};

// lane -> (trajectory slot of the workgroup, first column); slot >= RW: the lane idles
VA_HD void predict_lane(const PredictGeo &g, int D, int tid, int *slot, int *col0)
{
    if (g.wave) { *slot = tid / D; *col0 = tid - *slot * D; }
    else { *slot = 0; *col0 = tid; }
}

inline size_t predict_lds_doubles(int RW, int D, int NP, int nstim) { return (size_t)RW * (2 * (size_t)D + NP) + 2 * (size_t)nstim; }

inline bool plan_predict(int D, long T, int NP, int nstim, PredictGeo &g)
{
    g = PredictGeo();
    if (D < 1 || T < 1 || NP < 0 || nstim < 0) { g.why = "bad sizes"; return false; }
    if (D > PREDICT_MAX_D) { g.why = "the predictor carries states of at most 1024 columns (256 threads x 4 columns per lane)"; return false; }
    if (D <= 64) { g.wave = 1; g.RW = 64 / D; g.threads = 64; g.E = 1; }
    else {
        g.wave = 0; g.RW = 1;
        const int up = ((D + 63) / 64) * 64;
        g.threads = up < 256 ? up : 256;
        g.E = (D + g.threads - 1) / g.threads;
    }
    if (nstim > g.threads) { g.why = "more stimulus columns than threads of a workgroup"; return false; }      // (a lane keeps one column's rows)
    g.lds_bytes = sizeof(double) * predict_lds_doubles(g.RW, D, NP, nstim);
    if (g.lds_bytes > 64 * 1024) { g.why = "parameters and stage inputs do not fit 64 KiB of LDS"; return false; }
    g.grid = (T + g.RW - 1) / g.RW;
    if (g.grid > 2147483647L) { g.why = "too many trajectories for one launch"; return false; }
    return true;
}

}  // namespace va
