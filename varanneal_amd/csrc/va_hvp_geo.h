// va_hvp_geo.h -- launch geometry of the Hessian-vector kernel k_hvp (va_hvp.h), as plain host C++: shared by the
// launcher (va_hess_vec), by the host run of the kernel's phases and by the CPU check that records it
// (tests/cpu_emul/hvp_check.cpp, tests/test_hvp_cpu.py).
#pragma once
#include <stddef.h>

#include "va_core.h"

namespace va {

constexpr int HVP_THREADS = 256;                    // 4 waves per workgroup, as the flat evaluation kernel
constexpr size_t HVP_LDS_CAP = 160 * 1024;          // a CU's whole LDS (the opt-in of va_device.h eval_op)

struct HvpGeo {
    int T = 0;              // time rows a workgroup owns
    int ntiles = 0;         // ceil(N / T)
    int Tmax = 0;           // the most rows whose six staged images fit the LDS
    int maxD = 0;           // the widest state of which ONE owned row fits (what a refusal names)
    size_t lds_bytes = 0;
    long grid = 0;          // workgroups: points x directions x tiles
    const char *why = "";   // the refusal, when plan_hvp returns false
};

// Simpson-Hermite tiles of an ODD number of rows (the flat evaluation kernel only takes even ones).  Such a tile may end on
// an even row m, whose adjoint reads q of row m + 1, i.e. the interval's far end m + 2: it stages two more rows behind
// Halo<DISC>::HR and forms q for one more row.  And it may START on an odd row n0: its first staged row n0 - 2 is then odd,
// and tile_q forms that row's (never used) q from the row before it: every image gets one more row in FRONT, held at
// zero, so that this read stays inside the image.  Every other tile uses the halos of Halo<DISC> as they are.
VA_HD int hvp_front_rows(int disc, int T) { return (disc == DISC_SH && (T & 1)) ? 1 : 0; }
VA_HD int hvp_back_rows(int disc, int T) { return (disc == DISC_SH && (T & 1)) ? 2 : 0; }
VA_HD int hvp_extra_rows(int disc, int T) { return hvp_front_rows(disc, T) + hvp_back_rows(disc, T); }
VA_HD int hvp_halo(int disc, int T) { return (disc == DISC_SH ? 2 : 1) + 1 + hvp_extra_rows(disc, T); }      // HL + HR (+ 3)
// LDS of a workgroup: x, f -> s, q and v, fdot -> sdot, qdot at (T + halo) rows each; the waves' partial parameter rows
inline size_t hvp_lds_doubles(int T, int D, int disc, int NP)
{
    return (size_t)6 * (T + hvp_halo(disc, T)) * D + (size_t)(HVP_THREADS / 64) * (NP > 0 ? NP : 1);
}

// tile_rows: 0 = the library's choice, else the rows per tile to use (refused when they do not fit)
inline bool plan_hvp(int D, int N, int disc, int NP, long npts, long nvec, int tile_rows, HvpGeo &g)
{
    g = HvpGeo();
    if (D < 1 || N < 2 || NP < 0 || npts < 1 || nvec < 1 || tile_rows < 0) { g.why = "bad sizes"; return false; }
    const size_t cap = HVP_LDS_CAP / sizeof(double), red = (size_t)(HVP_THREADS / 64) * (NP > 0 ? NP : 1);
    // the smallest tile: one owned row, or two where that takes fewer staged rows (Simpson-Hermite: 2 + 3 against 1 + 6)
    const int rows1 = 1 + hvp_halo(disc, 1), rows2 = 2 + hvp_halo(disc, 2);
    g.maxD = (int)((cap - red) / (6 * (size_t)(rows1 < rows2 ? rows1 : rows2)));
    if (D > g.maxD) { g.why = "state too wide: six staged images of the smallest tile and its halo do not fit 160 KiB of LDS"; return false; }
    auto fits = [&](int T) { return hvp_lds_doubles(T, D, disc, NP) <= cap; };
    const size_t rows = (cap - red) / (6 * (size_t)D);
    g.Tmax = (int)(rows < (size_t)N ? rows : (size_t)N);
    while (g.Tmax > 1 && !fits(g.Tmax)) --g.Tmax;
    if (tile_rows > 0) {
        if (tile_rows > g.Tmax || !fits(tile_rows)) { g.why = "tile_rows: that many rows do not fit the LDS (or exceed the path)"; return false; }
        g.T = tile_rows;
    } else {
        // about four elements per thread and at least 16 rows (the halo rows are evaluated again by every tile)
        int want = (4 * HVP_THREADS + D - 1) / D;
        if (want < 16) want = 16;
        g.T = want < g.Tmax ? want : g.Tmax;
        if (disc == DISC_SH && (g.T & 1) && g.T > 1 && g.T < N) --g.T;      // (even tiles need no extra rows)
    }
    g.ntiles = (N + g.T - 1) / g.T;
    g.lds_bytes = sizeof(double) * hvp_lds_doubles(g.T, D, disc, NP);
    const long long grid = (long long)npts * nvec * g.ntiles;
    if (grid > 2147483647LL) { g.why = "points x directions x tiles exceed one launch"; return false; }
    g.grid = (long)grid;
    return true;
}

}  // namespace va
