// va_eval_geo.h -- which evaluation kernel a problem runs and with what tile geometry, as plain host C++: the flat
// k_eval, the workgroup column runs k_eval3, the wave-private column runs k_eval4 and the streaming strips k_eval5 each
// have a planner of their own, and plan_eval() is the order in which they are tried.  Included by the host
// (va_capi.hip) and by the CPU check of the plans (tests/cpu_emul/plan_check.cpp, tests/test_eval_geometry.py against
// tests/golden/eval_plans.txt).
#pragma once
#include <stddef.h>

#include <algorithm>
#include <vector>

#include "../../include/varanneal_amd.h"
#include "va_core.h"
#include "va_tile3.h"
#include "va_tile4.h"
#include "va_tile5.h"

namespace va {

// What the model offers besides the flat form every model has.
struct EvalForm {
    int ne = 0;                 // products per element of its column form (RhsL96s::NE; a module's RhsUserCol::NE), or 0: none
    int ghost = 0;              // ghost columns per side of its ghosted form (RhsL96g::GHOST; a module's RhsUserG::GHOST), or 0: none
    bool has_reach5 = false;    // the column form may run the streaming kernel (va_tile5.h), with these reaches
    int reach5[4] = {0, 0, 0, 0};      // {xl, xr, gl, gr}
    int lin = 0;                // the flat form carries a dense constant linear part (RHS::LINEAR): one more staged array
    int nb = 0;                 // neighbour columns its column form reads (RhsL96s::NB; a module's RhsUserCol::NB), or 0: not known
};

// The chosen kernel and its geometry: what va_problem_create copies into the device image.
struct EvalPlan {
    int emode = 0, RY = 0, NT = 0, maxr = 0, T = 0, ntiles = 0;      // as Dims (va_core.h)
    int ghost = 2;
    Geo4 g4{};                  // emode 4, with
    int wg4 = 1;                //   row groups (ntiles counts them: 4 waves, g4.T rows, one row of the partial tables) per workgroup
    Geo5 g5{};                  // emode 5, with
    std::vector<int> ystrip;    //   [NS][2] per strip: first data column staged (even), 16-byte pieces per observation row
};

// The problems only the flat kernel carries, whatever forms the model has: NULL, or why.
inline const char *flat_only_reason(const va_problem_desc *d)
{
    if (d->lower && d->upper) return "box bounds (carried by the flat kernel only)";      // the clamp / projected gradient
    if (d->p_time_dependent) return "time-dependent parameters";                           // per-row parameters
    if (d->rm_kind == 2 || d->rf_kind == 2) return "full RM / RF matrices (flat kernel only)";
    return nullptr;
}

// the next shorter run length of the column-run kernels: Simpson-Hermite keeps K even; never below 4
inline int shorter_run(int K, bool sh) { return K - ((sh || K == 5) ? (K == 5 ? 1 : 2) : 1); }

// Small grids run as a handful of workgroups per CU, all resident at once: the busiest CU sets the time.  The run
// length kmin..8 whose (rounds of resident workgroups) x (rows per lane + fixed per-workgroup cost) is smallest; ties go
// to 6.  rows1: rows a workgroup owns per row of run length; resident(k): workgroups the chip holds at once.
template <class F>
inline int fewest_rounds_run(const va_problem_desc *d, int rows1, int kmin, bool sh, F resident)
{
    int K = 6;
    long best = -1;
    for (int k = kmin; k <= 8; ++k) {
        if (sh && (k & 1)) continue;              // Simpson-Hermite runs start on even rows
        const long wgs = (long)d->batch * ((d->N_model + rows1 * k - 1) / (rows1 * k)), per_round = resident(k);
        const long cost = ((wgs + per_round - 1) / per_round) * (k + 2) * 4 + (k == 6 ? 0 : 1);     // ties go to 6
        if (best < 0 || cost < best) { best = cost; K = k; }
    }
    return K;
}

// streaming column strips: wide even states, a column form, scalar or per-row weights with
// data at every model time (what every BASELINE config has); anything else keeps the tile kernels
inline bool plan_eval5(const va_problem_desc *d, const EvalForm &f, EvalPlan &p)
{
    const int D = d->D, N = d->N_model, ne = f.ne;
    const bool sh = d->disc == VA_DISC_SIMPSON_HERMITE;
    const int *reach5 = f.reach5;
    const bool ws5 = d->rm_kind <= 1 && d->rf_kind <= 1 && d->merr_nskip >= 1 && d->L >= 1;     // (full matrices: flat kernel)
    if (!(f.has_reach5 && ne > 0 && ws5 && D > 64 && (!sh || (N & 1)) && tile5_ok(D, reach5[0], reach5[1], reach5[2], reach5[3])))
        return false;
    Geo5 g = tile5_cols(D, reach5[0], reach5[1], reach5[2], reach5[3]);
    g.ne = ne;
    // segments: as many workgroups as the chip holds at once (four 4-wave groups per CU: 128 registers, 40 KiB
    // of LDS each), every one with the same number of rows; at least 32 rows per segment
    const long per_row = (long)d->batch * g.NSG;
    long nseg = (4L * 256) / per_row;
    if (d->tile_rows > 0) nseg = (N + d->tile_rows - 1) / d->tile_rows;
    if (nseg > N / 32) nseg = N / 32;
    if (nseg < 1) nseg = 1;
    g.SEGL = (int)((N + nseg - 1) / nseg);
    g.SEGL = (g.SEGL + 1) & ~1;
    g.NSEG = (N + g.SEGL - 1) / g.SEGL;
    // observation rows per strip: the data columns of the strip's own state columns (Lidx ascending on the device)
    std::vector<int> ls(d->Lidx, d->Lidx + d->L), ystrip(2 * g.NS, 0);
    std::sort(ls.begin(), ls.end());
    g.YPMAX = 1;
    for (int s5 = 0; s5 < g.NS; ++s5) {
        const int c0 = tile5_c0(D, g.NS, s5), c1 = tile5_c0(D, g.NS, s5 + 1);
        const int l0 = (int)(std::lower_bound(ls.begin(), ls.end(), c0) - ls.begin());
        const int l1 = (int)(std::lower_bound(ls.begin(), ls.end(), c1) - ls.begin());
        int start = l0 & ~1;
        int yp = (l1 - start + 1) / 2;
        if (yp < 1) yp = 1;                           // (every staging instruction has an active lane: the queue counts are exact)
        ystrip[2 * s5] = start; ystrip[2 * s5 + 1] = yp;
        if (yp > g.YPMAX) g.YPMAX = yp;
    }
    // (a strip owns at most T5_CW_MAX = 56 columns, so distinct observed columns stage at most 29 pieces: only a
    // descriptor that lists a state column twice, which va_problem_create refuses, is turned away here)
    if (g.YPMAX > 32) return false;
    // ring depth: four slots (three requested ahead) while four workgroups still share a CU's 160 KiB, else three.
    // Measured at C4 (profiles/r03_e5_experiments.txt): 3 and 4 slots equal; 6 slots drop a workgroup per CU (+33 %)
    g.xdpp = (reach5[2] <= 2 && reach5[3] <= 2) ? 1 : 0;
    auto fits = [&](int nslot, bool lsr) { return (size_t)g.WPG * tile5_wave_doubles(g, nslot, lsr) * sizeof(double) <= 40 * 1024; };
    g.nslot = fits(4, false) ? 4 : 3;
    g.nslot_ls = fits(4, true) ? 4 : 3;
    g.warr = (d->rm_kind == 1 || d->rf_kind == 1 || d->merr_nskip > 1) ? 1 : 0;
    if (g.warr) g.nslot = g.nslot_ls = 3;          // (two more images per slot; only the three-slot instantiations exist)
    g.LY = (d->L + 1) & ~1;                        // (data rows are staged by 16-byte pieces: an odd L gets a pad column on the device)
    p.g5 = g;
    p.ystrip = ystrip;
    p.emode = 5; p.RY = 0; p.NT = 64 * g.WPG; p.maxr = 2; p.T = g.SEGL;
    p.ntiles = g.NSEG * g.NSG;
    return true;
}

// 4-wave workgroups of k_eval4 a CU holds, by registers (eval4_wpc, va_eval4.h); a column form whose neighbour count
// is not known counts as the smaller
inline int eval4_per_cu(int K, int nb) { return (nb > 0 && K <= 7 && K * nb <= 28) ? 3 : 2; }

constexpr int EVAL4_CUS = 256;              // (the device the planners' round arithmetic is written for)
// Does a handle start on the width plan_eval4_groups chooses?  No: measured at C3 (64 seeds, N = 1000, runs of 7 rows; same
// box, alternated, profiles/r06_groups_c3.txt) one 12-wave workgroup per CU runs 9.07-9.09 us against 8.50-8.54 us for three
// 4-wave workgroups -- twelve waves now wait at the publishing barrier for the slowest of them instead of four.  Handles
// start on 4-wave workgroups; va_problem_tune(VA_TUNE_WIDE, 1) puts one on the rule's width.
constexpr bool EVAL4_WIDE_DEFAULT = false;

// Row groups per workgroup of k_eval4, for `ntiles` row groups per seed at run length K.  A grid that is ONE resident
// round of w 4-wave workgroups per CU runs in lockstep: the w workgroups of a CU stage, compute, publish and store
// together, each with a publishing wave, an arrival and a dispatch slot of its own.  G of them as one workgroup keep
// the waves per SIMD, the registers and the LDS of the CU as they are and leave one of each.  The largest G <= w for
// which the busiest CU still owns no more row groups than before and the workgroup's LDS fits; 1 for any grid of more
// than one round.
inline int plan_eval4_groups(long batch, int ntiles, int K, int nb, const Geo4 &g4)
{
    const int w = eval4_per_cu(K, nb);
    const long grid1 = batch * ntiles, rounds1 = (grid1 + EVAL4_CUS - 1) / EVAL4_CUS;      // (row groups on the busiest CU)
    if (grid1 > (long)EVAL4_CUS * w) return 1;
    for (int G = w; G > 1; --G) {
        const long grid = batch * ((ntiles + G - 1) / G), rounds = (grid + EVAL4_CUS - 1) / EVAL4_CUS;
        if (G * rounds <= rounds1 && sizeof(double) * (size_t)G * g4.NW * g4.WAVE <= 160 * 1024) return G;
    }
    return 1;
}

// wave-private column runs: T = 4 waves x RW runs x K rows, narrow even states that fill a wave, a column form
inline bool plan_eval4(const va_problem_desc *d, const EvalForm &f, EvalPlan &p)
{
    const int D = d->D, N = d->N_model, ne = f.ne;
    const bool sh = d->disc == VA_DISC_SIMPSON_HERMITE;
    if (!tile4_ok(D) || ne <= 0) return false;
    // K is the run length that gives
    // every CU the same number of workgroups when the grid is only a few per CU (C3: 64 seeds,
    // N = 1000: K = 7 -> 12 tiles x 64 = 768 = 3 x 256), 6 otherwise
    const int RW = 64 / D, rows1 = 4 * RW;
    int K = 6;
    auto ntl = [&](int k) { return (long)d->batch * ((N + rows1 * k - 1) / (rows1 * k)); };
    if (ntl(K) < 256) K = 4;
    else if (ntl(K) >= 8 * 256) {
        // many rounds of workgroups: the run length that stages the fewest rows (own + halo) per seed,
        // longest on ties, up to 7 (8 drops the kernel to two waves per SIMD).  N = 1000, D = 20: K = 7
        // (12 tiles x 9 rows per lane against 14 x 8 for K = 6): 370 vs 409 us at 4096 seeds
        long best = -1;
        for (int k = 5; k <= 7; ++k) {
            if (sh && (k & 1)) continue;
            const long cost = (long)((N + rows1 * k - 1) / (rows1 * k)) * (k + (sh ? 3 : 2));
            if (best < 0 || cost <= best) { best = cost; K = k; }
        }
    } else {
        // a few workgroups per CU, all resident at once: the busiest CU sets the time.  Pick the K whose (workgroups per
        // CU, rounded up) x (rows per lane + fixed per-workgroup cost) is smallest, e.g. C3 (64 seeds, N = 1000):
        // K = 7 gives 12 tiles x 64 = 768 workgroups = exactly 3 per CU.  Simpson-Hermite (even K; 8 runs at two waves
        // per SIMD, so only two workgroups per CU are resident): rounds of resident workgroups x rows per lane --
        // N = 1001: K = 4 -> 2 rounds x 6 rows (11.4 us) against 2 x 8 at K = 6 (11.7) and 2 x 10 at K = 8 (12.1)
        K = fewest_rounds_run(d, rows1, sh ? 4 : 5, sh, [&](int k) { return sh ? 256L * (k <= 7 ? 3 : 2) : 256L; });
        // Simpson-Hermite, D = 20, scalar weights: runs of 12 rows (two workgroups per CU, no spill) when they put the whole
        // grid in ONE round of resident workgroups -- a launch of this size is a chain of latencies, not of rows: N = 1001,
        // 64 seeds: K = 4 -> 21 tiles, 1.75 rounds, 11.3 us; K = 12 -> 7 tiles, 448 workgroups, 9.4 us (trapezoid at K = 7: 8.6)
        // (measured for the built-in right-hand side: a generated model keeps the chooser's K unless asked)
        if (sh && D == 20 && d->rhs == VA_RHS_LORENZ96 && d->rm_kind == 0 && d->rf_kind == 0 && ntl(12) <= 2 * 256 && ntl(K) > 3 * 256) K = 12;
    }
    if (d->tile_rows > 0) {
        K = (d->tile_rows + rows1 - 1) / rows1;
        const bool k12 = D == 20 && d->rm_kind == 0 && d->rf_kind == 0 && (d->merr_nskip == 1 || d->rhs == VA_RHS_LORENZ96);     // (the one longer run compiled)
        K = K < 4 ? 4 : (K >= 12 && k12 ? 12 : (K > 8 ? 8 : K));
        if (sh && (K & 1)) ++K;
    }
    // weight arrays / data every nskip-th row: runs of 6 and 7 rows do not fit three waves per SIMD's 168 registers
    // with their weight registers (35-58 spilled; measured at the C3 shape, profiles/r03_f3_variants.txt: 21 us
    // against 13 us for K = 5): those problems run K <= 5, or 8 at two waves per SIMD -- except the built-in
    // right-hand side at D = 20, whose instantiations park the RF weights in LDS, fold the RM weights into the data
    // registers before the f evaluations (va_tile4.h) and mask merr_nskip's rows by a bit each
    {
        const bool ws4 = (d->rm_kind == 0 && d->rf_kind == 0 && d->merr_nskip == 1) || (D == 20 && d->rhs == VA_RHS_LORENZ96);
        if (!ws4 && (K == 6 || K == 7)) K = sh ? 4 : 5;
    }
    // column forms with many products per element (a ring of coupled units: 8): the product arrays grow with the run
    // length; keep at least two workgroups per CU (measured, five 4-state units at the C3 shape: K = 4 23.4 us, K = 7 31.5)
    if (d->tile_rows <= 0) {
        while (K > 4) {
            const Geo4 gt = sh ? tile4_geo<3>(D, K, ne, 1) : tile4_geo<2>(D, K, ne, 1);
            if (sizeof(double) * (size_t)gt.NW * gt.WAVE <= 80 * 1024) break;
            K = shorter_run(K, sh);
        }
    }
    // (one wave per SIMD walking SUB sub-tiles in turn was measured slower than co-resident waves -- DESIGN.md section 7;
    // only SUB = 1 is instantiated, and the host never asks for anything else)
    const int SUB = 1;
    const Geo4 g4 = sh ? tile4_geo<3>(D, K, ne, SUB) : tile4_geo<2>(D, K, ne, SUB);
    // (D = 20 is compiled with its geometry constant: the kernel sizes its staging loop exactly)
    // (no width tile4_ok admits fails this at a run length chosen above -- every even D with K = 4..8, and D = 20 up to
    // 12, was tried; the test stays because the kernel's piece arithmetic is wrong without it)
    if (!((D == 20 || (g4.XP + 63) / 64 <= T4_NI_MAX) && tile4_magic_ok(g4))) return false;
    p.g4 = g4;
    p.emode = 4; p.RY = 4 * RW; p.NT = 256; p.maxr = K; p.T = g4.T;
    p.ntiles = (N + p.T - 1) / p.T;
    p.wg4 = plan_eval4_groups(d->batch, p.ntiles, K, f.nb, g4);
    return true;
}

// column-run kernel: T = RY*K exactly, K rows per lane in {4, 6, 8}; a ghosted form, a lane per column
inline bool plan_eval3(const va_problem_desc *d, const EvalForm &f, EvalPlan &p)
{
    const int D = d->D, N = d->N_model;
    const bool sh = d->disc == VA_DISC_SIMPSON_HERMITE;
    const int HLR = sh ? 3 : 2;
    if (f.ghost <= 0 || D > 1024) return false;           // column runs: a lane per column
    const int RY = tile3_RY(D), NT = tile3_threads(D);
    // K = 6 keeps the kernel at 128 VGPRs (4 waves/SIMD) and measured best from 64 to 4096
    // seeds (profiles/r01_sweep_*.txt); drop to 4 when that leaves CUs without a workgroup
    int K = 6;
    if ((long)d->batch * ((N + RY * K - 1) / (RY * K)) < 256) K = 4;
    else if ((long)d->batch * ((N + RY * K - 1) / (RY * K)) < 8 * 256 && NT == 256) {
        // small grids run as a handful of workgroups per CU, all resident at once: the busiest
        // CU sets the time.  Pick the K whose (workgroups per CU, rounded up) x (rows per lane +
        // fixed per-workgroup cost) is smallest, e.g. C3 (64 seeds, N = 1000): K = 7 gives
        // 12 tiles x 64 = 768 workgroups = exactly 3 per CU (10.2 us) against 3.5 for K = 6 (10.7 us).
        K = fewest_rounds_run(d, RY, 5, sh, [](int) { return 256L; });
    }
    if (d->tile_rows > 0) {
        K = (d->tile_rows + RY - 1) / RY;
        K = K < 4 ? 4 : (K > 8 ? 8 : K);
        if (sh && (K & 1)) ++K;
    }
    if (D > 64 && d->tile_rows <= 0 && (long)d->batch * ((N + RY * 8 - 1) / (RY * 8)) >= 256)
        K = 8;                                         // few lanes per column: long runs keep the halo share down
    if (NT == 1024 && K > 6) K = 6;                    // (1024-thread groups live on 128 registers: runs of 8 rows spill 20-88 of them)
    for (;;) {                                        // shrink until the staging arrays fit in LDS
        const size_t elems = (size_t)tile3_stage_elems(K, D, f.ghost, RY, HLR) + tile3_s_elems(K, D, f.ghost, RY);
        if (sizeof(double) * elems <= (D <= 64 ? 60 : (D <= 512 ? 78 : 150)) * 1024 || K <= 4) break;   // two groups per CU (one beyond D = 512)
        K = shorter_run(K, sh);
    }
    p.emode = 3; p.RY = RY; p.NT = NT; p.maxr = K; p.T = RY * K;
    p.ntiles = (N + p.T - 1) / p.T;
    return true;
}

// flat mapping: every model, every problem
inline void plan_flat(const va_problem_desc *d, const EvalForm &f, EvalPlan &p)
{
    const int D = d->D, N = d->N_model;
    const bool sh = d->disc == VA_DISC_SIMPSON_HERMITE;
    const int HLR = sh ? 3 : 2;
    // LDS: 3 staged arrays of (T+halo) rows (4 when the right-hand side has a dense linear part: J^T s of it)
    // ~24 KiB per workgroup (six per CU) measured best (D = 100: T = 8, 349 us against 403 us at
    // T = 18); wider states take 48 KiB, then whatever still gives two owned rows
    const size_t narr = 3 + (f.lin ? 1 : 0);
    auto rows_in = [&](size_t kib) { return (int)((kib * 1024) / (narr * sizeof(double) * D)) - HLR; };
    int tmax = rows_in(24);
    if (f.lin) {
        // the matrix cores take 16 staged rows at a time and every workgroup reads the whole table of the linear
        // part per product: the smallest budget that stages >= 16 rows, up to 80 KiB (two workgroups per CU)
        for (size_t kib : {24, 48, 80}) { tmax = rows_in(kib); if (tmax + HLR >= 16) break; }
    }
    if (tmax < 2) tmax = rows_in(48);
    if (tmax < 2) tmax = rows_in(150);
    if (f.lin && d->tile_rows > tmax && d->tile_rows <= rows_in(150)) tmax = d->tile_rows;     // (an explicit run length may take the CU's whole LDS)
    int tmin = (EVAL_THREADS + D - 1) / D;               // >= one element per lane
    if (tmax < 2) tmax = 2;
    if (tmin > tmax) tmin = tmax;
    int T;
    if (d->tile_rows > 0) T = d->tile_rows < tmax ? d->tile_rows : tmax;
    else {
        // enough workgroups to cover 256 CUs a few times over
        int want = (1024 + d->batch - 1) / d->batch;     // tiles per seed
        T = N / (want > 0 ? want : 1);
        if (T < tmin) T = tmin;
        if (T > tmax) T = tmax;
    }
    if (T > N) T = N;
    if (sh && (T & 1)) T += (T + 1 <= tmax) ? 1 : -1;
    if (T < 2) T = 2;
    p.emode = 1; p.RY = 0; p.NT = EVAL_THREADS; p.maxr = 0; p.T = T;
    p.ntiles = (N + T - 1) / T;
}

// Tile geometry of the eval kernel: which mapping, rows per workgroup, threads.
inline EvalPlan plan_eval(const va_problem_desc *d, const EvalForm &f)
{
    EvalPlan p;
    p.ghost = f.ghost > 0 ? f.ghost : 2;
    // no column form (or a case only the flat kernel carries)
    if ((f.ne <= 0 && f.ghost <= 0) || flat_only_reason(d)) { plan_flat(d, f, p); return p; }
    int want = d->eval_kernel;
    if (want == 2) want = 3;                              // (the row-strided kernel of round 1 is gone)
    if (want == 5) { if (plan_eval5(d, f, p)) return p; want = 0; }      // (refused: as if no kernel had been asked for)
    if (want < 1 || want > 5) {
        // auto: wave-private column runs for narrow states that fill a wave, streaming strips for the wide even states
        // that can run them, workgroup column runs up to 1024 columns, flat mapping beyond
        if (tile4_ok(d->D) && f.ne > 0) want = 4;
        else if (plan_eval5(d, f, p)) return p;
        else want = 3;
    }
    // a column-run kernel that refuses the problem hands it to the workgroup column runs, those to the flat mapping
    if (want == 4 && plan_eval4(d, f, p)) return p;
    if (want >= 3 && plan_eval3(d, f, p)) return p;
    plan_flat(d, f, p);
    return p;
}

// The column-run instantiation a plan calls for: what a generated module is compiled for (va_eval_plan) and what the
// module a problem comes with is compared against (va_problem_create).  W: kernel 4 -- 1 for scalar weights with data
// at every model time; kernel 3 -- threads per workgroup.  All zero: the flat kernel.
struct VariantKey {
    int kernel = 0, disc = 0, K = 0, W = 0;
    bool operator==(const VariantKey &o) const { return kernel == o.kernel && disc == o.disc && K == o.K && W == o.W; }
};
inline VariantKey variant_key(const EvalPlan &p, const va_problem_desc *d)
{
    VariantKey k;
    if (p.emode != 3 && p.emode != 4 && p.emode != 5) return k;
    k.kernel = p.emode; k.disc = d->disc;
    if (p.emode == 5) return k;                           // (k_eval5 takes neither a run length nor a weight switch)
    k.K = p.maxr;
    k.W = p.emode == 4 ? ((d->rm_kind == 0 && d->rf_kind == 0 && d->merr_nskip == 1) ? 1 : 0) : p.NT;
    return k;
}

// The one column-run instantiation a generated module carries besides its flat kernel, decoded from the integers its
// va_user_variant_info writes (UV_*, va_core.h).
struct ModuleVariant {
    int kernel = 0, disc = 0, K = 0, W = 0;      // eval kernel 3 / 4 / 5, or 0: the module has the flat kernel only
    int ne = 0, ghost = 0, reach[4] = {0, 0, 0, 0};
    int has_linear = 0;                          // the flat kernel carries a dense linear part
    int n_colp_vectors = 0;                      // > 0: the instantiation is of the model's column-parameter form (RhsUserColP)
    int nb = 0;                                  // kernel 4: neighbour columns of the column form (va_user_col_neighbours; 0: a module without it)

    static ModuleVariant decode(const int *v)
    {
        ModuleVariant m;
        m.kernel = v[UV_KERNEL]; m.disc = v[UV_DISC]; m.K = v[UV_K]; m.W = v[UV_W];
        m.ne = v[UV_NE]; m.ghost = v[UV_GHOST];
        for (int k = 0; k < 4; ++k) m.reach[k] = v[UV_REACH + k];
        m.has_linear = v[UV_LINEAR] ? 1 : 0; m.n_colp_vectors = v[UV_NCV];
        return m;
    }
    bool column_params() const { return n_colp_vectors > 0 && (kernel == 4 || kernel == 5); }
    EvalForm flat_form() const { EvalForm f; f.lin = has_linear; return f; }
    EvalForm form() const
    {
        EvalForm f = flat_form();
        f.ne = (kernel == 4 || kernel == 5) ? ne : 0;
        f.nb = kernel == 4 ? nb : 0;
        f.ghost = kernel == 3 ? ghost : 0;
        f.has_reach5 = kernel == 5;
        for (int k = 0; k < 4; ++k) f.reach5[k] = reach[k];
        return f;
    }
    // (as variant_key forms it: k_eval5's instantiation depends on neither K nor W, k_eval4's on W != 0 alone)
    VariantKey key() const
    {
        VariantKey k;
        k.kernel = kernel; k.disc = disc;
        if (kernel == 5) return k;
        k.K = K; k.W = kernel == 4 ? (W != 0 ? 1 : 0) : W;
        return k;
    }
};

}  // namespace va
