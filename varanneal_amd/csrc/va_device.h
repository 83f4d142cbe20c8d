// va_device.h -- device-side problem image shared by va_kernels.hip and va_capi.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "va_core.h"
#include "va_tile2.h"
#include "va_tile3.h"
#include "va_tile4.h"
#include "va_tile5.h"

namespace va {

constexpr int VEC_THREADS = 256;
constexpr int VEC_CHUNK = 1024;      // elements of a seed's vector per workgroup (2 x double2 per lane)

// Arrival counters sit one per 256-byte line: returning atomics on words of one line serialise
// (~10 ns each: 3072 arrivals on 64 adjacent words cost 25 us), on different lines they do not.
constexpr int CNT_STRIDE = 64;

// what the last-arriving wave of an evaluation does with the seed's partial sums (va_epilogue.h)
enum { EPI_NONE = 0, EPI_FINALIZE = 1, EPI_LS = 2 };

// The persistent per-seed kernel's exchange area (va_persist.h): G workgroups per seed
struct Persist {
    unsigned long long *xch;          // [B][2 buffers][G rows][granule pairs of 16 bytes]: one row per workgroup and cycle
    unsigned long long *cycles;       // cycles run by the last launch (summed over seeds)
    int *abort_flag;                  // 0; 1 a poll timed out (workgroups not co-resident); 2 cycle budget exceeded
    double *stamps;                   // measurement builds (-DVA_PZ_STAMPS) leave their per-phase tick sums here
    long long max_cycles;
};

// Everything a kernel needs, passed by value as the kernel argument.
struct Dev {
    Dims dm;
    Geo4 g4;                       // wave-private column-run geometry (emode 4)
    Geo5 g5;                       // streaming column-strip geometry (emode 5)
    const int *ystrip;             // [NS][2] per strip: first data column staged (even), 16-byte pieces per observation row
    int lsrun;                     // this launch may hold line-search points (seeds in PH_LS): stage d as well
    int epi;                       // EPI_*: tail folded into the evaluation kernel
    unsigned nwg_magic;            // k_eval4: floor(w / nwg) == umulhi(w, nwg_magic) for w < B*nwg, nwg = eval4_nwg(dv) workgroups per seed
    int gaux;                      // 1: gradient stores write through (sc1)
    int wg4;                       // k_eval4: row groups (of 4 waves, Geo4::T rows) per workgroup, 1 .. 3 (0 reads as 1)
    int sticky;                    // measurement only (va_lbfgs_timed): last arrivers leave upd / dir set
    int evcols;                    // 8, 16 or 32 >= EP_GP + NP: columns of the eval partial rows in use
    ProblemPtrs pp;
    Opts o;
    // per-seed vectors, stride dm.ld (multiple of 16 doubles -> 128-byte aligned rows)
    double *x, *g, *gt, *d;
    double *S, *Y;                 // [B][m][ld]
    SeedState *st;                 // [B]
    double *evp;                   // [B][ntiles][EP_N]       eval partials
    double *evp_big;               // NULL or [B][ntiles][npbig]: parameter-gradient partials of parameters RHS_MAX_NP, RHS_MAX_NP + 1, ... (flat kernel)
    int npbig;                     // = NP - RHS_MAX_NP when positive
    double *upp;                   // [B][nchunks][ups]       update-kernel dot partials
    double *dpp;                   // [B][nchunks][DP_N]      direction partials
    int ups;                       // = UP_OLD + 4*m
    // ladder + results (device copies; host reads them back once at the end)
    const double *rf_ladder;       // [nbeta]
    int nbeta, max_beta;
    double *ame;                   // [B][max_beta][3]
    double *pest;                  // [B][max_beta][NPest]
    int *status, *nit;             // [B][max_beta]
    long long *nfev;               // [B][max_beta]
    double *minpaths;              // NULL or [B][max_beta][ND+NP]
    int *n_active;
    unsigned *cnt_eval, *cnt_upd, *cnt_dir;   // [B][CNT_STRIDE] arrival counters of the three kernels of a cycle (zero between launches)
    unsigned long long *n_evals;   // seed-evaluations consumed by k_ls since create
    // S1 outputs
    double *outA, *outme, *outfe;  // [B]
    // bounded problems (va_lbfgsb.hip): Cauchy point / subspace minimiser z, reduced gradient r, the copy xp,
    // breakpoints t, variable status iwhere ([B][ld] each); S'Y, S'S, T ([B][3 m m]); d'd of the direction in use ([B])
    double *lb_z, *lb_r, *lb_xp, *lb_t, *lb_mat, *lb_dtd;
    int *lb_iwhere;
    Persist pz;
    // (last: the fields above keep their kernel-argument offsets)
    // column-parameter form on k_eval4 / k_eval5 (a module's RhsUserColP; 0 / NULL otherwise): cps shared scalars and
    // cpv = NCV * D vector entries.  cpmap [2][cps + cpv]: the global parameter index of each, then its index in p_est
    // or -1 (fixed); evv [B][ntiles][cpv]: the vector entries' gradient partials per workgroup; cpnsg: k_eval5's
    // workgroups per row of strips (only those of a column's strip hold its partials), 0 for k_eval4
    const int *cpmap;
    double *evv;
    int cps, cpv, cpnsg;
    // >= 0: this launch is an S1 evaluation -- the host has put EVERY seed in PH_START at this rf_scale (launch_init_states),
    // so the kernel and its tail take phase and RF from here and read nothing of the seeds' states.  Negative: read them.
    // Set by run_eval alone (va_capi.hip), from the RF the caller armed the seeds with; never inferred from lsrun.
    double s1_rf;
};

// ------------------------------------------------------------------ one prepare-or-launch operation
// Every evaluation kernel is reached through eval_op: a family names its instantiation ONCE and hands it here, so the
// kernel that is opted in to its LDS (once per handle and device) cannot differ from the one that is launched.
struct EvalOp { bool prepare; hipStream_t s; hipError_t err; };

constexpr size_t LDS_DEFAULT_BYTES = 64 * 1024, LDS_OPTIN_BYTES = 160 * 1024;      // without / with the opt-in: a CU's whole LDS

// (a multiple of 8: xcd_swizzle deals the workgroups over the 8 XCDs)
inline int eval_grid(int nwork) { return ((nwork + 7) / 8) * 8; }
inline int eval_grid(const Dims &dm) { return eval_grid(dm.B * dm.ntiles); }

// k_eval4's two counts: dm.ntiles (= dm.nprow) is the seed's ROW GROUPS -- the 4-wave units of Geo4::T rows that each own a
// row of the partial tables, what the epilogue reduces over -- and a workgroup runs wg4 consecutive ones, so the grid,
// the decoding of blockIdx and the arrival count go by the seed's WORKGROUPS
VA_HD int eval4_groups(const Dev &dv) { return dv.wg4 > 1 ? dv.wg4 : 1; }
VA_HD int eval4_nwg(const Dev &dv) { return (dv.dm.ntiles + eval4_groups(dv) - 1) / eval4_groups(dv); }

// (grid < 0: one workgroup per tile, eval_grid(dv.dm))
template <class KERNEL>
inline void eval_op(KERNEL kern, const Dev &dv, int threads, size_t lds, EvalOp &op, int grid = -1)
{
    if (op.prepare) {
        if (lds <= LDS_DEFAULT_BYTES) return;
        const hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_OPTIN_BYTES);
        if (e != hipSuccess) op.err = e;
        return;
    }
    hipLaunchKernelGGL(kern, dim3(grid < 0 ? eval_grid(dv.dm) : grid), dim3(threads), lds, op.s, dv);
}

// the run-time discretisation as a compile-time constant: f(std::integral_constant<int, DISC_*>)
template <class F>
inline void with_disc(int disc, F &&f)
{
    switch (disc) {
    case DISC_EULER: f(std::integral_constant<int, DISC_EULER>()); break;
    case DISC_TRAPEZOID: f(std::integral_constant<int, DISC_TRAPEZOID>()); break;
    case DISC_SH: f(std::integral_constant<int, DISC_SH>()); break;
    default: f(std::integral_constant<int, DISC_FWDMAP>()); break;
    }
}

// ------------------------------------------------------------------ one entry table per right-hand side
// Everything the host launches that depends on the right-hand side.  The built-in Lorenz-96 fills one in va_kernels.hip
// (builtin_rhs_table); a generated module fills one through its only entry point, va_user_rhs_table (va_user_rhs.hip).
struct PredictArgs;
struct HvpArgs;
struct RhsTable {
    int bytes;                                 // sizeof(RhsTable), then the sizes of what crosses the boundary by value or by layout
    int dev_bytes, seed_bytes, predict_bytes;
    int NP, D, NSTIM;
    void (*eval)(const Dev &, EvalOp &);       // the flat kernel (a module), the kernel dv.dm.emode names (built-in); a handle's copy: ITS kernel
    void (*eval_var)(const Dev &, EvalOp &);   // a module's ONE carried column-run instantiation (va_user_variant_info describes it), or NULL
    void (*seed)(const Dev &, EvalOp &);       // the persistent per-seed ladder kernel k_seed (va_persist.h), or NULL
    hipError_t (*predict)(const PredictArgs &, hipStream_t);      // the RK4 predictor (va_predict.h), or NULL
};
void builtin_rhs_table(RhsTable &t);
// The launcher slots of the kernels that call the right-hand side's derivatives along a direction (RHS::jvp and beyond): the
// Hessian-vector kernel (va_hvp.h), the tangent-linear predictor (va_predict_tlm.h), the predictor's entry beside
// `predict`, and the Lyapunov-spectrum kernel (va_lyap.h); and, because this is where new launchers go while RhsTable's layout
// stays fixed, the ensemble Kalman filter (va_enkf.h), which calls RHS::f alone.  A table of its own beside RhsTable, whose layout modules and their checks already agree on: the built-in
// fills one in va_kernels.hip (builtin_hvp_table), a generated module through a second entry point, va_user_hvp_table
// (va_user_rhs.hip); a module without that entry point has no such kernels.
struct PredictTlmArgs;
struct LyapArgs;
struct PredictAdjArgs;
struct ShootArgs;
struct EnkfArgs;
struct ShootBoxArgs;
struct HvpTable {
    int bytes, hvp_bytes, tlm_bytes, lyap_bytes;      // sizeof(HvpTable), sizeof(HvpArgs), sizeof(PredictTlmArgs), sizeof(LyapArgs)
    int adj_bytes;                                    // sizeof(PredictAdjArgs)
    int shoot_bytes;                                  // sizeof(ShootArgs)
    int enkf_bytes;                                   // sizeof(EnkfArgs)
    int shoot_box_bytes;                              // sizeof(ShootBoxArgs)
    hipError_t (*hvp)(const HvpArgs &, size_t lds_bytes, hipStream_t);      // or NULL
    hipError_t (*predict_tlm)(const PredictTlmArgs &, hipStream_t);         // or NULL
    hipError_t (*lyap)(const LyapArgs &, hipStream_t);                      // or NULL
    hipError_t (*predict_adj)(const PredictAdjArgs &, hipStream_t);         // the adjoint predictor (va_predict_adj.h), or NULL
    hipError_t (*shoot)(const ShootArgs &, hipStream_t);                    // the shooting kernel (va_shoot.h), or NULL
    hipError_t (*enkf)(const EnkfArgs &, hipStream_t);                      // the ensemble Kalman filter (va_enkf.h), or NULL
    hipError_t (*shoot_box)(const ShootBoxArgs &, hipStream_t);             // the boxed shooting kernel (va_shoot_box.h), or NULL
};
void builtin_hvp_table(HvpTable &t);

// launch wrappers (va_kernels.hip); all asynchronous on `s`
void launch_ls(const Dev &dv, hipStream_t s);
void launch_update(const Dev &dv, hipStream_t s);
void launch_direction(const Dev &dv, hipStream_t s);
void launch_init_states(const Dev &dv, int phase, double rf_scale_or_neg, hipStream_t s);
void launch_arm_full_history(const Dev &dv, hipStream_t s);
void launch_arm_ls(const Dev &dv, double rf, hipStream_t s);
void launch_clamp_x(const Dev &dv, hipStream_t s);
void launch_finalize_eval(const Dev &dv, hipStream_t s);
size_t eval_lds_bytes(const Dev &dv);
size_t update_lds_bytes(const Dims &dm);
// bounded problems: L-BFGS-B's direction step in k_direction's place (va_lbfgsb.hip)
void launch_lbfgsb_dir(const Dev &dv, hipStream_t s);
hipError_t prepare_lbfgsb(const Dev &dv);
// the built-in right-hand side on k_eval4's wider workgroups (va_eval4_g2.hip, va_eval4_g3.hip)
void eval4_builtin_g2(const Dev &dv, EvalOp &op);
void eval4_builtin_g3(const Dev &dv, EvalOp &op);
// streaming column strips for the built-in right-hand side (va_eval5.hip)
void eval5_builtin(const Dev &dv, EvalOp &op);
size_t eval5_lds(const Dev &dv);

}  // namespace va
