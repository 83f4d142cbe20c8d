// va_user_rhs.hip -- translation unit of a GENERATED right-hand-side module.
//
// varanneal_amd/codegen.py traces the user's `f(t, x, p)` (the callable of set_model,
// varanneal/va_ode.py:56-67), differentiates it symbolically and writes a header that
// defines `struct RhsUser` with f, J^T v and (df/dp)^T v.  This file instantiates the model's
// kernels -- the flat-mapped tile kernel, the persistent ladder kernel, the RK4 predictor, its tangent-linear model and the Lyapunov-spectrum kernel, the Hessian-vector kernel and at most
// ONE column-run kernel -- and exports the entry point va_user_rhs_table, which fills the table of
// launchers (RhsTable, va_device.h) the host reaches them through, va_user_hvp_table for the launchers of the Hessian-vector
// kernel and the tangent-linear predictor (HvpTable); two more functions return data
// (va_user_variant_info, va_user_colp_map).  It is compiled with
//     hipcc --offload-arch=gfx950 -shared -DVA_USER_RHS_HEADER='"<header>"' va_user_rhs.hip
// and registered through va_rhs_load_module().  The reference replays an ADOL-C tape of f
// instead (_autodiffmin.py:32-58).
#include "va_eval_flat.h"
#include "va_eval3.h"
#include "va_eval4.h"
#include "va_eval5.h"
#include "va_persist.h"
#include "va_predict.h"
#include "va_predict_tlm.h"
#include "va_predict_adj.h"
#include "va_shoot.h"
#include "va_shoot_box.h"
#include "va_lyap.h"
#include "va_enkf.h"
#include "va_hvp.h"

#ifndef VA_USER_RHS_HEADER
#error "compile with -DVA_USER_RHS_HEADER='\"path/to/generated_header.h\"'"
#endif
#include VA_USER_RHS_HEADER

namespace {
// Besides the flat kernel a module may carry ONE instantiation of a column-run kernel, named when the module
// was generated (va_eval_plan; -DVA_USER_EK=3|4 -DVA_USER_DISC -DVA_USER_K -DVA_USER_W):
//   EK = 4: the model's column form (struct RhsUserCol: a translation-invariant stencil, or a small dense
//           system) on the wave-private kernel k_eval4; W = 1 for scalar weights
//   EK = 5: a stencil's column form on the streaming kernel k_eval5 (wide even states, autonomous)
//   EK = 3: a stencil's ghosted form (struct RhsUserG) on the workgroup kernel k_eval3; W = threads per workgroup
// A model in column-parameter form (struct RhsUserColP: a stencil with per-column parameter vectors) takes the place of
// the column form for EK = 4 and 5.
#if defined(VA_USER_COLP)
#define VA_USER_COLT va::RhsUserColP
#elif defined(VA_USER_COL)
#define VA_USER_COLT va::RhsUserCol
#endif
#if defined(VA_USER_EK) && VA_USER_EK == 5 && defined(VA_USER_COLT)
#define VA_USER_VARIANT 5
#elif defined(VA_USER_EK) && VA_USER_EK == 4 && defined(VA_USER_COLT)
#define VA_USER_VARIANT 4
#elif defined(VA_USER_EK) && VA_USER_EK == 3 && defined(VA_USER_GHOST)
#define VA_USER_VARIANT 3
#endif
// the carried instantiation, named once
#if !defined(VA_USER_VARIANT)
constexpr void (*user_eval_var)(const va::Dev &, va::EvalOp &) = nullptr;
#elif VA_USER_VARIANT == 5
constexpr auto user_eval_var = va::eval5_op<VA_USER_COLT, VA_USER_DISC, VA_USER_COLT::D>;
#elif VA_USER_VARIANT == 4
constexpr auto user_eval_var = va::eval4_op_groups<VA_USER_COLT, VA_USER_DISC, VA_USER_K, VA_USER_COLT::D, VA_USER_W != 0>;      // (every workgroup width, Dev::wg4)
#else
constexpr auto user_eval_var = va::eval3_op<va::RhsUserG, VA_USER_DISC, VA_USER_K, va::RhsUserG::D, VA_USER_W>;     // (D compiled in, as the built-in's D = 200)
#endif

// A model of more than RHS_BIG_NP parameters has no flat struct (RhsUser::FLAT = false): nothing of the flat kernel, of
// k_seed or of the predictor is instantiated, and the host never asks for them (va_problem_create refuses such problems on
// any other kernel than the carried one, va_predict refuses the handle).  (A template: only there are the branches not
// taken left uninstantiated.)
template <class R> void fill_table(va::RhsTable &t)
{
    t = va::RhsTable{(int)sizeof(va::RhsTable), (int)sizeof(va::Dev), (int)sizeof(va::SeedState), (int)sizeof(va::PredictArgs),
                     R::NP, R::D, R::NSTIM, nullptr, user_eval_var, nullptr, nullptr};
    if constexpr (va::rhs_flat<R>::value) { t.eval = va::eval_flat_op<R>; t.predict = va::launch_predict<R, R::D>; }
    if constexpr (va::seed_kernel_exists<R>()) t.seed = va::seed_op<R>;
}
// the Hessian-vector kernel, the tangent-linear predictor, its adjoint and the Lyapunov-spectrum kernel: derivatives of the element-wise
// part only (a split-off linear part would need products of its own), and only where a flat struct exists.  The ensemble
// Kalman filter calls f alone, through predict_f as the predictor does: a split-off linear part is carried there
template <class R> void fill_hvp_table(va::HvpTable &t)
{
    t = va::HvpTable{(int)sizeof(va::HvpTable), (int)sizeof(va::HvpArgs), (int)sizeof(va::PredictTlmArgs), (int)sizeof(va::LyapArgs),
                     (int)sizeof(va::PredictAdjArgs), (int)sizeof(va::ShootArgs), (int)sizeof(va::EnkfArgs), (int)sizeof(va::ShootBoxArgs), nullptr, nullptr,
                     nullptr, nullptr, nullptr, nullptr, nullptr};
    if constexpr (va::rhs_flat<R>::value) t.enkf = va::launch_enkf<R, R::D>;
    if constexpr (va::rhs_flat<R>::value && !va::rhs_linear<R>::value) {
        t.hvp = va::launch_hvp<R>; t.predict_tlm = va::launch_predict_tlm<R, R::D>;
        t.predict_adj = va::launch_predict_adj<R, R::D>;
        if constexpr (R::D <= va::SHOOT_MAX_D) { t.shoot = va::launch_shoot<R, R::D>; t.shoot_box = va::launch_shoot_box<R, R::D>; }
        if constexpr (R::D <= va::LYAP_MAX_D) t.lyap = va::launch_lyap<R, R::D>;
    }
}
}  // namespace

extern "C" {

// The module's one entry point.  bytes: sizeof(RhsTable) as the caller knows it; returns the module's own, and fills *out
// only when the two agree (va_rhs_load_module checks that, and the sizes of Dev, SeedState and PredictArgs in the table).
int va_user_rhs_table(va::RhsTable *out, int bytes)
{
    if (bytes == (int)sizeof(va::RhsTable)) fill_table<va::RhsUser>(*out);
    return (int)sizeof(va::RhsTable);
}

// The launchers of the Hessian-vector kernel and the tangent-linear predictor, with the same size handshake (HvpTable, va_device.h).
int va_user_hvp_table(va::HvpTable *out, int bytes)
{
    if (bytes == (int)sizeof(va::HvpTable)) fill_hvp_table<va::RhsUser>(*out);
    return (int)sizeof(va::HvpTable);
}

// (the integers are named in va_core.h: UV_*)
void va_user_variant_info(int *out)
{
    for (int k = 0; k < va::UV_N; ++k) out[k] = 0;
    out[va::UV_LINEAR] = va::rhs_linear<va::RhsUser>::value ? 1 : 0;     // the flat kernel stages one more array (va_eval_flat.h lin_gemm)
#ifdef VA_USER_VARIANT
    out[va::UV_KERNEL] = VA_USER_VARIANT; out[va::UV_DISC] = VA_USER_DISC; out[va::UV_K] = VA_USER_K; out[va::UV_W] = VA_USER_W;
#if VA_USER_VARIANT == 5
    out[va::UV_NE] = VA_USER_COLT::NE;
    out[va::UV_REACH] = va::t5_xl<VA_USER_COLT>(); out[va::UV_REACH + 1] = va::t5_xr<VA_USER_COLT>();
    out[va::UV_REACH + 2] = va::t5_gl<VA_USER_COLT>(); out[va::UV_REACH + 3] = va::t5_gr<VA_USER_COLT>();
    out[va::UV_NCV] = va::rhs_ncv<VA_USER_COLT>::value;
#elif VA_USER_VARIANT == 4
    out[va::UV_NE] = VA_USER_COLT::NE;
    out[va::UV_NCV] = va::rhs_ncv<VA_USER_COLT>::value;
#else
    out[va::UV_GHOST] = va::RhsUserG::GHOST;
#endif
#endif
}
#if defined(VA_USER_VARIANT) && VA_USER_VARIANT == 4
// Neighbour columns the carried k_eval4 instantiation's column form reads: with the run length they set the kernel's
// registers, hence how many 4-wave workgroups a CU holds and which workgroup widths exist (eval4_wpc, va_eval4.h).
// (An entry point of its own: va_user_variant_info's integers are counted by its callers.)
int va_user_col_neighbours(void) { return VA_USER_COLT::NB; }
#endif
#if defined(VA_USER_COLP)
// the column-parameter form's map: (shared scalars S, vectors V), then the global parameter index of each shared scalar
// and of each vector entry (v, column i) at S + v D + i
void va_user_colp_map(int *out)
{
    out[0] = va::RhsUserColP::NP; out[1] = va::RhsUserColP::NCV;
    for (int k = 0; k < va::RhsUserColP::NP; ++k) out[2 + k] = va::va_colp_sidx[k];
    for (int e = 0; e < va::RhsUserColP::NCV * va::RhsUserColP::D; ++e) out[2 + va::RhsUserColP::NP + e] = va::va_colp_vidx[e];
}
#endif

}  // extern "C"
