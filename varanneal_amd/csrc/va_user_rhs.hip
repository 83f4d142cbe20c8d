// va_user_rhs.hip -- translation unit of a GENERATED right-hand-side module.
//
// varanneal_amd/codegen.py traces the user's `f(t, x, p)` (the callable of set_model,
// varanneal/va_ode.py:56-67), differentiates it symbolically and writes a header that
// defines `struct RhsUser` with f, J^T v and (df/dp)^T v.  This file instantiates the
// flat-mapped tile kernel for it; it is compiled with
//     hipcc --offload-arch=gfx950 -shared -DVA_USER_RHS_HEADER='"<header>"' va_user_rhs.hip
// and registered through va_rhs_load_module().  The reference replays an ADOL-C tape of f
// instead (_autodiffmin.py:32-58).
#include "va_eval_flat.h"
#include "va_eval3.h"
#include "va_eval4.h"
#include "va_eval5.h"
#include "va_persist.h"
#include "va_predict.h"

#ifndef VA_USER_RHS_HEADER
#error "compile with -DVA_USER_RHS_HEADER='\"path/to/generated_header.h\"'"
#endif
#include VA_USER_RHS_HEADER

namespace {
// A model of more than RHS_BIG_NP parameters has no flat struct (RhsUser::FLAT = false): nothing of the flat kernel or of
// k_seed is instantiated, and the host never asks for them (va_problem_create refuses such problems on any other kernel)
template <class R> void user_launch_eval(const va::Dev &dv, hipStream_t s)
{
    if constexpr (va::rhs_flat<R>::value) va::launch_eval_rhs<R>(dv, s);
    else { (void)dv; (void)s; }
}
template <class R> hipError_t user_prepare_eval(const va::Dev &dv)
{
    if constexpr (va::rhs_flat<R>::value) return va::prepare_eval_rhs<R>(dv);
    else { (void)dv; return hipErrorNotSupported; }
}
}  // namespace

extern "C" {

// (NP, D, NSTIM, sizeof(Dev), sizeof(SeedState)) -- checked by va_rhs_load_module
void va_user_rhs_info(int *out)
{
    out[0] = va::RhsUser::NP; out[1] = va::RhsUser::D; out[2] = va::RhsUser::NSTIM;
    out[3] = (int)sizeof(va::Dev); out[4] = (int)sizeof(va::SeedState);
}

void va_user_launch_eval(const va::Dev *dv, void *stream)
{
    user_launch_eval<va::RhsUser>(*dv, (hipStream_t)stream);
}

// once per problem handle, on the handle's device: opt the kernel in to the LDS it needs
int va_user_prepare_eval(const va::Dev *dv)
{
    return (int)user_prepare_eval<va::RhsUser>(*dv);
}

// the persistent per-seed ladder kernel (va_persist.h) for this model: few seeds, short paths
int va_user_seed_kernel(const va::Dev *dv, int launch, void *stream)
{
    return (int)va::seed_kernel_op<va::RhsUser>(*dv, launch != 0, (hipStream_t)stream);
}

// the RK4 predictor (va_predict.h) for this model: only a module with a flat struct (the generator says so: VA_USER_FLAT)
// has the f(x_row, i, ...) the integrator calls.  args_bytes: sizeof(PredictArgs) as the caller knows it
#ifdef VA_USER_FLAT
int va_user_predict(const va::PredictArgs *a, int args_bytes, void *stream)
{
    if (args_bytes != (int)sizeof(va::PredictArgs)) return (int)hipErrorInvalidValue;
    return (int)va::launch_predict<va::RhsUser, va::RhsUser::D>(*a, (hipStream_t)stream);
}
#endif

// Besides the flat kernel a module may carry ONE instantiation of a column-run kernel, named when the module
// was generated (va_eval_plan; -DVA_USER_EK=3|4 -DVA_USER_DISC -DVA_USER_K -DVA_USER_W):
//   EK = 4: the model's column form (struct RhsUserCol: a translation-invariant stencil, or a small dense
//           system) on the wave-private kernel k_eval4; W = 1 for scalar weights
//   EK = 5: a stencil's column form on the streaming kernel k_eval5 (wide even states, autonomous)
//   EK = 3: a stencil's ghosted form (struct RhsUserG) on the workgroup kernel k_eval3; W = threads per workgroup
// A model in column-parameter form (struct RhsUserColP: a stencil with per-column parameter vectors) takes the place of
// the column form for EK = 4 and 5.
// (the integers are named in va_core.h: UV_*)
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
#if defined(VA_USER_VARIANT) && VA_USER_VARIANT == 5
void va_user_launch_variant(const va::Dev *dv, void *stream)
{
    (void)va::eval5_run<VA_USER_COLT, VA_USER_DISC, VA_USER_COLT::D>(*dv, false, (hipStream_t)stream);
}
int va_user_prepare_variant(const va::Dev *dv)
{
    return (int)va::eval5_run<VA_USER_COLT, VA_USER_DISC, VA_USER_COLT::D>(*dv, true, nullptr);
}
#elif defined(VA_USER_VARIANT) && VA_USER_VARIANT == 4
void va_user_launch_variant(const va::Dev *dv, void *stream)
{
    va::launch_eval4_one<VA_USER_COLT, VA_USER_DISC, VA_USER_K, VA_USER_COLT::D, VA_USER_W != 0>(*dv, (hipStream_t)stream);
}
int va_user_prepare_variant(const va::Dev *dv)
{
    return (int)va::prepare_eval4_one<VA_USER_COLT, VA_USER_DISC, VA_USER_K, VA_USER_COLT::D, VA_USER_W != 0>(*dv);
}
#elif defined(VA_USER_VARIANT)
void va_user_launch_variant(const va::Dev *dv, void *stream)
{
    va::launch_eval3_one<va::RhsUserG, VA_USER_DISC, VA_USER_K, va::RhsUserG::D, VA_USER_W>(*dv, (hipStream_t)stream);     // (D compiled in, as the built-in's D = 200)
}
int va_user_prepare_variant(const va::Dev *dv)
{
    return (int)va::prepare_eval3_one<va::RhsUserG, VA_USER_DISC, VA_USER_K, va::RhsUserG::D, VA_USER_W>(*dv);
}
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
