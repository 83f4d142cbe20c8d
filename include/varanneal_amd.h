/* include/varanneal_amd.h -- C-ABI of the MI355X-native variational-annealing
 * hot path (libvaranneal_amd.so, HIP for gfx950).
 *
 * The reference (paulrozdeba/varanneal) has no FFI: its seam is the ADmin
 * mixin that va_ode.Annealer inherits (varanneal/va_ode.py:41,43).  Each entry
 * point below names the reference interface it stands in for; the ctypes
 * binding a maintainer would add is shown in INTEGRATION.md and implemented in
 * varanneal_amd/_capi.py.
 *
 * Conventions
 *   - every function returns VA_OK (0) or a negative VA_E* code; never exits,
 *     never throws (reference: print + sys.exit(1), va_ode.py:622-623,637-638).
 *     va_last_error() returns a thread-local message for the last failure.
 *   - caller owns every pointer it passes; host inputs need only stay valid
 *     for the duration of the call.
 *   - a handle is bound to one device and one HIP stream and is NOT re-entrant;
 *     distinct handles may be used from distinct threads.
 *   - all arithmetic is float64.
 *   - path vectors use the reference's packing (va_ode.py:688-693):
 *         XP[b] = [ X[b] flattened (N_model*D, time-major) | p_est (NPest) ]
 *     `ld` is the stride in doubles between consecutive seeds (>= n_var).
 *     `mem` says where XP/grad/outputs live: host (copied in/out) or device
 *     (used in place, no PCIe traffic).
 */
#ifndef VARANNEAL_AMD_H
#define VARANNEAL_AMD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VA_ABI_VERSION 12

enum { VA_OK = 0, VA_EINVAL = -1, VA_ENOMEM = -2, VA_EHIP = -3, VA_EUNSUPPORTED = -4,
       VA_ESTATE = -5 };

/* discretisations: va_ode.py:341-356 (euler), 358-380 (trapezoid),
 * 404-437 (SimpsonHermite, needs odd N_model), 439-454 (forwardmap) */
enum { VA_DISC_EULER = 0, VA_DISC_TRAPEZOID = 1, VA_DISC_SIMPSON_HERMITE = 2,
       VA_DISC_FORWARDMAP = 3 };

/* right-hand sides (the user `f(t,x,p)` of set_model, va_ode.py:56-67).
 * LORENZ96: built in; examples/Lorenz96_D20/Lorenz96_anneal.py:15-16, NP = 1 (forcing k).
 * ids >= VA_RHS_USER_BASE: generated-code modules registered with va_rhs_load_module
 * (varanneal_amd/codegen.py traces the user's Python callable, emits f, J^T v and
 * (df/dp)^T v as HIP and compiles them for gfx950). */
enum { VA_RHS_LORENZ96 = 0, VA_RHS_USER_BASE = 1000 };

enum { VA_MEM_HOST = 0, VA_MEM_DEVICE = 1 };

typedef struct va_problem_s *va_handle;

/* Everything anneal_init() freezes (va_ode.py:531-705). */
typedef struct va_problem_desc {
    int32_t struct_size;      /* = sizeof(va_problem_desc)                          */
    int32_t device;           /* HIP device ordinal                                  */
    int32_t batch;            /* B: independent initial paths ("seeds") resident     */
    int32_t D;                /* state dimension (set_model)                         */
    int32_t N_model;          /* time points of the path                             */
    int32_t N_data;           /* observation times                                   */
    int32_t merr_nskip;       /* int(dt_data/dt_model), va_ode.py:556                */
    int32_t L;                /* observed components                                 */
    const int32_t *Lidx;      /* [L]                                                 */
    const double *Y;          /* [N_data*L] observations, shared by all seeds        */
    double dt_model;
    int32_t rm_kind;          /* 0: scalar rm;  1: rm_array [N_data*L] (va_ode.py:147-148);
                               * 2: rm_array [N_data*L*L], full precision matrices (va_ode.py:149-152) */
    double rm;
    const double *rm_array;
    int32_t rf_kind;          /* 0: scalar rf0; 1: rf0_array [(N_model-1)*D] (va_ode.py:203-209);
                               * 2: rf0_array [(N_model-1)*D*D] full matrices, diff_n.(RF_n.diff_n) (va_ode.py:211-217) */
    double rf0;
    const double *rf0_array;
    int32_t NP;               /* parameters of the RHS                               */
    int32_t NPest;            /* how many are estimated                              */
    const int32_t *Pidx;      /* [NPest] indices into the parameter vector           */
    const double *P;          /* [B*NP] full parameter vector of every seed          */
    int32_t disc;             /* VA_DISC_*                                           */
    int32_t rhs;              /* VA_RHS_*                                            */
    int32_t lbfgs_m;          /* history pairs kept on device (SciPy maxcor, 10)     */
    int32_t max_beta;         /* longest ladder va_anneal will be asked for (>=1)    */
    int32_t keep_paths;       /* 1: keep every beta step's path on device (minpaths) */
    int32_t tile_rows;        /* 0 = auto; time rows per workgroup                   */
    int32_t eval_kernel;      /* 0 = auto; 1 = flat-mapped, 3 = workgroup column runs, 4 = wave-private column runs,
                               * 5 = streaming column strips (a kernel that does not apply falls back)          */
    const double *t_model;    /* NULL or [N_model]: times passed to a non-autonomous RHS (va_ode.py:553,558) */
    const double *stim;       /* NULL or [N_model*n_stim]: external stimulus rows, f(t,x,(p,stim)) (va_ode.py:345-375) */
    int32_t n_stim;
    int32_t p_time_dependent; /* 1: P is [B][N_model][NP] (P0.ndim == 2 upstream, va_ode.py:170-188); the path
                               * vector is then [X (N_model*D) | p_est (N_model*NPest), time-major],
                               * n_var = N_model*(D+NPest); trapezoid and SimpsonHermite only (upstream's
                               * euler/forwardmap branches slice p one row short, va_ode.py:345-349) */
    void *stream;             /* hipStream_t to run on; NULL = library-owned stream  */
    const double *lower;      /* NULL, or [n_var] box bounds of the path vector [X | p_est] shared by all seeds     */
    const double *upper;      /* (va_ode.py:582-605 expands `bounds` to this order); -/+HUGE_VAL = no bound.        */
                              /* With bounds va_minimize_lbfgs / va_anneal run L-BFGS-B itself on the device: the    */
                              /* direction step is csrc/va_lbfgsb.hip (generalised Cauchy point + subspace            */
                              /* minimisation, one workgroup per seed) in k_direction's place; same line search,     */
                              /* stopping rules on the projected gradient.  Iterates follow SciPy's step for step    */
                              /* (tests/test_gpu_codegen.py::test_bounded_device_minimiser_is_lbfgsb_step_for_step). */
} va_problem_desc;

/* SciPy option names (reference passes opt_args through, _autodiffmin.py:85-86) */
typedef struct va_lbfgs_opts {
    int32_t maxcor;           /* <= desc.lbfgs_m                                     */
    double ftol;              /* (f_k - f_{k+1})/max(|f_k|,|f_{k+1}|,1) <= ftol      */
    double gtol;              /* max|g_i| <= gtol                                    */
    int32_t maxiter;
    int64_t maxfun;
    int32_t maxls;
} va_lbfgs_opts;

int32_t va_abi_version(void);
const char *va_last_error(void);
int va_device_count(int32_t *count);

/* Register a compiled right-hand-side module (a shared object built from
 * varanneal_amd/csrc/va_user_rhs.hip + a generated header); returns its rhs id. */
int va_rhs_load_module(const char *path, int32_t *rhs_id);

/* For the code generator: which instantiation of a column-run evaluation kernel a problem of this shape
 * would run for a model that has a column form publishing `ne` products per element (wave-private kernel
 * k_eval4, narrow states; 0 = no such form) and / or a ghosted form with `ghost` ghost columns per side
 * (workgroup kernel k_eval3, wide states; 0 = none).  Reads only the sizes, kinds and flags of `desc`
 * (pointers other than lower/upper are not followed; no GPU call).
 * out[4] = (eval kernel: 0 flat / 3 / 4, disc, rows per lane run K,
 *           kernel 4: 1 if scalar weights else 0; kernel 3: threads per workgroup).
 * A module built for exactly that instantiation runs it; any other problem runs the module's flat kernel. */
int va_eval_plan(const va_problem_desc *desc, int32_t ne, int32_t ghost, int32_t *out);
/* The same for a column form whose reaches are known: reach[4] = {xl, xr, gl, gr} = how many columns to the left /
 * right f reads (xl, xr) and the adjoint gather receives from (gl, gr).  Wide even states (D > 64) with
 * scalar or per-row weights (any merr_nskip) then run the
 * streaming kernel k_eval5 (csrc/va_eval5.h): out = (5, disc, 0, 0).  Follows desc->Lidx (needs L and Lidx). */
int va_eval_plan_reach(const va_problem_desc *desc, int32_t ne, int32_t ghost, const int32_t *reach, int32_t *out);

int va_problem_create(const va_problem_desc *desc, va_handle *out);
void va_problem_destroy(va_handle h);

/* n_var = N_model*D + NPest; ld_internal = device stride the library uses. */
int va_problem_info(va_handle h, int64_t *n_var, int64_t *ld_internal, int32_t *tile_rows,
                    int32_t *ntiles);

/* Performance knobs of a handle.  None changes a result: the same sums are formed in the same order whichever
 * launch forms them (tests/test_gpu_parity.py::test_tuning_knobs_leave_every_bit_alone).  There are no environment
 * variables behind the library's choices; bench.py reports the knobs it was asked to set. */
#define VA_TUNE_FOLD 1       /* 1: the seed's last-arriving workgroup forms A / runs the line-search step inside the
                              * evaluation kernel (default while the grid is <= 8 workgroups per CU); 0: tail kernels */
#define VA_TUNE_GRAD_SC1 2   /* 1: gradient stores write through (default with FOLD)                                   */
#define VA_TUNE_PRIO 3       /* retired (issue priorities in k_eval4, measured without effect): accepted and ignored     */
#define VA_TUNE_GRAPH 4      /* 1: ladder cycles and timed evaluations are replayed from a hipGraph (default)        */
#define VA_TUNE_PERSIST 5    /* 1: ladders of few seeds on short paths run as ONE launch of the persistent
                              * per-seed kernel (csrc/va_persist.h: every vector of the minimisation resident in LDS),
                              * when the problem is eligible (default); 0: always the three-launch cycle.  Same
                              * arithmetic, different order of the partial sums: results agree to rounding, not bit for bit */
#define VA_TUNE_PERSIST_ROWS 6   /* time rows per workgroup of the persistent kernel (0: the library's choice); VA_EINVAL when not admissible */
#define VA_TUNE_NNET_FUSED 7     /* network handles whose layers are at most 128 wide (at most 64 layers, scalar RM): 1 forward and
                                 * state-gradient products in one kernel (k_nnet_fb), 0 the separate k_nnet_fwd + k_nnet_bwd_x.
                                 * The library's own choice: 1 when blocks of 32 examples x seeds >= 2 x CUs and the activation is a
                                 * built-in other than softplus.  2 + t: as 1, the first workgroups' starts spread over t us (measurement) */
#define VA_TUNE_WIDE 8           /* the wave-private kernel k_eval4: row groups (four waves, tile_rows rows, one row of partial sums)
                                 * per workgroup.  0: one (4-wave workgroups, the default: the wider forms measured slower); 1: the
                                 * planner's rule (as many as shared a CU, on single-round grids that still fill the device); 2, 3: that
                                 * many, VA_EUNSUPPORTED when the run length has no such kernel.  The sums and their order do not change */
int va_problem_tune(va_handle h, int32_t what, int32_t value);
/* The evaluation kernel's launch: row groups per workgroup (1 on every kernel but k_eval4) and the workgroups of one
 * launch, batch x workgroups per seed.  (va_problem_info's ntiles counts row groups.) */
int va_problem_eval_grid(va_handle h, int32_t *row_groups_per_workgroup, int32_t *workgroups);
/* 1 if va_anneal / va_minimize_lbfgs on this handle run the persistent per-seed kernel, with its geometry
 * (workgroups per seed, time rows per workgroup); 0 otherwise. */
int va_problem_persistent(va_handle h, int32_t *workgroups_per_seed, int32_t *rows_per_workgroup);

/* Which evaluation kernel the handle runs (the values of va_problem_desc.eval_kernel: 1 flat,
 * 3 workgroup column runs, 4 wave-private column runs, 5 streaming column strips) and the rows per lane run
 * (0 for the flat kernel, 2 = rows per ring slot for the streaming kernel). */
int va_problem_eval_kernel(va_handle h, int32_t *eval_kernel, int32_t *run_rows);

/* S1 evaluator -- replaces ADmin.A_gradA_taped (_autodiffmin.py:57-58), batched:
 * (A, me, fe, grad A) for all B seeds at RF = RF0*rf_scale.  me/fe follow
 * me_gaussian/fe_gaussian (va_ode.py:138-234).  A/me/fe: [B]; grad: [B*ldg] or NULL.
 * Outputs live where `mem` says. */
int va_action_grad(va_handle h, const double *XP, int64_t ld, int32_t mem, double rf_scale,
                   double *A, double *me, double *fe, double *grad, int64_t ldg);

/* S2 minimiser -- replaces ADmin.min_lbfgs_scipy (_autodiffmin.py:72-95) for
 * bounds=None: device-resident batched L-BFGS with L-BFGS-B's stopping rules.
 * status[b]: 0 converged, 1 maxiter/maxfun reached, 2 abnormal (SciPy warnflag).
 * XP_inout (mem) receives the minimisers; Amin/status/nit/nfev are HOST arrays [B]. */
int va_minimize_lbfgs(va_handle h, double *XP_inout, int64_t ld, int32_t mem, double rf_scale,
                      const va_lbfgs_opts *opts, double *Amin, double *me, double *fe,
                      int32_t *status, int32_t *nit, int64_t *nfev);

/* S3 ladder -- replaces the beta loop of Annealer.anneal + anneal_step
 * (va_ode.py:474-490, 707-789) for all B seeds, each seed climbing the ladder
 * at its own pace, without returning to the host between steps.
 *   rf_scale[nbeta]  = alpha**beta_k (computed by the caller, va_ode.py:650,782)
 *   XP_inout         start paths in, final-step minimisers out
 *   ame  [B*nbeta*3] HOST: (A, me, fe) per seed per step (va_ode.py:773-775)
 *   pest [B*nbeta*NPest] HOST: estimated parameters per step (may be NULL)
 *   status/nit/nfev [B*nbeta] HOST (may be NULL)
 *   minpaths [B*nbeta*(N_model*D+NP)] HOST or NULL; needs desc.keep_paths=1 */
int va_anneal(va_handle h, double *XP_inout, int64_t ld, int32_t mem, const double *rf_scale,
              int32_t nbeta, const va_lbfgs_opts *opts, double *ame, double *pest,
              int32_t *status, int32_t *nit, int64_t *nfev, double *minpaths);

/* Copy the path stored for (seed, beta step) by the last va_anneal (keep_paths=1):
 * out[N_model*D + NP] HOST. */
int va_get_minpath(va_handle h, int32_t seed, int32_t beta_idx, double *out);

/* Forecast from estimated states: integrate T trajectories of the handle's model forward with classical RK4 at the fixed
 * step dt_model / substeps (csrc/va_predict.h; the reference leaves this to the user's script).
 *   x0 [T*D], p [T*NP] (full parameter vectors, constant over the forecast), HOST
 *   stim NULL, or [(n_steps+1)*n_stim] HOST: the stimulus at the model-step times t0 + n dt_model, shared by all
 *        trajectories, interpolated linearly at the stage times in between
 *   out [T*n_out*D] HOST, n_out = n_steps / every + 1: model steps 0, every, 2 every, ...; row 0 is x0 itself
 * The model, D, NP, n_stim, dt_model, device and stream are the handle's.  Not tied to the stored minpaths (the caller
 * chooses the states to start from), and the handle's resident paths, seed states and captured graphs are left alone.
 * VA_EINVAL: T, n_steps, substeps or every < 1; stim missing on a model with a stimulus, or given to one without.
 * VA_EUNSUPPORTED: network handles; D > 1024; a generated model without a flat form (more than 128 parameters). */
int va_predict(va_handle h, const double *x0, const double *p, int32_t T, double t0,
               int32_t n_steps, int32_t substeps, int32_t every, const double *stim, double *out);

/* Hessian-vector products of the action: HV = (d^2 A / d[X | p_est]^2) V at npts points along nvec directions each, on the
 * device (csrc/va_hvp.h: the gradient's linear phases run on tangent inputs, plus the model's second-derivative term).  The
 * reference exposes adolc.hessian of a taped action; a handful of products recovers the block-banded Hessian with its
 * parameter border (va_ode.Annealer.action_hessian), whose inverse is the Laplace approximation's covariance.
 *   XP [npts*ld], V and HV [npts*nvec*ld], HOST, in the usual [X | p_est] packing (the directions of point i follow each
 *        other); P [npts*NP] HOST, full parameter vectors whose estimated entries are taken from XP
 *   rf_scale as in va_action_grad; gauss_newton != 0: the Gauss-Newton part 2 J^T W J only (no second derivatives of the model)
 *   tile_rows 0, or the time rows a workgroup owns (the parameter rows are sums over tiles in tile order: the same bits for
 *        the same geometry)
 * The data, weights, discretisation, device and stream are the handle's.  The handle's BOUNDS are ignored: this is the
 * Hessian of the unconstrained action.  Resident paths, seed states and captured graphs are left alone.
 * VA_EINVAL: npts or nvec < 1, ld < n_var, tile_rows that do not fit the LDS.
 * VA_EUNSUPPORTED (reason in va_last_error): network handles, p_time_dependent, rm_kind / rf_kind 2, modules with a split
 * linear part, generated models without a flat form (more than 128 parameters), states too wide for one owned row. */
int va_hess_vec(va_handle h, const double *XP, const double *P, const double *V, int32_t npts, int32_t nvec, int64_t ld,
                double rf_scale, int32_t gauss_newton, int32_t tile_rows, double *HV);

/* Selected inverse and log-determinant of npts symmetric positive definite block-tridiagonal matrices with a dense border
 * (csrc/va_selinv.h: block Cholesky forward, Takahashi's recurrence backward, one workgroup per matrix), on the handle's
 * device and stream; any handle serves, the blocks are the caller's.  All arrays HOST, C order:
 *   Dk [npts][K][W][W] diagonal blocks, Bk [npts][K-1][W][W] the blocks under them (H_{k+1,k}), Pk [npts][K][NPe][W] the
 *   border, Hpp [npts][NPe][NPe]; NPe = 0 is legal (Pk, Hpp unused), Bk unused at K = 1
 *   Skk, Snk, Spk, Spp: the same blocks of the inverse; any of them NULL: not written
 *   logdet [npts]; status [npts]: 0 fine, k + 1 a pivot <= 0 or NaN in path block k, -1 in the parameters' Schur complement.
 *        Every requested output of a failed matrix is NaN, the others are unaffected, the call returns VA_OK.
 * The same inputs give the same bits on every call.
 * VA_EUNSUPPORTED: W > 64 or NPe > 32 (reason in va_last_error). */
int va_blocktri_selinv(va_handle h, int32_t npts, int32_t K, int32_t W, int32_t NPe, const double *Dk, const double *Bk,
                       const double *Pk, const double *Hpp, double *Skk, double *Snk, double *Spk, double *Spp, double *logdet,
                       int32_t *status);

/* Laplace approximation at npts points: the inverse of the action's Hessian on its own sparsity pattern and log det H.  Per
 * point: coloured directions, k_hvp, k_hblocks, k_selinv; only what is asked for comes back.
 *   XP [npts*ld], P [npts*NP] as in va_hess_vec; rf_scale [npts]: every point its own; gauss_newton as in va_hess_vec
 *   chunk_pts 0, or the points per chunk: the device workspace of a chunk stays under 1 GiB (csrc/va_selinv_geo.h)
 *   var_x [npts*N*D] always; cov_xx [npts*N*D*D] the same-time D x D blocks, cov_px [npts*NPest*N*D], cov_pp
 *        [npts*NPest*NPest]: NULL = not wanted; logdet [npts], status [npts] as in va_blocktri_selinv (blocks of hb = 1 time
 *        row, 2 with Simpson-Hermite).  A point whose Hessian is not positive definite is NaN with its status set.
 * Bounds are ignored, resident paths, seed states and captured graphs left alone, as in va_hess_vec.
 * VA_EINVAL: npts < 1, ld < n_var, a forced chunk that does not fit the workspace.
 * VA_EUNSUPPORTED: whatever va_hess_vec refuses; D > 64, D > 32 with Simpson-Hermite, more than 32 estimated parameters. */
int va_laplace(va_handle h, const double *XP, const double *P, int32_t npts, int64_t ld, const double *rf_scale,
               int32_t gauss_newton, int32_t chunk_pts, double *var_x, double *cov_xx, double *cov_px, double *cov_pp,
               double *logdet, int32_t *status);

/* Forecast spread: va_predict's trajectories and, with each, the tangent-linear model of the discrete RK4 map along nvec
 * directions (csrc/va_predict_tlm.h: every stage's k' = J(x_stage) v_stage + (df/dp) v_p, the exact derivative of the
 * integrator, not of the differential equation), and their sums over directions.  With the directions of a trajectory
 * the columns of a square root S of the covariance Sigma_0 = S S^T of (x0, p_est), var and cov are the linearised forecast
 * covariance M_n Sigma_0 M_n^T at every output row.
 *   x0, p, T, t0, n_steps, substeps, every, stim as in va_predict (the stimulus is known: it has no tangent)
 *   V0 [T*nvec*(D+NPest)] HOST: per direction the state part, then the estimated parameters' in Pidx order (constant)
 *   out [T*n_out*D] the nominal trajectory, row 0 is x0
 *   dX [T*nvec*n_out*D] the tangents' state parts, row 0 is V0's state part; var [T*n_out*D] = sum over directions of
 *        dX^2; cov [T*n_out*D*D] = sum over directions of dX_i dX_j at equal times; each may be NULL: not wanted.  The sums
 *        run in direction order, products and additions rounded one by one: the same bits on every call.
 * All arrays HOST.  The tangents live in a device workspace chunked over trajectories (a chunk under 1 GiB).  The handle's
 * resident paths, seed states and captured graphs are left alone.
 * VA_EINVAL: what va_predict rejects; nvec < 1.
 * VA_EUNSUPPORTED (reason in va_last_error): network handles; D > 1024; generated models without a flat form (more than
 * 128 parameters); modules with a split linear part; one trajectory's tangents past the workspace limit. */
int va_predict_tangent(va_handle h, const double *x0, const double *p, const double *V0, int32_t T, int32_t nvec, double t0,
                       int32_t n_steps, int32_t substeps, int32_t every, const double *stim, double *out, double *dX,
                       double *var, double *cov);

/* Adjoint of the forecast (csrc/va_predict_adj.h): va_predict's trajectories and, for ncot cotangent sets per trajectory, the
 * transpose of the derivative of the DISCRETE RK4 map that va_predict_tangent applies (not a discretisation of the continuous
 * adjoint equation): gx0 = (d out / d x0)^T G and gp = (d out / d p_est)^T G, one backward sweep per set.  The nominal is
 * integrated forward with checkpoints of every RK4 step (n_steps * substeps * D doubles per trajectory and workgroup that
 * carries it, in device memory), then the steps are walked backward.
 *   x0, p, T, t0, n_steps, substeps, every, stim as in va_predict
 *   exactly one of G and Y:
 *   G [T*ncot*n_out*D] cotangent mode: the cotangents of the output rows
 *   Y [T*n_out*L], or [n_out*L] with y_shared != 0: misfit mode, ncot = 1: observations of the handle's Lidx columns (in the
 *        order the handle was created with) at the output rows; weights [L].  The cotangents are 2 w_l (x_l - y_l) and
 *        cost [T] = sum over rows and columns of w_l (x_l - y_l)^2 (per column in row order, then over the columns in order)
 *   out [T*n_out*D] the nominal trajectory; gx0 [T*ncot*D]; gp [T*ncot*NPest], the estimated parameters in Pidx order
 * All arrays HOST.  No atomics anywhere: the same bits on every call.  The handle's bounds are ignored; its resident paths,
 * seed states and captured graphs are left alone.
 * VA_EINVAL: what va_predict rejects; both or neither of G and Y; ncot < 1; misfit mode with ncot != 1, no weights or no cost.
 * VA_EUNSUPPORTED (reason in va_last_error): network handles; D > 1024; generated models without a flat form (more than
 * 128 parameters); modules with a split linear part; parameters and partials past 64 KiB of LDS; one trajectory's
 * checkpoints and cotangents past the workspace limit. */
int va_predict_adjoint(va_handle h, const double *x0, const double *p, const double *G, const double *Y, const double *weights,
                       int32_t y_shared, int32_t T, int32_t ncot, double t0, int32_t n_steps, int32_t substeps, int32_t every,
                       const double *stim, double *out, double *gx0, double *gp, double *cost);

/* Strong-constraint shooting on the device (csrc/va_shoot.h): for each of T points, minimise va_predict_adjoint's misfit
 *     cost(x0, p_est) = sum over rows and columns of w_l (x_l(t; x0, p) - y_l)^2
 * over x0 and the handle's estimated parameters by L-BFGS (what SciPy's L-BFGS-B does without bounds: dcsrch line search, m
 * history pairs), all points in ONE launch per chunk of points: a point's workgroup evaluates cost and gradient with the
 * adjoint predictor's phases and steps the point's minimiser, evaluation after evaluation, without returning to the host.
 *   x0 [T*D], p [T*NP] the starts (full parameter vectors); Y, weights, y_shared, t0, n_steps, substeps, every, stim as in
 *        va_predict_adjoint's misfit mode
 *   m history pairs (1 .. 32); maxiter >= 1; 1 <= maxfun <= 100000; maxls >= 1 trials per line search; ftol, gtol: stop when
 *        f_old - f <= ftol max(|f_old|, |f|, 1), or when the largest gradient entry <= gtol
 *   x0_out [T*D], p_out [T*NP] the returned points (full vectors; entries that are not estimated are the caller's);
 *   cost [T], cost_start [T]; grad_max [T] the largest gradient entry at the returned point; nit [T]; nfev [T] (<= maxfun + 1);
 *   status [T]: 0 converged, 1 maxiter or maxfun reached, 2 abnormal line search, 3 the cost at the start was not finite
 *        (that point comes back unchanged; nothing raises).  A finite iterate is what comes back in every case.
 * All arrays HOST.  No atomics, every sum in index order: the same bits on every call, and whichever points share a launch.
 * The handle's resident paths, seed states and captured graphs are left alone.
 * VA_EINVAL: what va_predict_adjoint rejects in misfit mode; m, maxiter, maxfun or maxls out of range.
 * VA_EUNSUPPORTED (reason in va_last_error): what va_predict_adjoint refuses; D > 512; a handle with box bounds (no projected
 * step yet). */
int va_shoot(va_handle h, const double *x0, const double *p, const double *Y, const double *weights, int32_t y_shared, int32_t T,
             double t0, int32_t n_steps, int32_t substeps, int32_t every, const double *stim, int32_t m, int64_t maxiter,
             int64_t maxfun, int32_t maxls, double ftol, double gtol, double *x0_out, double *p_out, double *cost,
             double *cost_start, double *grad_max, int32_t *nit, int32_t *nfev, int32_t *status);

/* va_shoot inside a box (csrc/va_shoot_box.h): the same misfit, minimised subject to lower <= [x0 | p_est] <= upper by
 * L-BFGS-B, one lane per point running the published algorithm between evaluations (Byrd, Lu, Nocedal & Zhu 1995; Algorithm
 * 778 in its 3.0 form, the one SciPy runs: generalised Cauchy point, subspace minimisation over the free variables with the
 * projection step, dcsrch limited by the largest feasible step).  Arguments and outputs as va_shoot, and
 *   lower, upper [n] (box_shared != 0: one table for all points) or [T*n], n = D + NPest: the D state columns, then the
 *        estimated parameters in Pidx order; -inf / +inf: no bound
 * The start is projected onto the box first: cost_start is the cost of the PROJECTED start.  grad_max [T] is the
 * projected-gradient norm at the returned point (it takes the largest gradient entry's place in the gtol test).  Every
 * returned entry satisfies lower <= x <= upper exactly; a finite, feasible iterate comes back in every case.  The same bits
 * on every call, and whichever points share a launch.
 * The handle's own bounds table is not looked at (as in va_hess_vec): the caller's box is the box, on bounded and unbounded
 * handles alike.  va_shoot keeps refusing bounded handles.
 * VA_EINVAL: what va_shoot rejects; lower / upper NULL; an entry with lower > upper or NaN (named in va_last_error).
 * VA_EUNSUPPORTED: what va_shoot refuses, but for the handle's bounds. */
int va_shoot_box(va_handle h, const double *x0, const double *p, const double *Y, const double *weights, int32_t y_shared, int32_t T,
                 double t0, int32_t n_steps, int32_t substeps, int32_t every, const double *stim, int32_t m, int64_t maxiter,
                 int64_t maxfun, int32_t maxls, double ftol, double gtol, const double *lower, const double *upper, int32_t box_shared,
                 double *x0_out, double *p_out, double *cost, double *cost_start, double *grad_max, int32_t *nit, int32_t *nfev,
                 int32_t *status);

/* Lyapunov spectra of the handle's model (csrc/va_lyap.h): T trajectories from x0 with the parameters p, each with K <= D
 * tangents carried by the tangent-linear model of the RK4 integrator (va_predict's steps, stage times and stimulus; the
 * parameter tangent is zero) and re-orthonormalised together by a thin QR with positive diagonal after every qr_every model
 * steps.  With gains g = coupling[t] >= 0 every tangent stage is J(x) v - g o v: the exponents are then the CONDITIONAL
 * ones of a copy of the model driven through those columns.
 *   x0 [T][D], p [T][NP]; Q0 [T][K][D] the starting tangents (rows), or NULL: the first K unit vectors;
 *   coupling [T][D] or NULL; stim as va_predict's;  n_steps a multiple of qr_every, n_qr = n_steps / qr_every,
 *   0 <= n_skip < n_qr: the QRs left out of the sums
 *   logsum [T][K]: sum of log R_jj over the QRs n_skip .. n_qr - 1, in time order (the exponents are
 *           logsum / ((n_qr - n_skip) qr_every dt_model));  x_end [T][D], Q_end [T][K][D]: where a following call starts
 *           (at t0 + n_steps dt_model);  trace NULL or [T][n_qr][K]: every log R_jj;  status [T]: 0, or j + 1 of the first
 *           R_jj that was zero or not finite -- that trajectory's logsum is then NaN, the call still returns VA_OK.
 * Works on buffers of its own, chunked over trajectories, like va_predict_tangent; the handle's resident state is left alone.
 * VA_EINVAL (before the device is touched): what va_predict rejects; K outside 1 .. D; n_steps not a multiple of qr_every;
 * n_skip outside 0 .. n_qr - 1; a negative or non-finite gain.
 * VA_EUNSUPPORTED (reason in va_last_error): network handles; modules with a split linear part; generated models without a
 * flat form; D > 64 or (K + 1) D > 2048. */
int va_lyapunov(va_handle h, const double *x0, const double *p, const double *Q0, const double *coupling, int32_t T, int32_t K,
                double t0, int32_t n_steps, int32_t substeps, int32_t qr_every, int32_t n_skip, const double *stim,
                double *logsum, double *x_end, double *Q_end, double *trace, int32_t *status);

/* Track new data from the estimates: the ensemble Kalman filter of the handle's model on the device (csrc/va_enkf.h).  T
 * points of M members each; for observation row k = 0 .. n_obs - 1 every member moves obs_every model steps as va_predict
 * moves a trajectory (each with its own parameter vector), the forecast mean and standard deviation of the D + NQ augmented
 * variables z = (x, p[est]) are recorded (mean in member order, variance over M - 1), the members are inflated about their
 * mean (z = mean + inflation (z - mean); skipped exactly at 1), the observations of the row are assimilated one after the
 * other by the serial ensemble square-root filter (Whitaker & Hamill 2002; a NaN is a missing observation), and the analysis
 * mean and standard deviation are recorded.
 *   x0 [T][M][D], p [T][M][NP] full vectors; est [NQ] the positions in p that the filter updates (NQ = 0: states only; the
 *   other entries stay as given); Y [T][n_obs][L] the handle's Lidx columns, row k at t0 + (k + 1) obs_every dt_model;
 *   obs_var [L]; stim as va_predict's, n_obs obs_every + 1 rows
 *   mean_f, sd_f, mean_a, sd_a [T][n_obs][D + NQ];  x_end [T][M][D], p_end [T][M][NP]: where a following call starts;
 *   status [T]: 0, or k + 1 of the first row at whose forecast some member of the point is not finite -- from that row on the
 *           point's statistics are NaN, x_end / p_end hold what the arithmetic gave, the call still returns VA_OK.
 * One workgroup per point: a point's bits do not depend on what shares its call.  Works on buffers of its own, chunked over
 * points, like va_predict; the handle's resident state is left alone.  Bounds are not enforced on filtered parameters.
 * VA_EINVAL (before the device is touched): what va_predict rejects; sizes below 1; est entries outside 0 .. NP-1 or
 * repeated; an obs_var entry that is not positive and finite; inflation < 1.
 * VA_EUNSUPPORTED (reason in va_last_error): network handles; generated models without a flat form; M < 2; M D > 2048; members,
 * parameters and stimulus past 64 KiB of LDS; more stimulus columns than threads of a workgroup.  A module whose dense linear
 * part was split off is carried (the members move through the predictor's own right-hand side). */
int va_enkf(va_handle h, const double *x0, const double *p, const int32_t *est, int32_t NQ, const double *Y, const double *obs_var,
            double inflation, int32_t T, int32_t M, double t0, int32_t n_obs, int32_t obs_every, int32_t substeps, const double *stim,
            double *mean_f, double *sd_f, double *mean_a, double *sd_a, double *x_end, double *p_end, int32_t *status);

/* Sample exp(-A(X, p)) at one rf_scale: B Hamiltonian Monte Carlo chains, one per seed of the handle, on the device
 * (csrc/va_hmc.h).  An iteration draws a momentum p = z / sqrt(minv), runs n_leap leapfrog steps of size
 * eps_it = eps[b] (1 + jitter (2 u - 1)) -- n_leap evaluations by the handle's own evaluation kernel, an element-wise launch
 * between two of them -- and accepts iff log(u_acc) < -dH, dH = (A1 + K1) - (A0 + K0), K = 1/2 sum p^2 minv.  A non-finite
 * dH is a rejection (counted in n_divergent); a rejected iteration leaves the chain where it was.
 *   XP [B*ld] in: start points; out: the chains' final states (HOST or DEVICE, `mem`)
 *   eps [B]; jitter in [0, 1); minv NULL (identity) or minv_n = n_var values shared by the chains, or B * n_var
 *   seed: key of the counter-based generator (Philox4x32-10, counter (chain, iteration, element, stream)): the draws do not
 *        depend on the launch geometry.  noise NULL, or [n_iter][B][n_var + 2] the caller's own numbers instead: n_var
 *        standard normals, the accept uniform, the jitter uniform
 *   thin, keep_idx [n_keep_idx] (indices into the path vector): kept [B][n_iter / thin][n_keep_idx] holds those entries of
 *        the state after every thin-th iteration
 *   mean, var [B*n_var] over the n_iter states (var: sample variance, 0 for n_iter = 1); A_trace, dH, accepted
 *        [B*n_iter]; n_divergent [B].  All HOST, any may be NULL.  The same inputs give the same bits on every call.
 * One rf_scale per call.  The handle's resident paths are saved and restored, its seeds left idle; the evaluations
 * (B (n_iter n_leap + 1)) are counted as va_action_grad's.  Plain launches on the handle's stream.
 * VA_EINVAL: n_iter, n_leap or thin < 1; an eps or minv entry not positive and finite; jitter outside [0, 1); a keep_idx
 * outside [0, n_var); a minv_n that is neither n_var nor B * n_var.
 * VA_EUNSUPPORTED: handles with box bounds (va_hmc_box samples those), network handles. */
int va_hmc(va_handle h, double *XP, int64_t ld, int32_t mem, double rf_scale, int32_t n_iter, int32_t n_leap, const double *eps,
           double jitter, const double *minv, int64_t minv_n, uint64_t seed, const double *noise, int32_t thin,
           const int64_t *keep_idx, int32_t n_keep_idx, double *mean, double *var, double *A_trace, double *dH, int32_t *accepted,
           int32_t *n_divergent, double *kept);
/* va_hmc for box-bounded problems (csrc/va_hmc_box.h): the chain runs in an unconstrained z with x = T(z) element by
 * element (T algebraic: + - * / sqrt), on the target U(z) = A(T(z)) - sum log|T'(z)|, so the x of its states follow exp(-A)
 * restricted to the box.  va_hmc's arguments and outputs, which speak of x (statistics, kept columns, A_trace), plus:
 *   lower, upper [n_var] (-/+HUGE_VAL: no bound), shared by the chains; both NULL: the handle's own bounds.  Bounds may be
 *        passed on a handle created without any -- the sampler does not care which evaluation kernel runs.
 *   Z0 NULL: the chains start at XP, inverted on the host; or [B][n_var] the start in z (XP is then only written)
 *   Z_out NULL or [B][n_var]: the final z -- pass it as the next call's Z0 to continue a chain without re-inverting x
 *   minv is the inverse mass of z; dH includes the log-Jacobian terms.
 * The tails of T are polynomial (|dx/dz| ~ 1/z^2 for one-sided, 1/|z|^3 for two-sided bounds): good for bounds used as
 * guards, weak where the posterior piles up on a bound.
 * VA_EINVAL (naming the entry): lower[i] >= upper[i] or NaN; a start not strictly inside its box; a Z0 entry not finite;
 * everything va_hmc rejects.  VA_EUNSUPPORTED: network handles; no finite bound from either source. */
int va_hmc_box(va_handle h, double *XP, int64_t ld, int32_t mem, double rf_scale, int32_t n_iter, int32_t n_leap, const double *eps,
               double jitter, const double *minv, int64_t minv_n, uint64_t seed, const double *noise, int32_t thin,
               const int64_t *keep_idx, int32_t n_keep_idx, const double *lower, const double *upper, const double *Z0, double *Z_out,
               double *mean, double *var, double *A_trace, double *dH, int32_t *accepted, int32_t *n_divergent, double *kept);
/* The map of va_hmc_box as the current device computes it, entry by entry over a table: x = T(z), dx = dx/dz,
 * dlj = d log|dx/dz| / dz, lj = log|dx/dz| [n].  HOST arrays.  Needs no handle. */
int va_hmc_box_map(int64_t n, const double *lower, const double *upper, const double *z, double *x, double *dx, double *dlj, double *lj);
/* Exactly what va_hmc's kernels draw for (seed, chain, iteration), computed on the current device: words [(n + 1)*4] the
 * generator's four words for each of the n elements and for the extra stream, normals [n], uniforms [2] (accept, jitter).
 * HOST arrays, any may be NULL.  Needs no handle. */
int va_hmc_noise(uint64_t seed, int32_t chain, int32_t iteration, int64_t n, uint32_t *words, double *normals, double *uniforms);

/* Measurement hook for bench.py: `iters` complete S1 evaluations (the same launch va_action_grad
 * makes: A, me, fe and the full gradient are formed every time) on the resident paths (those of
 * the last va_action_grad / va_anneal call), bracketed by HIP events on the handle's stream;
 * returns elapsed ms. */
int va_eval_timed(va_handle h, double rf_scale, int32_t iters, float *elapsed_ms);
/* Everything va_eval_timed(h, rf_scale, iters, ..) would otherwise do before its first launch -- arming the seeds,
 * capturing / instantiating / uploading the hipGraph of the chunk of launches it replays -- done now, so that a caller
 * who brackets va_eval_timed with a wall clock of its own (bench.py) times the launches only.  The graph is keyed on
 * the bytes of the device image it captured: any later change of the handle makes va_eval_timed rebuild it. */
int va_eval_timed_prepare(va_handle h, double rf_scale, int32_t iters);

/* Measurement hook for bench.py: `iters` launches each of the two L-BFGS vector kernels (k_update,
 * k_direction) with every seed's history full (lbfgs_m pairs), bracketed by HIP events; returns the
 * elapsed ms of each.  Overwrites the resident paths and the L-BFGS state: evaluate / anneal again
 * from host data afterwards.  VA_EUNSUPPORTED for a bounded handle (its third launch is k_lbfgsb_dir). */
int va_lbfgs_timed(va_handle h, int32_t iters, float *ms_update, float *ms_direction);
/* Measurement only: `iters` evaluation launches as a ladder cycle makes them (every seed at a line-search trial
 * point x + stp*d, the tail runs one line-search step), each after re-arming the seeds; *ms_eval = the launches'
 * time with the re-arming kernel's own time (measured in a second pass) subtracted.  Leaves the seeds idle. */
int va_eval_ls_timed(va_handle h, double rf_scale, int32_t iters, float *ms_eval);

/* The outputs the last S1 evaluation (va_action_grad or va_eval_timed) left on the device:
 * A/me/fe [B], grad [B*ldg] (any may be NULL), HOST arrays. */
int va_read_eval_outputs(va_handle h, double *A, double *me, double *fe, double *grad, int64_t ldg);

/* Profiling hook: copy the first n doubles of the L-BFGS inner-product partial table to the host. */
int va_debug_read_partials(va_handle h, double *out, int64_t n);

/* Profiling hook: the per-phase tick sums (100 MHz) a -DVA_PZ_STAMPS measurement build of the persistent kernel leaves
 * behind (n <= 14 doubles; zeros from the product library). */
int va_debug_read_persist(va_handle h, double *out, int64_t n);

/* Cumulative counters since create: batched eval launches, seed-evaluations,
 * L-BFGS cycles. */
int va_get_counters(va_handle h, int64_t *eval_launches, int64_t *seed_evals, int64_t *cycles);

/* ---- the single collective of a multi-GPU job -------------------------------
 * Independent annealing runs are sharded over the GPUs of a node, one process per GPU; the reference's
 * counterpart is an SGE array job whose tasks leave their results in files
 * (examples/nnet_barimages/SGEcluster/submit_multiM.sh:14-30, SGE_bardata_anneal.py:129-132).  Nothing is
 * exchanged while the ladders run; at the end ONE RCCL all-gather over xGMI collects the per-seed result
 * tables (KBs: latency-bound).  librccl.so is loaded on first use (dlopen); a job that never gathers
 * does not need it.  The Python host normally issues the same collective through torch.distributed
 * (varanneal_amd/parallel.py: backend "nccl" is RCCL); these entry points serve callers without torch. */
typedef struct va_comm_s *va_comm;
#define VA_COMM_ID_BYTES 128
/* rank 0 calls this once and hands the 128 bytes to the other ranks (file, socket, MPI, ...) */
int va_comm_unique_id(char id[VA_COMM_ID_BYTES]);
/* every rank: join the communicator of `world` ranks on `device` (blocks until all have joined) */
int va_comm_create(const char id[VA_COMM_ID_BYTES], int32_t world, int32_t rank, int32_t device, va_comm *out);
void va_comm_destroy(va_comm c);
/* After va_anneal(h, ..., nbeta, ...): all-gather the result tables of every rank's B seeds (the same B
 * on all ranks) on h's stream.  HOST outputs, rank-major then seed-major:
 *   table  [world*B][nbeta][3 + NPest] = (A, me, fe, estimated parameters) per seed and ladder step
 *   status [world*B][nbeta]            (may be NULL) */
int va_gather_results(va_handle h, va_comm c, int32_t nbeta, double *table, int32_t *status);

/* ---- feed-forward-network action (reference: varanneal/va_nnet.py) -------------------
 * va_nnet.Annealer estimates the neuron states of M training examples and (a subset of)
 * the weights/biases of an all-to-all layered network; the "model error" is the mismatch
 * x_{n+1} - f(W_n x_n + b_n) of every layer transition (va_nnet.py:175-255), the
 * measurement error acts on observed input/output neurons (va_nnet.py:117-173).
 * A handle made here is used with the SAME S1/S2/S3 entry points above; its path vector is
 *     XP[b] = [ X[b]: M examples x NDnet states, example-major | p_est (NPest) ]   (va_nnet.py:440)
 * with NDnet = sum(structure); the flat parameter vector is W_0 (structure[1] x structure[0],
 * row-major), b_0, W_1, b_1, ... (va_nnet.py:194-207).  minpaths rows returned by va_anneal
 * for such a handle are [X | p_est] (n_var wide); the caller scatters p_est into P. */
enum { VA_ACT_SIGMOID = 0,   /* 1/(1+exp(-(W x + b))): examples/nnet_twin/nnet_twin_anneal.py:20-22 */
       VA_ACT_TANH = 1, VA_ACT_LINEAR = 2,
       VA_ACT_RELU = 3,      /* max(W x + b, 0) */
       VA_ACT_SOFTPLUS = 4,  /* log(1 + exp(W x + b)) */
       VA_ACT_USER_BASE = 1000 /* ids >= this: generated activation modules (va_act_load_module) */ };

typedef struct va_nnet_desc {
    int32_t struct_size;      /* = sizeof(va_nnet_desc)                                  */
    int32_t device;
    int32_t batch;            /* B independent initial guesses ("seeds")                  */
    int32_t n_layers;         /* len(structure), >= 2 (set_structure, va_nnet.py:59-69)   */
    const int32_t *structure; /* [n_layers] neurons per layer                             */
    int32_t M;                /* training examples (set_input_data, va_nnet.py:78-91)     */
    int32_t L_in, L_out;      /* observed input / output neurons (va_nnet.py:324-332)     */
    const int32_t *Lidx_in;   /* [L_in]  indices into the input layer                     */
    const int32_t *Lidx_out;  /* [L_out] indices into the output layer                    */
    const double *data_in;    /* [M][L_in]                                                */
    const double *data_out;   /* [M][L_out]                                               */
    double rm_in, rm_out;     /* RM scalar -> both equal; RM = [a, b] -> (a, b) (va_nnet.py:132-147) */
    double rf0;               /* RF = rf0 * rf_scale                                      */
    int32_t NP, NPest;        /* all parameters / estimated ones                          */
    const int32_t *Pidx;      /* [NPest] indices into the flat parameter vector           */
    const double *P;          /* [batch][NP] initial/fixed values                         */
    int32_t activation;       /* VA_ACT_* or an id from va_act_load_module                */
    int32_t lbfgs_m;          /* history pairs kept on the device (0 -> 10)               */
    int32_t max_beta;         /* longest ladder va_anneal will be given                   */
    int32_t keep_paths;       /* store every step's minimiser                             */
    void *stream;             /* hipStream_t to use, or NULL for a private one            */
    const double *rm_in_matrix;  /* NULL, or [L_in][L_in]:  RM = [RMin, RMout] with full matrices,       */
    const double *rm_out_matrix; /* NULL, or [L_out][L_out]: diff.(RM.diff) per example (va_nnet.py:136-139); both or neither */
} va_nnet_desc;

/* Register a compiled activation module (a shared object built from varanneal_amd/csrc/va_user_act.hip + a
 * generated header: the elementwise g of a user layer map f(x, W, b) = g(W x + b), va_nnet.py:71, 260-264);
 * returns the id to put in va_nnet_desc.activation. */
int va_act_load_module(const char *path, int32_t *act_id);

/* Everything va_nnet.Annealer.anneal_init() freezes (va_nnet.py:288-450). */
int va_nnet_problem_create(const va_nnet_desc *desc, va_handle *out);

#ifdef __cplusplus
}
#endif
#endif /* VARANNEAL_AMD_H */
