"""ctypes binding of include/varanneal_amd.h (libvaranneal_amd.so).

This is the thin shim north_star asks for: host code stays Python, the HIP
kernels are reached through a plain C-ABI.  There is NO CPU fallback: if the
shared library is missing or fails to load, importing callers get a loud
`VaLibraryError`.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VARANNEAL_AMD_LIB", os.path.join(_HERE, "libvaranneal_amd.so"))   # (env: diagnostic builds)

VA_OK = 0
VA_EUNSUPPORTED = -4
ABI_VERSION = 12         # VA_ABI_VERSION of include/varanneal_amd.h
ERRNAMES = {-1: "VA_EINVAL", -2: "VA_ENOMEM", -3: "VA_EHIP", -4: "VA_EUNSUPPORTED", -5: "VA_ESTATE"}
DISC = {"euler": 0, "trapezoid": 1, "SimpsonHermite": 2, "forwardmap": 3}
RHS = {"lorenz96": 0}
MEM_HOST, MEM_DEVICE = 0, 1

c_dp = C.POINTER(C.c_double)
c_ip = C.POINTER(C.c_int32)
c_lp = C.POINTER(C.c_int64)


class VaLibraryError(RuntimeError):
    pass


class VaError(RuntimeError):
    def __init__(self, code, msg):
        RuntimeError.__init__(self, "%s (%d): %s" % (ERRNAMES.get(code, "VA_E?"), code, msg))
        self.code = code


class VaUnsupported(VaError, NotImplementedError):
    """VA_EUNSUPPORTED: a case the library does not implement (the message names why), e.g. a model past 128 parameters
    on a problem its column-parameter form cannot run.  Still a VaError; a NotImplementedError as well, like every
    unsupported case of the Python layer."""


class ProblemDesc(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("device", C.c_int32), ("batch", C.c_int32),
                ("D", C.c_int32), ("N_model", C.c_int32), ("N_data", C.c_int32),
                ("merr_nskip", C.c_int32), ("L", C.c_int32),
                ("Lidx", c_ip), ("Y", c_dp), ("dt_model", C.c_double),
                ("rm_kind", C.c_int32), ("rm", C.c_double), ("rm_array", c_dp),
                ("rf_kind", C.c_int32), ("rf0", C.c_double), ("rf0_array", c_dp),
                ("NP", C.c_int32), ("NPest", C.c_int32), ("Pidx", c_ip), ("P", c_dp),
                ("disc", C.c_int32), ("rhs", C.c_int32), ("lbfgs_m", C.c_int32),
                ("max_beta", C.c_int32), ("keep_paths", C.c_int32), ("tile_rows", C.c_int32),
                ("eval_kernel", C.c_int32), ("t_model", c_dp), ("stim", c_dp), ("n_stim", C.c_int32),
                ("p_time_dependent", C.c_int32), ("stream", C.c_void_p),
                ("lower", c_dp), ("upper", c_dp)]


class NnetDesc(C.Structure):
    _fields_ = [("struct_size", C.c_int32), ("device", C.c_int32), ("batch", C.c_int32),
                ("n_layers", C.c_int32), ("structure", c_ip), ("M", C.c_int32),
                ("L_in", C.c_int32), ("L_out", C.c_int32), ("Lidx_in", c_ip), ("Lidx_out", c_ip),
                ("data_in", c_dp), ("data_out", c_dp), ("rm_in", C.c_double), ("rm_out", C.c_double),
                ("rf0", C.c_double), ("NP", C.c_int32), ("NPest", C.c_int32), ("Pidx", c_ip), ("P", c_dp),
                ("activation", C.c_int32), ("lbfgs_m", C.c_int32), ("max_beta", C.c_int32),
                ("keep_paths", C.c_int32), ("stream", C.c_void_p),
                ("rm_in_matrix", c_dp), ("rm_out_matrix", c_dp)]


ACTIVATION = {"sigmoid": 0, "tanh": 1, "linear": 2, "relu": 3, "softplus": 4}


class LbfgsOpts(C.Structure):
    _fields_ = [("maxcor", C.c_int32), ("ftol", C.c_double), ("gtol", C.c_double),
                ("maxiter", C.c_int32), ("maxfun", C.c_int64), ("maxls", C.c_int32)]


def make_opts(opt_args=None):
    """SciPy L-BFGS-B option names and defaults (scipy/optimize/_lbfgsb_py.py)."""
    o = dict(opt_args or {})
    return LbfgsOpts(int(o.get("maxcor", 10)), float(o.get("ftol", 2.2204460492503131e-09)),
                     float(o.get("gtol", 1e-5)), int(min(int(o.get("maxiter", 15000)), 2 ** 31 - 1)),
                     int(o.get("maxfun", 15000)), int(o.get("maxls", 20)))


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def make_desc(batch, D, N_model, Y, Lidx, dt_model, RM, RF0, P, Pidx, disc="trapezoid",
              rhs="lorenz96", merr_nskip=1, lbfgs_m=10, max_beta=1, keep_paths=0, tile_rows=0,
              eval_kernel=0, device=0, stream=None, t_model=None, stim=None, p_time_dependent=False, bounds=None):
    """Build a ProblemDesc plus the list of arrays that must outlive it.  With
    p_time_dependent, P has shape (batch, N_model, NP) (or (N_model, NP), shared by the seeds)."""
    Y = _f64(Y)
    N_data, L = Y.shape
    Lidx = np.ascontiguousarray(Lidx, dtype=np.int32)
    Pidx = np.ascontiguousarray(Pidx, dtype=np.int32)
    P = _f64(P)
    if p_time_dependent:
        if P.ndim == 2:
            P = np.ascontiguousarray(np.broadcast_to(P, (batch,) + P.shape))
        if P.ndim != 3 or P.shape[:2] != (batch, N_model):
            raise ValueError("time-dependent P must have shape (batch, N_model, NP)")
    elif P.ndim == 1:
        P = np.ascontiguousarray(np.broadcast_to(P, (batch, P.shape[0])))
    keep = [Y, Lidx, Pidx, P]
    d = ProblemDesc()
    d.struct_size = C.sizeof(ProblemDesc)
    d.device, d.batch, d.D, d.N_model, d.N_data = device, batch, D, N_model, N_data
    d.merr_nskip, d.L = merr_nskip, L
    d.Lidx = Lidx.ctypes.data_as(c_ip)
    d.Y = Y.ctypes.data_as(c_dp)
    d.dt_model = float(dt_model)
    if isinstance(RM, np.ndarray):
        rm = _f64(RM)
        if rm.shape not in [(N_data, L), (N_data, L, L)]:
            raise ValueError("RM array must have shape (N_data, L) or (N_data, L, L)")
        keep.append(rm)
        d.rm_kind, d.rm, d.rm_array = rm.ndim - 1, 0.0, rm.ctypes.data_as(c_dp)
    else:
        d.rm_kind, d.rm, d.rm_array = 0, float(RM), None
    if isinstance(RF0, np.ndarray):
        rf = _f64(RF0)
        if rf.shape not in [(N_model - 1, D), (N_model - 1, D, D)]:
            raise ValueError("RF0 array must have shape (N_model-1, D) or (N_model-1, D, D)")
        keep.append(rf)
        d.rf_kind, d.rf0, d.rf0_array = rf.ndim - 1, 0.0, rf.ctypes.data_as(c_dp)
    else:
        d.rf_kind, d.rf0, d.rf0_array = 0, float(RF0), None
    d.NP, d.NPest = P.shape[-1], len(Pidx)
    d.p_time_dependent = 1 if p_time_dependent else 0
    d.Pidx = Pidx.ctypes.data_as(c_ip)
    d.P = P.ctypes.data_as(c_dp)
    d.disc = DISC[disc] if isinstance(disc, str) else int(disc)
    d.rhs = RHS[rhs] if isinstance(rhs, str) else int(rhs)      # int: a module id from load_rhs_module
    d.lbfgs_m, d.max_beta, d.keep_paths, d.tile_rows = lbfgs_m, max_beta, keep_paths, tile_rows
    d.eval_kernel = eval_kernel
    if t_model is not None:
        tm = _f64(t_model)
        if tm.shape != (N_model,):
            raise ValueError("t_model must have shape (N_model,)")
        keep.append(tm)
        d.t_model = tm.ctypes.data_as(c_dp)
    else:
        d.t_model = None
    if stim is not None:
        st = _f64(stim)
        st = st.reshape(N_model, -1)
        keep.append(st)
        d.stim, d.n_stim = st.ctypes.data_as(c_dp), st.shape[1]
    else:
        d.stim, d.n_stim = None, 0
    d.stream = stream
    d.lower = d.upper = None
    if bounds is not None:
        # one (lo, hi) per entry of the path vector [X | p_est] (va_ode.py:582-605); None = no bound
        n_var = N_model * (D + len(Pidx)) if p_time_dependent else N_model * D + len(Pidx)
        if len(bounds) != n_var:
            raise ValueError("bounds must have one (lo, hi) pair per entry of the path vector (%d), got %d" % (n_var, len(bounds)))
        lo = np.array([-np.inf if b[0] is None else b[0] for b in bounds], dtype=np.float64)
        hi = np.array([np.inf if b[1] is None else b[1] for b in bounds], dtype=np.float64)
        keep += [lo, hi]
        d.lower, d.upper = lo.ctypes.data_as(c_dp), hi.ctypes.data_as(c_dp)
    return d, keep


_lib = None


def lib():
    """Load libvaranneal_amd.so (built by varanneal_amd._build / __graft_entry__.build)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VaLibraryError("%s not found: build it with `python -m varanneal_amd._build` "
                             "(hipcc --offload-arch=gfx950). There is no CPU fallback." % LIB_PATH)
    try:
        L = C.CDLL(LIB_PATH)
    except OSError as e:
        raise VaLibraryError("cannot load %s: %s" % (LIB_PATH, e))
    h = C.c_void_p
    L.va_abi_version.restype = C.c_int32
    if L.va_abi_version() != ABI_VERSION:
        raise VaLibraryError("%s has ABI version %d, this binding expects %d: rebuild it with "
                             "`python -m varanneal_amd._build --force`" % (LIB_PATH, L.va_abi_version(), ABI_VERSION))
    L.va_last_error.restype = C.c_char_p
    L.va_device_count.argtypes = [c_ip]
    L.va_problem_create.argtypes = [C.POINTER(ProblemDesc), C.POINTER(h)]
    L.va_nnet_problem_create.argtypes = [C.POINTER(NnetDesc), C.POINTER(h)]
    L.va_rhs_load_module.argtypes = [C.c_char_p, c_ip]
    L.va_act_load_module.argtypes = [C.c_char_p, c_ip]
    L.va_eval_plan.argtypes = [C.POINTER(ProblemDesc), C.c_int32, C.c_int32, C.POINTER(C.c_int32)]
    L.va_eval_plan_reach.argtypes = [C.POINTER(ProblemDesc), C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.va_problem_destroy.argtypes = [h]
    L.va_problem_destroy.restype = None
    L.va_problem_info.argtypes = [h, c_lp, c_lp, c_ip, c_ip]
    L.va_action_grad.argtypes = [h, C.c_void_p, C.c_int64, C.c_int32, C.c_double, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    L.va_minimize_lbfgs.argtypes = [h, C.c_void_p, C.c_int64, C.c_int32, C.c_double,
                                    C.POINTER(LbfgsOpts), c_dp, c_dp, c_dp, c_ip, c_ip, c_lp]
    L.va_anneal.argtypes = [h, C.c_void_p, C.c_int64, C.c_int32, c_dp, C.c_int32,
                            C.POINTER(LbfgsOpts), c_dp, c_dp, c_ip, c_ip, c_lp, c_dp]
    L.va_get_minpath.argtypes = [h, C.c_int32, C.c_int32, c_dp]
    L.va_predict.argtypes = [h, c_dp, c_dp, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32, c_dp, c_dp]
    L.va_predict_tangent.argtypes = [h, c_dp, c_dp, c_dp, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32] + [c_dp] * 5
    L.va_predict_tangent.restype = C.c_int
    L.va_predict_adjoint.argtypes = [h, c_dp, c_dp, c_dp, c_dp, c_dp, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int32,
                                     C.c_int32] + [c_dp] * 5
    L.va_predict_adjoint.restype = C.c_int
    L.va_shoot.argtypes = [h, c_dp, c_dp, c_dp, c_dp, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32, c_dp, C.c_int32,
                           C.c_int64, C.c_int64, C.c_int32, C.c_double, C.c_double] + [c_dp] * 5 + [c_ip] * 3
    L.va_shoot.restype = C.c_int
    L.va_shoot_box.argtypes = [h, c_dp, c_dp, c_dp, c_dp, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_int32, c_dp, C.c_int32,
                               C.c_int64, C.c_int64, C.c_int32, C.c_double, C.c_double, c_dp, c_dp, C.c_int32] + [c_dp] * 5 + [c_ip] * 3
    L.va_shoot_box.restype = C.c_int
    L.va_lyapunov.argtypes = [h, c_dp, c_dp, c_dp, c_dp, C.c_int32, C.c_int32, C.c_double] + [C.c_int32] * 4 + [c_dp] * 5 + [c_ip]
    L.va_lyapunov.restype = C.c_int
    L.va_enkf.argtypes = [h, c_dp, c_dp, c_ip, C.c_int32, c_dp, c_dp, C.c_double, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int32,
                          C.c_int32] + [c_dp] * 7 + [c_ip]
    L.va_enkf.restype = C.c_int
    L.va_hess_vec.argtypes = [h, c_dp, c_dp, c_dp, C.c_int32, C.c_int32, C.c_int64, C.c_double, C.c_int32, C.c_int32, c_dp]
    L.va_hess_vec.restype = C.c_int
    L.va_blocktri_selinv.argtypes = [h, C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [c_dp] * 9 + [c_ip]
    L.va_blocktri_selinv.restype = C.c_int
    L.va_laplace.argtypes = [h, c_dp, c_dp, C.c_int32, C.c_int64, c_dp, C.c_int32, C.c_int32] + [c_dp] * 5 + [c_ip]
    L.va_laplace.restype = C.c_int
    L.va_hmc.argtypes = [h, C.c_void_p, C.c_int64, C.c_int32, C.c_double, C.c_int32, C.c_int32, c_dp, C.c_double, c_dp, C.c_int64,
                         C.c_uint64, c_dp, C.c_int32, c_lp, C.c_int32, c_dp, c_dp, c_dp, c_dp, c_ip, c_ip, c_dp]
    L.va_hmc.restype = C.c_int
    L.va_hmc_box.argtypes = [h, C.c_void_p, C.c_int64, C.c_int32, C.c_double, C.c_int32, C.c_int32, c_dp, C.c_double, c_dp, C.c_int64,
                             C.c_uint64, c_dp, C.c_int32, c_lp, C.c_int32, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp, c_dp, c_ip, c_ip, c_dp]
    L.va_hmc_box.restype = C.c_int
    L.va_hmc_box_map.argtypes = [C.c_int64] + [c_dp] * 7
    L.va_hmc_box_map.restype = C.c_int
    L.va_hmc_noise.argtypes = [C.c_uint64, C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_uint32), c_dp, c_dp]
    L.va_hmc_noise.restype = C.c_int
    L.va_eval_timed.argtypes = [h, C.c_double, C.c_int32, C.POINTER(C.c_float)]
    L.va_eval_timed_prepare.argtypes = [h, C.c_double, C.c_int32]
    L.va_get_counters.argtypes = [h, c_lp, c_lp, c_lp]
    L.va_comm_unique_id.argtypes = [C.c_char_p]
    L.va_comm_create.argtypes = [C.c_char_p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(h)]
    L.va_comm_destroy.argtypes = [h]
    L.va_comm_destroy.restype = None
    L.va_gather_results.argtypes = [h, h, C.c_int32, c_dp, c_ip]
    L.va_lbfgs_timed.argtypes = [h, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.va_eval_ls_timed.argtypes = [h, C.c_double, C.c_int32, C.POINTER(C.c_float)]
    L.va_read_eval_outputs.argtypes = [h, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    L.va_debug_read_partials.argtypes = [h, c_dp, C.c_int64]
    L.va_problem_eval_kernel.argtypes = [h, c_ip, c_ip]
    L.va_problem_eval_grid.argtypes = [h, c_ip, c_ip]
    L.va_problem_eval_grid.restype = C.c_int
    L.va_problem_tune.argtypes = [h, C.c_int32, C.c_int32]
    L.va_debug_read_persist.argtypes = [h, c_dp, C.c_int64]
    L.va_debug_read_persist.restype = C.c_int
    L.va_problem_persistent.argtypes = [h, c_ip, c_ip]
    L.va_problem_persistent.restype = C.c_int
    for fn in ("va_device_count", "va_rhs_load_module", "va_act_load_module", "va_eval_plan", "va_eval_plan_reach", "va_problem_eval_kernel", "va_problem_tune", "va_problem_create", "va_nnet_problem_create",
               "va_problem_info", "va_action_grad",
               "va_minimize_lbfgs", "va_anneal", "va_get_minpath", "va_predict", "va_eval_timed", "va_eval_timed_prepare",
               "va_get_counters", "va_debug_read_partials", "va_read_eval_outputs", "va_lbfgs_timed", "va_eval_ls_timed",
               "va_comm_unique_id", "va_comm_create", "va_gather_results"):
        getattr(L, fn).restype = C.c_int
    _lib = L
    return L


EXPORTS = ["va_abi_version", "va_last_error", "va_device_count", "va_rhs_load_module", "va_act_load_module", "va_eval_plan", "va_eval_plan_reach", "va_problem_eval_kernel", "va_problem_eval_grid", "va_problem_tune", "va_problem_create",
           "va_problem_destroy", "va_problem_info", "va_action_grad", "va_minimize_lbfgs",
           "va_anneal", "va_get_minpath", "va_predict", "va_predict_tangent", "va_predict_adjoint", "va_shoot", "va_shoot_box", "va_lyapunov", "va_enkf", "va_hess_vec", "va_blocktri_selinv", "va_laplace", "va_hmc", "va_hmc_box", "va_hmc_box_map", "va_hmc_noise", "va_eval_timed", "va_eval_timed_prepare", "va_problem_persistent", "va_debug_read_persist", "va_get_counters", "va_nnet_problem_create", "va_debug_read_partials",
           "va_read_eval_outputs", "va_lbfgs_timed", "va_eval_ls_timed", "va_comm_unique_id", "va_comm_create", "va_comm_destroy",
           "va_gather_results"]


def check(rc):
    if rc != VA_OK:
        raise (VaUnsupported if rc == VA_EUNSUPPORTED else VaError)(rc, lib().va_last_error().decode("utf-8", "replace"))


def eval_plan(batch, D, N_model, disc, ne, ghost=0, rm_array=False, rm_full=False, rf_array=False, rf_full=False,
              merr_nskip=1, tile_rows=0, eval_kernel=0, bounded=False, p_time_dependent=False, reach=None, Lidx=None,
              builtin=False):
    """(eval kernel 3 | 4 | 5, disc, K, w) of the column-run kernel instantiation a problem of this shape would run
    for a model with a column form of `ne` products per element and / or a ghosted form of `ghost` ghost
    columns (0 = the model has no such form), or None (flat kernel).  w: kernel 4 -- 1 for scalar weights;
    kernel 3 -- threads per workgroup.  reach = (xl, xr, gl, gr) of the column form and Lidx (the observed columns)
    let wide states pick the streaming kernel 5.  builtin: the plan of the built-in Lorenz-96 (a few instantiations exist
    for it alone: runs of 12 rows, the row-mask variant of merr_nskip); the default is a generated model's plan -- what
    va_ode.py asks for before it writes a module.  No GPU call (va_eval_plan / va_eval_plan_reach)."""
    d = ProblemDesc()
    d.struct_size = C.sizeof(ProblemDesc)
    d.rhs = 0 if builtin else 1000                        # VA_RHS_LORENZ96 / VA_RHS_USER_BASE
    d.batch, d.D, d.N_model, d.merr_nskip = batch, D, N_model, merr_nskip
    d.N_data = (N_model - 1) // merr_nskip + 1
    d.rm_kind = (2 if rm_full else 1) if rm_array else 0
    d.rf_kind = (2 if rf_full else 1) if rf_array else 0
    d.disc = DISC[disc] if isinstance(disc, str) else int(disc)
    d.tile_rows, d.eval_kernel = tile_rows, eval_kernel
    d.p_time_dependent = 1 if p_time_dependent else 0
    dummy = (C.c_double * 1)()
    if bounded:
        d.lower = C.cast(dummy, c_dp); d.upper = C.cast(dummy, c_dp)
    out = (C.c_int32 * 4)()
    if reach is not None and Lidx is not None and len(Lidx) > 0:
        li = np.ascontiguousarray(Lidx, dtype=np.int32)
        d.L = len(li)
        d.Lidx = li.ctypes.data_as(c_ip)
        r = (C.c_int32 * 4)(*[int(v) for v in reach])
        check(lib().va_eval_plan_reach(C.byref(d), int(ne), int(ghost), r, out))
    else:
        check(lib().va_eval_plan(C.byref(d), int(ne), int(ghost), out))
    return (out[0], out[1], out[2], out[3]) if out[0] else None


def hmc_noise(seed, chain, iteration, n):
    """What Problem.hmc's kernels draw for (seed, chain, iteration), from the device itself (va_hmc_noise): (words
    (n + 1, 4) uint32 -- the generator's words of the n elements and of the extra stream --, normals (n,), uniforms (2,):
    accept, jitter).  One row of hmc's `noise` is np.concatenate([normals, uniforms])."""
    n = int(n)
    words = np.empty((n + 1, 4), np.uint32); normals = np.empty(n); uniforms = np.empty(2)
    check(lib().va_hmc_noise(int(seed) & (2 ** 64 - 1), int(chain), int(iteration), n, words.ctypes.data_as(C.POINTER(C.c_uint32)),
                             normals.ctypes.data_as(c_dp), uniforms.ctypes.data_as(c_dp)))
    return words, normals, uniforms


def hmc_box_map(lower, upper, z):
    """The map of Problem.hmc_box entry by entry, from the device itself (va_hmc_box_map): lower, upper, z (n,) -- infinite
    bounds mean none -- give (x, dx/dz, d log|dx/dz| / dz, log|dx/dz|), each (n,)."""
    lo, hi, z = (np.ascontiguousarray(_f64(v).reshape(-1)) for v in (lower, upper, z))
    if not lo.size == hi.size == z.size:
        raise ValueError("hmc_box_map: lower, upper and z have one entry each per table row")
    out = [np.empty(z.size) for _ in range(4)]
    check(lib().va_hmc_box_map(z.size, *[a.ctypes.data_as(c_dp) for a in [lo, hi, z] + out]))
    return tuple(out)


_modules = {}


def load_rhs_module(path):
    """Register a generated right-hand-side module; returns its rhs id (cached per path)."""
    path = os.path.abspath(path)
    if path not in _modules:
        rid = C.c_int32()
        check(lib().va_rhs_load_module(path.encode(), C.byref(rid)))
        _modules[path] = rid.value
    return _modules[path]


_act_modules = {}


def load_act_module(path):
    """Register a generated activation module; returns its activation id (cached per path)."""
    path = os.path.abspath(path)
    if path not in _act_modules:
        aid = C.c_int32()
        check(lib().va_act_load_module(path.encode(), C.byref(aid)))
        _act_modules[path] = aid.value
    return _act_modules[path]


class Comm(object):
    """RCCL communicator of the job's one collective (va_comm_*): rank 0 makes the id with
    Comm.unique_id() and hands the 128 bytes to the other ranks."""

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        check(lib().va_comm_unique_id(buf))
        return buf.raw

    def __init__(self, uid, world, rank, device=0):
        self._L = lib()
        self.world, self.rank = world, rank
        self._c = C.c_void_p()
        check(self._L.va_comm_create(uid, world, rank, device, C.byref(self._c)))

    def close(self):
        if getattr(self, "_c", None) is not None and self._c.value:
            self._L.va_comm_destroy(self._c)
            self._c = C.c_void_p()

    __del__ = close


class Problem(object):
    """RAII wrapper of a va_handle; arrays are NumPy (host) or raw device pointers."""

    def __init__(self, batch, D, N_model, Y, Lidx, dt_model, RM, RF0, P, Pidx, **kw):
        self._L = lib()
        self.desc, self._keep = make_desc(batch, D, N_model, Y, Lidx, dt_model, RM, RF0, P, Pidx, **kw)
        self.B, self.D, self.N = batch, D, N_model
        self.NP, self.NPest = self.desc.NP, self.desc.NPest
        self.n_var = N_model * D + self.NPest
        if self.desc.p_time_dependent:
            # [X | p_est time-major]: to the shared solver one flat run without a parameter tail
            self.n_var = N_model * (D + self.NPest)
            self.NPe_t, self.NPt = self.NPest, self.NP
            self.N, self.D, self.NP, self.NPest = 1, self.n_var, 0, 0
        self.max_beta = self.desc.max_beta
        self._h = C.c_void_p()
        check(self._L.va_problem_create(C.byref(self.desc), C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.va_problem_destroy(self._h)
            self._h = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def info(self):
        nv, ld = C.c_int64(), C.c_int64()
        T, nt = C.c_int32(), C.c_int32()
        check(self._L.va_problem_info(self._h, C.byref(nv), C.byref(ld), C.byref(T), C.byref(nt)))
        ek, rr = C.c_int32(), C.c_int32()
        check(self._L.va_problem_eval_kernel(self._h, C.byref(ek), C.byref(rr)))
        # (k_eval4: tile_rows / ntiles describe a row group, the four waves that own one row of partial sums; a workgroup
        # runs row_groups of them and eval_grid workgroups make one launch)
        rg, wgs = C.c_int32(), C.c_int32()
        check(self._L.va_problem_eval_grid(self._h, C.byref(rg), C.byref(wgs)))
        return dict(n_var=nv.value, ld=ld.value, tile_rows=T.value, ntiles=nt.value, eval_kernel=ek.value,
                    run_rows=rr.value, row_groups=rg.value, eval_grid=wgs.value)

    TUNE = {"fold": 1, "grad_sc1": 2, "prio": 3, "graph": 4, "persist": 5, "persist_rows": 6, "nnet_fused": 7, "wide": 8}      # VA_TUNE_* of include/varanneal_amd.h

    def debug_read_persist(self, n):
        out = np.empty(n)
        check(self._L.va_debug_read_persist(self._h, out.ctypes.data_as(c_dp), n))
        return out

    def persistent(self):
        """(workgroups per seed, time rows per workgroup) when ladders on this handle run the persistent per-seed
        kernel (csrc/va_persist.h), else None"""
        g, t = C.c_int32(), C.c_int32()
        on = self._L.va_problem_persistent(self._h, C.byref(g), C.byref(t))
        return (g.value, t.value) if on else None

    def tune(self, **knobs):
        """performance knobs that change no result: fold= (tail inside the evaluation kernel), grad_sc1=, graph=,
        wide= (k_eval4's row groups per workgroup: 0 one (default), 1 the planner's rule, 2 / 3 that many); prio= is retired and ignored"""
        for k, v in knobs.items():
            check(self._L.va_problem_tune(self._h, self.TUNE[k], int(v)))

    def _xp(self, XP):
        XP = _f64(XP)
        if XP.shape != (self.B, self.n_var):
            raise ValueError("XP must have shape (B, N*D+NPest) = (%d, %d), got %s" %
                             (self.B, self.n_var, XP.shape))
        return XP

    def action_grad(self, XP, rf_scale=1.0, want_grad=True):
        XP = self._xp(XP)
        A = np.empty(self.B); me = np.empty(self.B); fe = np.empty(self.B)
        g = np.empty((self.B, self.n_var)) if want_grad else None
        check(self._L.va_action_grad(self._h, XP.ctypes.data, self.n_var, MEM_HOST, float(rf_scale),
                                     A.ctypes.data, me.ctypes.data, fe.ctypes.data,
                                     g.ctypes.data if want_grad else None, self.n_var))
        return A, me, fe, g

    def action_grad_device(self, xp_ptr, ld, rf_scale, A_ptr, me_ptr, fe_ptr, g_ptr, ldg):
        check(self._L.va_action_grad(self._h, xp_ptr, ld, MEM_DEVICE, float(rf_scale), A_ptr, me_ptr,
                                     fe_ptr, g_ptr, ldg))

    def minimize_lbfgs(self, XP, rf_scale, opt_args=None):
        XP = self._xp(XP).copy()
        o = make_opts(opt_args)
        A = np.empty(self.B); me = np.empty(self.B); fe = np.empty(self.B)
        st = np.empty(self.B, np.int32); nit = np.empty(self.B, np.int32); nfev = np.empty(self.B, np.int64)
        check(self._L.va_minimize_lbfgs(self._h, XP.ctypes.data, self.n_var, MEM_HOST, float(rf_scale),
                                        C.byref(o), A.ctypes.data_as(c_dp), me.ctypes.data_as(c_dp),
                                        fe.ctypes.data_as(c_dp), st.ctypes.data_as(c_ip),
                                        nit.ctypes.data_as(c_ip), nfev.ctypes.data_as(c_lp)))
        return dict(x=XP, A=A, me=me, fe=fe, status=st, nit=nit, nfev=nfev)

    def anneal(self, XP, rf_scale, opt_args=None, want_paths=False, xp_device=None, ld=None):
        rf = _f64(rf_scale)
        nb = rf.shape[0]
        o = make_opts(opt_args)
        B = self.B
        ame = np.empty((B, nb, 3)); pest = np.empty((B, nb, self.NPest))
        st = np.empty((B, nb), np.int32); nit = np.empty((B, nb), np.int32); nfev = np.empty((B, nb), np.int64)
        mp = np.empty((B, nb, self.N * self.D + self.NP)) if want_paths else None
        if xp_device is None:
            XP = self._xp(XP).copy()
            ptr, stride, mem = XP.ctypes.data, self.n_var, MEM_HOST
        else:
            ptr, stride, mem = xp_device, ld, MEM_DEVICE
        check(self._L.va_anneal(self._h, ptr, stride, mem, rf.ctypes.data_as(c_dp), nb, C.byref(o),
                                ame.ctypes.data_as(c_dp), pest.ctypes.data_as(c_dp),
                                st.ctypes.data_as(c_ip), nit.ctypes.data_as(c_ip),
                                nfev.ctypes.data_as(c_lp), mp.ctypes.data_as(c_dp) if want_paths else None))
        return dict(x=XP if xp_device is None else None, A=ame[:, :, 0], me=ame[:, :, 1],
                    fe=ame[:, :, 2], pest=pest, status=st, nit=nit, nfev=nfev, minpaths=mp)

    def predict(self, x0, p, n_steps, t0=0.0, substeps=1, every=1, stim=None):
        """Integrate the model forward from the T states x0 (T, D) with the full parameter vectors p (T, NP): classical
        RK4 at the fixed step dt_model / substeps on the device (va_predict).  stim: (n_steps + 1, n_stim), the stimulus at
        the model-step times from t0 on (models with a stimulus only).  Returns (T, n_steps // every + 1, D): the model
        steps 0, every, 2 every, ...; row 0 is x0."""
        if not isinstance(self.desc, ProblemDesc):
            raise NotImplementedError("predict: a network handle has no differential equation to integrate")
        D, NP = self.desc.D, self.desc.NP
        x0 = _f64(x0).reshape(-1, D)
        T = x0.shape[0]
        p = _f64(p).reshape(-1, NP) if NP else np.zeros((T, 0))
        if p.shape[0] == 1 and T > 1:
            p = np.ascontiguousarray(np.broadcast_to(p, (T, NP)))
        if p.shape[0] != T:
            raise ValueError("predict: %d states but %d parameter vectors" % (T, p.shape[0]))
        n_steps, substeps, every = int(n_steps), int(substeps), int(every)
        st = None
        if stim is not None:
            st = _f64(stim).reshape(max(n_steps, 0) + 1, -1)
            if st.shape[1] != self.desc.n_stim and self.desc.n_stim:
                raise ValueError("predict: the stimulus must have %d rows of %d column(s)" % (n_steps + 1, self.desc.n_stim))
        out = np.empty((T, n_steps // every + 1 if every >= 1 and n_steps >= 1 else 1, D))
        check(self._L.va_predict(self._h, x0.ctypes.data_as(c_dp), p.ctypes.data_as(c_dp), T, float(t0), n_steps, substeps,
                                 every, st.ctypes.data_as(c_dp) if st is not None else None, out.ctypes.data_as(c_dp)))
        return out

    def predict_tangent(self, x0, p, V0, n_steps, t0=0.0, substeps=1, every=1, stim=None, want=("dx", "var")):
        """predict() and, along the nvec directions V0 (T, nvec, D + NPest) of every trajectory ([state part | estimated
        parameters' part], or (nvec, D + NPest) for one trajectory), the tangent-linear model of the discrete RK4 map on the
        device (va_predict_tangent; csrc/va_predict_tlm.h).  Returns a dict: out (T, n_out, D), the nominal trajectories,
        and of want: dx (T, nvec, n_out, D), the tangents' state parts (row 0 is V0's); var (T, n_out, D), their squares
        summed over directions; cov (T, n_out, D, D), the same-time products summed over directions.  With V0 a square
        root of the covariance of (x0, p_est), var and cov are the linearised forecast covariance."""
        if not isinstance(self.desc, ProblemDesc):
            raise NotImplementedError("predict_tangent: a network handle has no differential equation to integrate")
        bad = set(want) - {"dx", "var", "cov"}
        if bad:
            raise ValueError("predict_tangent: want holds 'dx', 'var', 'cov', not %s" % sorted(bad))
        D, NP, nw = self.desc.D, self.desc.NP, self.desc.D + self.NPest
        x0 = _f64(x0).reshape(-1, D)
        T = x0.shape[0]
        p = _f64(p).reshape(-1, NP) if NP else np.zeros((T, 0))
        if p.shape[0] == 1 and T > 1:
            p = np.ascontiguousarray(np.broadcast_to(p, (T, NP)))
        if p.shape[0] != T:
            raise ValueError("predict_tangent: %d states but %d parameter vectors" % (T, p.shape[0]))
        V0 = _f64(V0)
        if V0.size == 0:
            raise ValueError("predict_tangent: at least one direction (nvec = 0)")
        if V0.shape[-1:] != (nw,) or V0.size % (T * nw):
            raise ValueError("predict_tangent: V0 must have shape (%d, nvec, D + NPest = %d), got %s" % (T, nw, V0.shape))
        V0 = V0.reshape(T, -1, nw)
        nvec = V0.shape[1]
        n_steps, substeps, every = int(n_steps), int(substeps), int(every)
        st = None
        if stim is not None:
            st = _f64(stim).reshape(max(n_steps, 0) + 1, -1)
            if st.shape[1] != self.desc.n_stim and self.desc.n_stim:
                raise ValueError("predict_tangent: the stimulus must have %d rows of %d column(s)" % (n_steps + 1, self.desc.n_stim))
        n_out = n_steps // every + 1 if every >= 1 and n_steps >= 1 else 1
        r = dict(out=np.empty((T, n_out, D)))
        for name, shape in (("dx", (T, nvec, n_out, D)), ("var", (T, n_out, D)), ("cov", (T, n_out, D, D))):
            if name in want:
                r[name] = np.empty(shape)
        ptr = lambda a: a.ctypes.data_as(c_dp) if a is not None else None
        check(self._L.va_predict_tangent(self._h, ptr(x0), ptr(p), ptr(V0), T, nvec, float(t0), n_steps, substeps, every, ptr(st),
                                         ptr(r["out"]), ptr(r.get("dx")), ptr(r.get("var")), ptr(r.get("cov"))))
        return r

    def predict_adjoint(self, x0, p, n_steps, G=None, Y=None, weights=None, t0=0.0, substeps=1, every=1, stim=None):
        """predict() and one backward sweep per cotangent set: the transpose of the derivative of the discrete RK4 map that
        predict_tangent applies, on the device (va_predict_adjoint; csrc/va_predict_adj.h).  Pass exactly one of
        G (T, ncot, n_out, D), or (ncot, n_out, D) for one trajectory: the cotangents of the output rows (cotangent mode), and
        Y (T, n_out, L) or (n_out, L), shared by the trajectories: observations of the handle's Lidx columns at the output rows,
        with weights (L,) (misfit mode: the cotangents are 2 w (x - y)).  Returns a dict: out (T, n_out, D), the nominal
        trajectories; gx0 (T, ncot, D) and gp (T, ncot, NPest), the gradients with respect to x0 and the estimated
        parameters; in misfit mode cost (T,) = sum w (x - y)^2.  The handle's bounds are ignored."""
        if not isinstance(self.desc, ProblemDesc):
            raise NotImplementedError("predict_adjoint: a network handle has no differential equation to integrate")
        if (G is None) == (Y is None):
            raise ValueError("predict_adjoint: pass exactly one of G (cotangent mode) and Y (misfit mode)")
        D, NP, NPe = self.desc.D, self.desc.NP, self.NPest
        x0 = _f64(x0).reshape(-1, D)
        T = x0.shape[0]
        p = _f64(p).reshape(-1, NP) if NP else np.zeros((T, 0))
        if p.shape[0] == 1 and T > 1:
            p = np.ascontiguousarray(np.broadcast_to(p, (T, NP)))
        if p.shape[0] != T:
            raise ValueError("predict_adjoint: %d states but %d parameter vectors" % (T, p.shape[0]))
        n_steps, substeps, every = int(n_steps), int(substeps), int(every)
        n_out = n_steps // every + 1 if every >= 1 and n_steps >= 1 else 1
        st = None
        if stim is not None:
            st = _f64(stim).reshape(max(n_steps, 0) + 1, -1)
            if st.shape[1] != self.desc.n_stim and self.desc.n_stim:
                raise ValueError("predict_adjoint: the stimulus must have %d rows of %d column(s)" % (n_steps + 1, self.desc.n_stim))
        w, shared, ncot = None, 0, 1
        if G is not None:
            G = _f64(G)
            if G.size == 0 or G.shape[-2:] != (n_out, D) or G.size % (T * n_out * D) or G.ndim not in (3, 4) or (G.ndim == 4 and G.shape[0] != T):
                raise ValueError("predict_adjoint: G must have shape (%d, ncot, n_out = %d, D = %d), got %s" % (T, n_out, D, G.shape))
            G = G.reshape(T, -1, n_out, D)
            ncot = G.shape[1]
        else:
            Ld = self.desc.L
            Y = _f64(Y)
            if Y.shape not in ((n_out, Ld), (T, n_out, Ld)):
                raise ValueError("predict_adjoint: Y must have shape (n_out = %d, L = %d) or (%d, %d, %d), got %s" % (n_out, Ld, T, n_out, Ld, Y.shape))
            shared = 1 if Y.ndim == 2 else 0
            if weights is None:
                raise ValueError("predict_adjoint: misfit mode takes weights of shape (L = %d,)" % Ld)
            w = _f64(weights)
            if w.shape != (Ld,):
                raise ValueError("predict_adjoint: weights must have shape (L = %d,), got %s" % (Ld, w.shape))
        if G is not None and weights is not None:
            raise ValueError("predict_adjoint: weights belong to misfit mode (Y)")
        r = dict(out=np.empty((T, n_out, D)), gx0=np.empty((T, ncot, D)), gp=np.empty((T, ncot, NPe)))
        if Y is not None:
            r["cost"] = np.empty(T)
        ptr = lambda a: a.ctypes.data_as(c_dp) if a is not None else None
        check(self._L.va_predict_adjoint(self._h, ptr(x0), ptr(p), ptr(G), ptr(Y), ptr(w), shared, T, ncot, float(t0), n_steps, substeps,
                                         every, ptr(st), ptr(r["out"]), ptr(r["gx0"]), ptr(r["gp"]), ptr(r.get("cost"))))
        return r

    def shoot(self, x0, p, n_steps, Y, weights, t0=0.0, substeps=1, every=1, stim=None, m=10, maxiter=15000, maxfun=15000, maxls=20,
              ftol=1e-15, gtol=1e-9):
        """Strong-constraint shooting on the device (va_shoot; csrc/va_shoot.h): from each of the T starts x0 (T, D) with the
        full parameter vectors p (T, NP), minimise predict_adjoint's misfit cost = sum w (x - y)^2 over x0 and the estimated
        parameters by L-BFGS -- SciPy's L-BFGS-B without bounds: m pairs, ftol, gtol, maxiter, maxfun, maxls -- every point's
        whole minimisation in one launch.  Y (T, n_out, L) or (n_out, L), weights (L,), t0, substeps, every, stim as in
        predict_adjoint.  Returns a dict: x0 (T, D), p (T, NP) the returned points (full vectors), cost, cost_start, grad_max
        (largest gradient entry at the returned point), nit, nfev, status (T,): 0 converged, 1 maxiter / maxfun, 2 abnormal
        line search, 3 non-finite cost at the start (the point comes back unchanged).  D <= 512; a handle with bounds is refused."""
        if not isinstance(self.desc, ProblemDesc):
            raise NotImplementedError("shoot: a network handle has no differential equation to integrate")
        D, NP, Ld = self.desc.D, self.desc.NP, self.desc.L
        x0 = _f64(x0).reshape(-1, D)
        T = x0.shape[0]
        p = _f64(p).reshape(-1, NP) if NP else np.zeros((T, 0))
        if p.shape[0] == 1 and T > 1:
            p = np.ascontiguousarray(np.broadcast_to(p, (T, NP)))
        if p.shape[0] != T:
            raise ValueError("shoot: %d states but %d parameter vectors" % (T, p.shape[0]))
        n_steps, substeps, every = int(n_steps), int(substeps), int(every)
        n_out = n_steps // every + 1 if every >= 1 and n_steps >= 1 else 1
        st = None
        if stim is not None:
            st = _f64(stim).reshape(max(n_steps, 0) + 1, -1)
            if st.shape[1] != self.desc.n_stim and self.desc.n_stim:
                raise ValueError("shoot: the stimulus must have %d rows of %d column(s)" % (n_steps + 1, self.desc.n_stim))
        Y = _f64(Y)
        if Y.shape not in ((n_out, Ld), (T, n_out, Ld)):
            raise ValueError("shoot: Y must have shape (n_out = %d, L = %d) or (%d, %d, %d), got %s" % (n_out, Ld, T, n_out, Ld, Y.shape))
        w = _f64(weights)
        if w.shape != (Ld,):
            raise ValueError("shoot: weights must have shape (L = %d,), got %s" % (Ld, w.shape))
        r = dict(x0=np.empty((T, D)), p=np.empty((T, NP)), cost=np.empty(T), cost_start=np.empty(T), grad_max=np.empty(T),
                 nit=np.empty(T, dtype=np.int32), nfev=np.empty(T, dtype=np.int32), status=np.empty(T, dtype=np.int32))
        ptr = lambda a: a.ctypes.data_as(c_dp) if a is not None else None
        iptr = lambda a: a.ctypes.data_as(c_ip)
        check(self._L.va_shoot(self._h, ptr(x0), ptr(p), ptr(Y), ptr(w), 1 if Y.ndim == 2 else 0, T, float(t0), n_steps, substeps, every,
                               ptr(st), int(m), int(maxiter), int(maxfun), int(maxls), float(ftol), float(gtol), ptr(r["x0"]), ptr(r["p"]),
                               ptr(r["cost"]), ptr(r["cost_start"]), ptr(r["grad_max"]), iptr(r["nit"]), iptr(r["nfev"]), iptr(r["status"])))
        return r

    def shoot_box(self, x0, p, n_steps, Y, weights, lower, upper, t0=0.0, substeps=1, every=1, stim=None, m=10, maxiter=15000,
                  maxfun=15000, maxls=20, ftol=1e-15, gtol=1e-9):
        """shoot() inside a box (va_shoot_box; csrc/va_shoot_box.h): the same misfit over x0 and the estimated parameters,
        subject to lower <= [x0 | p_est] <= upper, by L-BFGS-B (the published algorithm SciPy runs: generalised Cauchy point,
        subspace minimisation with the 3.0 projection step, dcsrch), every point's whole minimisation in one launch.
        lower, upper: (n,) for all points or (T, n), n = D + NPest: the D state columns, then the estimated parameters in
        Pidx order; None, -inf / +inf: no bound.  The start is projected onto the box; cost_start is the projected start's
        cost.  Returns shoot's dict; grad_max is the projected-gradient norm at the returned point, and every returned
        entry satisfies lower <= x <= upper exactly.  The handle's own bounds are not looked at: the caller's box is the box."""
        if not isinstance(self.desc, ProblemDesc):
            raise NotImplementedError("shoot_box: a network handle has no differential equation to integrate")
        D, NP, Ld, nv = self.desc.D, self.desc.NP, self.desc.L, self.desc.D + self.desc.NPest
        x0 = _f64(x0).reshape(-1, D)
        T = x0.shape[0]
        p = _f64(p).reshape(-1, NP) if NP else np.zeros((T, 0))
        if p.shape[0] == 1 and T > 1:
            p = np.ascontiguousarray(np.broadcast_to(p, (T, NP)))
        if p.shape[0] != T:
            raise ValueError("shoot_box: %d states but %d parameter vectors" % (T, p.shape[0]))
        n_steps, substeps, every = int(n_steps), int(substeps), int(every)
        n_out = n_steps // every + 1 if every >= 1 and n_steps >= 1 else 1
        st = None
        if stim is not None:
            st = _f64(stim).reshape(max(n_steps, 0) + 1, -1)
            if st.shape[1] != self.desc.n_stim and self.desc.n_stim:
                raise ValueError("shoot_box: the stimulus must have %d rows of %d column(s)" % (n_steps + 1, self.desc.n_stim))
        Y = _f64(Y)
        if Y.shape not in ((n_out, Ld), (T, n_out, Ld)):
            raise ValueError("shoot_box: Y must have shape (n_out = %d, L = %d) or (%d, %d, %d), got %s" % (n_out, Ld, T, n_out, Ld, Y.shape))
        w = _f64(weights)
        if w.shape != (Ld,):
            raise ValueError("shoot_box: weights must have shape (L = %d,), got %s" % (Ld, w.shape))

        def side(b, none, name):
            b = np.asarray(b, dtype=object)
            if b.shape not in ((nv,), (T, nv)):
                raise ValueError("shoot_box: %s must have shape (n = %d,) or (%d, %d), got %s" % (name, nv, T, nv, b.shape))
            return np.ascontiguousarray(np.where(np.equal(b, None), none, b).astype(np.float64))
        lo, hi = side(lower, -np.inf, "lower"), side(upper, np.inf, "upper")
        if lo.shape != hi.shape:
            raise ValueError("shoot_box: lower %s and upper %s must have the same shape" % (lo.shape, hi.shape))
        shared = lo.ndim == 1
        r = dict(x0=np.empty((T, D)), p=np.empty((T, NP)), cost=np.empty(T), cost_start=np.empty(T), grad_max=np.empty(T),
                 nit=np.empty(T, dtype=np.int32), nfev=np.empty(T, dtype=np.int32), status=np.empty(T, dtype=np.int32))
        ptr = lambda a: a.ctypes.data_as(c_dp) if a is not None else None
        iptr = lambda a: a.ctypes.data_as(c_ip)
        check(self._L.va_shoot_box(self._h, ptr(x0), ptr(p), ptr(Y), ptr(w), 1 if Y.ndim == 2 else 0, T, float(t0), n_steps, substeps,
                                   every, ptr(st), int(m), int(maxiter), int(maxfun), int(maxls), float(ftol), float(gtol), ptr(lo), ptr(hi),
                                   1 if shared else 0, ptr(r["x0"]), ptr(r["p"]), ptr(r["cost"]), ptr(r["cost_start"]), ptr(r["grad_max"]),
                                   iptr(r["nit"]), iptr(r["nfev"]), iptr(r["status"])))
        return r

    def lyapunov(self, x0, p, K, n_steps, t0=0.0, substeps=1, qr_every=1, n_skip=0, Q0=None, coupling=None, stim=None, trace=False):
        """Lyapunov spectra of the model on the device (va_lyapunov; csrc/va_lyap.h): from the T states x0 (T, D) with the
        full parameter vectors p (T, NP), K <= D tangents per trajectory carried by the tangent-linear RK4 map and
        re-orthonormalised by a QR every qr_every model steps (n_steps a multiple of it).  Q0 (T, K, D) or (K, D): the
        starting tangents (default: the first K unit vectors); coupling (T, D) or (D,): non-negative gains g, every tangent
        stage then J(x) v - g o v (conditional exponents); n_skip: QRs left out of the sums.  Returns a dict: logsum (T, K),
        the sums of log R_jj; exponents (T, K) = logsum / ((n_qr - n_skip) qr_every dt_model); x_end (T, D), Q_end (T, K, D);
        status (T,), 0 or j + 1 of the first R_jj that was zero or not finite (that row of logsum is NaN; nothing raises);
        and with trace=True trace (T, n_qr, K), every log R_jj."""
        if not isinstance(self.desc, ProblemDesc):
            raise NotImplementedError("lyapunov: a network handle has no differential equation to integrate")
        D, NP = self.desc.D, self.desc.NP
        x0 = _f64(x0).reshape(-1, D)
        T = x0.shape[0]
        p = _f64(p).reshape(-1, NP) if NP else np.zeros((T, 0))
        if p.shape[0] == 1 and T > 1:
            p = np.ascontiguousarray(np.broadcast_to(p, (T, NP)))
        if p.shape[0] != T:
            raise ValueError("lyapunov: %d states but %d parameter vectors" % (T, p.shape[0]))
        K, n_steps, substeps, qr_every, n_skip = int(K), int(n_steps), int(substeps), int(qr_every), int(n_skip)
        if K < 1 or K > D:
            raise ValueError("lyapunov: K=%d outside 1 .. D=%d" % (K, D))

        def per_traj(arr, shape, what):
            if arr is None:
                return None
            arr = _f64(arr)
            if arr.shape == shape:
                arr = np.broadcast_to(arr, (T,) + shape)
            if arr.shape != (T,) + shape:
                raise ValueError("lyapunov: %s must have shape %s or %s, got %s" % (what, (T,) + shape, shape, arr.shape))
            return np.ascontiguousarray(arr)
        Q0 = per_traj(Q0, (K, D), "Q0")
        coupling = per_traj(coupling, (D,), "coupling")
        st = None
        if stim is not None:
            st = _f64(stim).reshape(max(n_steps, 0) + 1, -1)
            if st.shape[1] != self.desc.n_stim and self.desc.n_stim:
                raise ValueError("lyapunov: the stimulus must have %d rows of %d column(s)" % (n_steps + 1, self.desc.n_stim))
        n_qr = n_steps // qr_every if qr_every >= 1 and n_steps >= 1 else 0
        r = dict(logsum=np.empty((T, K)), x_end=np.empty((T, D)), Q_end=np.empty((T, K, D)), status=np.zeros(T, dtype=np.int32))
        if trace:
            r["trace"] = np.empty((T, max(n_qr, 0), K))
        ptr = lambda a: a.ctypes.data_as(c_dp) if a is not None else None
        check(self._L.va_lyapunov(self._h, ptr(x0), ptr(p), ptr(Q0), ptr(coupling), T, K, float(t0), n_steps, substeps, qr_every, n_skip,
                                  ptr(st), ptr(r["logsum"]), ptr(r["x_end"]), ptr(r["Q_end"]), ptr(r.get("trace")),
                                  r["status"].ctypes.data_as(c_ip)))
        r["exponents"] = r["logsum"] / ((n_qr - n_skip) * qr_every * self.desc.dt_model)
        return r

    def enkf(self, x0, p, Y, obs_var, obs_every=1, est=(), inflation=1.0, t0=0.0, substeps=1, stim=None):
        """The ensemble Kalman filter of the model on the device (va_enkf; csrc/va_enkf.h): T points of M members, x0 (T, M, D)
        with the members' full parameter vectors p (T, M, NP) ((M, NP) and (NP,) are repeated), observations Y (T, n_obs, L) or
        (n_obs, L) for all points alike, of the handle's Lidx columns, NaN where one is missing; row k is at
        t0 + (k + 1) obs_every dt_model.  obs_var (L,) or a scalar: the observation error variances; est: the positions in p the
        filter updates; inflation >= 1 about the forecast mean.  Per row: obs_every model steps of every member (predict()'s
        RK4), then the serial ensemble square-root analysis.  Returns a dict: mean_f, sd_f, mean_a, sd_a (T, n_obs, D + len(est))
        of (x, p[est]) before and after each analysis; x_end (T, M, D), p_end (T, M, NP) to continue from; status (T,), 0 or
        k + 1 of the first row whose forecast was not finite (the statistics are NaN from there; nothing raises)."""
        if not isinstance(self.desc, ProblemDesc):
            raise NotImplementedError("enkf: a network handle has no differential equation to integrate")
        D, NP, Ld = self.desc.D, self.desc.NP, self.desc.L
        x0 = _f64(x0)
        if x0.ndim == 2:
            x0 = x0[None]
        if x0.ndim != 3 or x0.shape[2] != D:
            raise ValueError("enkf: x0 must have shape (T, M, D = %d), got %s" % (D, x0.shape))
        T, M = x0.shape[:2]
        p = _f64(p) if NP else np.zeros((T, M, 0))
        if p.shape[-1:] != (NP,) or p.shape not in ((NP,), (M, NP), (T, M, NP)):
            raise ValueError("enkf: p must have shape (%d, %d, NP = %d), (%d, %d) or (%d,), got %s" % (T, M, NP, M, NP, NP, p.shape))
        p = np.ascontiguousarray(np.broadcast_to(p, (T, M, NP)))
        Y = _f64(Y)
        if Y.ndim == 2:
            Y = np.broadcast_to(Y, (T,) + Y.shape)
        if Y.ndim != 3 or Y.shape[0] != T or Y.shape[2] != Ld:
            raise ValueError("enkf: Y must have shape (n_obs, L = %d) or (%d, n_obs, %d), got %s" % (Ld, T, Ld, Y.shape))
        Y = np.ascontiguousarray(Y)
        n_obs, obs_every, substeps = Y.shape[1], int(obs_every), int(substeps)
        ov = np.asarray(obs_var, dtype=np.float64)
        if ov.shape not in ((), (Ld,)):
            raise ValueError("enkf: obs_var must be a scalar or have shape (L = %d,), got %s" % (Ld, ov.shape))
        ov = np.ascontiguousarray(np.broadcast_to(ov, (Ld,)))
        est = np.ascontiguousarray(np.asarray(est, dtype=np.int32).reshape(-1))
        NV = D + est.size
        st = None
        if stim is not None:
            st = _f64(stim).reshape(max(n_obs * obs_every, 0) + 1, -1)
            if st.shape[1] != self.desc.n_stim and self.desc.n_stim:
                raise ValueError("enkf: the stimulus must have %d rows of %d column(s)" % (n_obs * obs_every + 1, self.desc.n_stim))
        r = dict(mean_f=np.empty((T, n_obs, NV)), sd_f=np.empty((T, n_obs, NV)), mean_a=np.empty((T, n_obs, NV)),
                 sd_a=np.empty((T, n_obs, NV)), x_end=np.empty((T, M, D)), p_end=np.empty((T, M, NP)), status=np.zeros(T, dtype=np.int32))
        ptr = lambda a: a.ctypes.data_as(c_dp) if a is not None else None
        check(self._L.va_enkf(self._h, ptr(x0), ptr(p), est.ctypes.data_as(c_ip) if est.size else None, est.size, ptr(Y), ptr(ov),
                              float(inflation), T, M, float(t0), n_obs, obs_every, substeps, ptr(st), ptr(r["mean_f"]), ptr(r["sd_f"]),
                              ptr(r["mean_a"]), ptr(r["sd_a"]), ptr(r["x_end"]), ptr(r["p_end"]), r["status"].ctypes.data_as(c_ip)))
        return r

    def hess_vec(self, XP, V, rf_scale, P=None, gauss_newton=False, tile_rows=0):
        """Hessian-vector products of the action on the device (va_hess_vec): XP (npts, n_var) points, V (npts, nvec, n_var)
        directions (or (nvec, n_var) for one point), both packed [X | p_est].  P: (npts, NP) or (NP,) full parameter vectors
        (estimated entries come from XP); default the handle's first seed's.  gauss_newton: 2 J^T W J only.  tile_rows: time
        rows per workgroup (0: the library's choice).  Returns (npts, nvec, n_var).  The handle's bounds are ignored, its
        resident state is left alone."""
        if not isinstance(self.desc, ProblemDesc):
            raise NotImplementedError("hess_vec: the network action has no second derivatives here (ODE handles only)")
        n = self.n_var
        XP = _f64(XP).reshape(-1, n)
        npts = XP.shape[0]
        V = _f64(V)
        one = V.ndim == 2 and npts == 1
        V = V.reshape(npts, -1, n)
        NP = self.desc.NP
        if P is None:
            P = np.ctypeslib.as_array(self.desc.P, shape=(NP,)) if (NP and not self.desc.p_time_dependent) else np.zeros(NP)
        P = _f64(P).reshape(-1, NP) if NP else np.zeros((npts, 0))
        if P.shape[0] == 1 and npts > 1:
            P = np.ascontiguousarray(np.broadcast_to(P, (npts, NP)))
        if P.shape[0] != npts:
            raise ValueError("hess_vec: %d points but %d parameter vectors" % (npts, P.shape[0]))
        HV = np.empty_like(V)
        check(self._L.va_hess_vec(self._h, XP.ctypes.data_as(c_dp), P.ctypes.data_as(c_dp), V.ctypes.data_as(c_dp), npts,
                                  V.shape[1], n, float(rf_scale), 1 if gauss_newton else 0, int(tile_rows), HV.ctypes.data_as(c_dp)))
        return HV[0] if one else HV

    def blocktri_selinv(self, Dk, Bk, Pk, Hpp, want=("Skk", "Snk", "Spk", "Spp")):
        """Selected inverse and log-determinant of npts block-tridiagonal matrices with a dense border, on the device
        (va_blocktri_selinv; csrc/va_selinv.h).  Dk (npts, K, W, W), Bk (npts, K - 1, W, W) the blocks H_{k+1,k}, Pk
        (npts, K, NPe, W), Hpp (npts, NPe, NPe); NPe = 0 is legal.  want: which blocks of the inverse come back (the others
        are not written).  Returns a dict of them plus logdet (npts,) and status (npts,): 0 fine, k + 1 / -1 where a
        matrix stopped being positive definite (its outputs are NaN)."""
        Dk = _f64(Dk)
        npts, K, W = Dk.shape[:3]
        Hpp = _f64(Hpp).reshape(npts, -1)
        NPe = int(round(np.sqrt(Hpp.shape[1])))
        Bk, Pk = _f64(Bk).reshape(npts, K - 1, W, W), _f64(Pk).reshape(npts, K, NPe, W)
        Hpp = Hpp.reshape(npts, NPe, NPe)
        out = {}
        for name, shape in (("Skk", Dk.shape), ("Snk", Bk.shape), ("Spk", Pk.shape), ("Spp", Hpp.shape)):
            if name in want:
                out[name] = np.empty(shape)
        out["logdet"], out["status"] = np.empty(npts), np.empty(npts, np.int32)
        ptr = lambda a: a.ctypes.data_as(c_dp) if a is not None and a.size else None
        check(self._L.va_blocktri_selinv(self._h, npts, K, W, NPe, ptr(Dk), ptr(Bk), ptr(Pk), ptr(Hpp), ptr(out.get("Skk")),
                                         ptr(out.get("Snk")), ptr(out.get("Spk")), ptr(out.get("Spp")),
                                         out["logdet"].ctypes.data_as(c_dp), out["status"].ctypes.data_as(c_ip)))
        return out

    def laplace(self, XP, rf_scale, P=None, gauss_newton=False, full=False, chunk_pts=0):
        """Laplace approximation at the points XP (npts, n_var), each with its own rf_scale (a scalar serves all), on the
        device (va_laplace): the coloured Hessian-vector products, the block-tridiagonal factor and the selected inverse.
        P as in hess_vec.  Returns a dict: var_x (npts, N, D), cov_pp (npts, NPest, NPest), logdet, status; with full=True
        also cov_xx (npts, N, D, D), the same-time blocks, and cov_px (npts, NPest, N D).  A point whose Hessian is not
        positive definite is NaN with status k + 1 (block k of the path) or -1 (the parameters' Schur complement).
        chunk_pts: points per chunk of device workspace (0: as many as stay under 1 GiB)."""
        if not isinstance(self.desc, ProblemDesc):
            raise NotImplementedError("laplace: the network action has no second derivatives here (ODE handles only)")
        n = self.n_var
        XP = _f64(XP).reshape(-1, n)
        npts = XP.shape[0]
        NP, NPe, N, D = self.desc.NP, self.NPest, self.N, self.D
        if P is None:
            P = np.ctypeslib.as_array(self.desc.P, shape=(NP,)) if (NP and not self.desc.p_time_dependent) else np.zeros(NP)
        P = _f64(P).reshape(-1, NP) if NP else np.zeros((npts, 0))
        if P.shape[0] == 1 and npts > 1:
            P = np.ascontiguousarray(np.broadcast_to(P, (npts, NP)))
        if P.shape[0] != npts:
            raise ValueError("laplace: %d points but %d parameter vectors" % (npts, P.shape[0]))
        rf = np.ascontiguousarray(np.broadcast_to(_f64(rf_scale).reshape(-1), (npts,)))
        out = dict(var_x=np.empty((npts, N, D)), cov_pp=np.empty((npts, NPe, NPe)), logdet=np.empty(npts),
                   status=np.empty(npts, np.int32))
        if full:
            out["cov_xx"], out["cov_px"] = np.empty((npts, N, D, D)), np.empty((npts, NPe, N * D))
        ptr = lambda a: a.ctypes.data_as(c_dp) if a is not None else None
        check(self._L.va_laplace(self._h, ptr(XP), ptr(P), npts, n, ptr(rf), 1 if gauss_newton else 0, int(chunk_pts),
                                 ptr(out["var_x"]), ptr(out.get("cov_xx")), ptr(out.get("cov_px")), ptr(out["cov_pp"]),
                                 ptr(out["logdet"]), out["status"].ctypes.data_as(c_ip)))
        return out

    def hmc(self, XP, rf_scale, n_iter, n_leap, eps, jitter=0.0, minv=None, seed=0, noise=None, thin=1, keep_idx=None):
        """B Hamiltonian Monte Carlo chains of exp(-A) at one rf_scale on the device (va_hmc; csrc/va_hmc.h), started at
        XP (B, n_var).  eps: a step size, or one per chain; minv: None (identity), (n_var,) or (B, n_var); noise: None (the
        generator keyed by `seed`) or (n_iter, B, n_var + 2) standard normals, accept uniform, jitter uniform; keep_idx:
        path-vector entries kept after every thin-th iteration.  Returns a dict: x (B, n_var) the final states, mean, var
        (B, n_var), A, dH, accepted (B, n_iter), n_divergent (B,), kept (B, n_iter // thin, len(keep_idx)).  The handle's
        resident state is left as found."""
        if not isinstance(self.desc, ProblemDesc):
            raise NotImplementedError("hmc: network handles are not sampled (ODE handles only)")
        XP = self._xp(XP).copy()
        B, n = self.B, self.n_var
        n_iter, n_leap, thin = int(n_iter), int(n_leap), int(thin)
        eps = np.ascontiguousarray(np.broadcast_to(_f64(eps).reshape(-1), (B,)))
        if minv is not None:
            minv = _f64(minv)
            if minv.shape not in [(n,), (B, n)]:
                raise ValueError("hmc: minv must have shape (n_var,) = (%d,) or (B, n_var) = (%d, %d), got %s" % (n, B, n, minv.shape))
        if noise is not None:
            noise = _f64(noise)
            if noise.shape != (max(n_iter, 0), B, n + 2):
                raise ValueError("hmc: noise must have shape (n_iter, B, n_var + 2) = (%d, %d, %d), got %s" % (n_iter, B, n + 2, noise.shape))
        keep = np.ascontiguousarray(np.zeros(0) if keep_idx is None else keep_idx, dtype=np.int64).reshape(-1)
        ni, nk = max(n_iter, 1), max(n_iter, 1) // max(thin, 1)
        out = dict(x=XP, mean=np.empty((B, n)), var=np.empty((B, n)), A=np.empty((B, ni)), dH=np.empty((B, ni)),
                   accepted=np.empty((B, ni), np.int32), n_divergent=np.empty(B, np.int32), kept=np.empty((B, nk, keep.size)))
        ptr = lambda a: a.ctypes.data_as(c_dp) if a is not None else None
        check(self._L.va_hmc(self._h, XP.ctypes.data, n, MEM_HOST, float(rf_scale), n_iter, n_leap, ptr(eps), float(jitter), ptr(minv),
                             0 if minv is None else minv.size, int(seed) & (2 ** 64 - 1), ptr(noise), thin, keep.ctypes.data_as(c_lp),
                             keep.size, ptr(out["mean"]), ptr(out["var"]), ptr(out["A"]), ptr(out["dH"]),
                             out["accepted"].ctypes.data_as(c_ip), out["n_divergent"].ctypes.data_as(c_ip), ptr(out["kept"])))
        return out

    def hmc_box(self, XP, rf_scale, n_iter, n_leap, eps, bounds=None, z0=None, jitter=0.0, minv=None, seed=0, noise=None, thin=1,
                keep_idx=None):
        """hmc() for box-bounded problems (va_hmc_box; csrc/va_hmc_box.h): the chains run in an unconstrained z with
        x = T(z) element by element, so every state lies inside its closed box and follows exp(-A) restricted to it.  bounds: one
        (lo, hi) per entry of the path vector (None: no bound on that side), shared by the chains; None: the handle's own.
        z0 (B, n_var): start in z instead of XP (the 'z' of an earlier result continues its chain without re-inverting
        x); a start in XP must lie strictly inside its box.  minv is the inverse mass OF z.  Returns hmc's dict (all of
        it about x) plus z (B, n_var), the final unconstrained state."""
        if not isinstance(self.desc, ProblemDesc):
            raise NotImplementedError("hmc_box: network handles are not sampled (ODE handles only)")
        XP = self._xp(XP).copy()
        B, n = self.B, self.n_var
        n_iter, n_leap, thin = int(n_iter), int(n_leap), int(thin)
        eps = np.ascontiguousarray(np.broadcast_to(_f64(eps).reshape(-1), (B,)))
        lo = hi = None
        if bounds is not None:
            if len(bounds) != n:
                raise ValueError("hmc_box: bounds must have one (lo, hi) pair per entry of the path vector (%d), got %d" % (n, len(bounds)))
            lo = np.array([-np.inf if b[0] is None else b[0] for b in bounds], dtype=np.float64)
            hi = np.array([np.inf if b[1] is None else b[1] for b in bounds], dtype=np.float64)
        if z0 is not None:
            z0 = _f64(z0)
            if z0.shape != (B, n):
                raise ValueError("hmc_box: z0 must have shape (B, n_var) = (%d, %d), got %s" % (B, n, z0.shape))
        if minv is not None:
            minv = _f64(minv)
            if minv.shape not in [(n,), (B, n)]:
                raise ValueError("hmc_box: minv must have shape (n_var,) = (%d,) or (B, n_var) = (%d, %d), got %s" % (n, B, n, minv.shape))
        if noise is not None:
            noise = _f64(noise)
            if noise.shape != (max(n_iter, 0), B, n + 2):
                raise ValueError("hmc_box: noise must have shape (n_iter, B, n_var + 2) = (%d, %d, %d), got %s" % (n_iter, B, n + 2, noise.shape))
        keep = np.ascontiguousarray(np.zeros(0) if keep_idx is None else keep_idx, dtype=np.int64).reshape(-1)
        ni, nk = max(n_iter, 1), max(n_iter, 1) // max(thin, 1)
        out = dict(x=XP, z=np.empty((B, n)), mean=np.empty((B, n)), var=np.empty((B, n)), A=np.empty((B, ni)), dH=np.empty((B, ni)),
                   accepted=np.empty((B, ni), np.int32), n_divergent=np.empty(B, np.int32), kept=np.empty((B, nk, keep.size)))
        ptr = lambda a: a.ctypes.data_as(c_dp) if a is not None else None
        check(self._L.va_hmc_box(self._h, XP.ctypes.data, n, MEM_HOST, float(rf_scale), n_iter, n_leap, ptr(eps), float(jitter), ptr(minv),
                                 0 if minv is None else minv.size, int(seed) & (2 ** 64 - 1), ptr(noise), thin, keep.ctypes.data_as(c_lp),
                                 keep.size, ptr(lo), ptr(hi), ptr(z0), ptr(out["z"]), ptr(out["mean"]), ptr(out["var"]), ptr(out["A"]),
                                 ptr(out["dH"]), out["accepted"].ctypes.data_as(c_ip), out["n_divergent"].ctypes.data_as(c_ip), ptr(out["kept"])))
        return out

    def eval_timed_prepare(self, rf_scale, iters):
        """arm the seeds and build / upload the hipGraph eval_timed(rf_scale, iters) replays (nothing timed)"""
        check(self._L.va_eval_timed_prepare(self._h, float(rf_scale), int(iters)))

    def eval_timed(self, rf_scale, iters):
        ms = C.c_float()
        check(self._L.va_eval_timed(self._h, float(rf_scale), int(iters), C.byref(ms)))
        return ms.value

    def gather_results(self, comm, nbeta):
        """va_gather_results: (table [world*B, nbeta, 3+NPest], status [world*B, nbeta]) on every rank"""
        n = comm.world * self.B
        table = np.empty((n, nbeta, 3 + self.NPest)); st = np.empty((n, nbeta), np.int32)
        check(self._L.va_gather_results(self._h, comm._c, nbeta, table.ctypes.data_as(c_dp), st.ctypes.data_as(c_ip)))
        return table, st

    def lbfgs_timed(self, iters):
        """(ms of `iters` k_update launches, ms of `iters` k_direction launches) with full histories;
        destroys the resident state."""
        a, b = C.c_float(), C.c_float()
        check(self._L.va_lbfgs_timed(self._h, int(iters), C.byref(a), C.byref(b)))
        return a.value, b.value

    def eval_ls_timed(self, rf_scale, iters):
        """ms of `iters` evaluation launches as a ladder cycle makes them (line-search trial points, line-search step
        in the tail); destroys the resident line-search state."""
        a = C.c_float()
        check(self._L.va_eval_ls_timed(self._h, float(rf_scale), int(iters), C.byref(a)))
        return a.value

    def read_eval_outputs(self, want_grad=True):
        """(A, me, fe, grad) as the last S1 evaluation (action_grad / eval_timed) left them on the device."""
        A = np.empty(self.B); me = np.empty(self.B); fe = np.empty(self.B)
        g = np.empty((self.B, self.n_var)) if want_grad else None
        check(self._L.va_read_eval_outputs(self._h, A.ctypes.data, me.ctypes.data, fe.ctypes.data,
                                           g.ctypes.data if want_grad else None, self.n_var))
        return A, me, fe, g

    def debug_partials(self, n):
        out = np.empty(n)
        check(self._L.va_debug_read_partials(self._h, out.ctypes.data_as(c_dp), n))
        return out

    def counters(self):
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        check(self._L.va_get_counters(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return dict(eval_launches=a.value, seed_evals=b.value, cycles=c.value)


def make_nnet_desc(batch, structure, data_in, data_out, Lidx, RM, RF0, P, Pidx, act="sigmoid",
                   lbfgs_m=10, max_beta=1, keep_paths=0, device=0, stream=None):
    """Fill a va_nnet_desc from what va_nnet.Annealer.anneal_init holds (va_nnet.py:288-450)."""
    st = np.ascontiguousarray(structure, dtype=np.int32)
    din = _f64(np.atleast_2d(data_in)); dout = _f64(np.atleast_2d(data_out))
    M = din.shape[0]
    lin = np.ascontiguousarray(Lidx[0], dtype=np.int32); lout = np.ascontiguousarray(Lidx[1], dtype=np.int32)
    if din.shape != (M, lin.size) or dout.shape != (M, lout.size):
        raise ValueError("data_in/data_out must have shapes (M, len(Lidx[0])) / (M, len(Lidx[1])), got %s / %s"
                         % (din.shape, dout.shape))
    rmm = None
    if isinstance(RM, (list, tuple, np.ndarray)) and np.ndim(RM[0] if len(RM) else 0) == 2:
        # [RMin, RMout] with full matrices (va_nnet.py:136-139)
        rmm = (_f64(RM[0]), _f64(RM[1]))
        if len(RM) != 2 or rmm[0].shape != (lin.size, lin.size) or rmm[1].shape != (lout.size, lout.size):
            raise ValueError("matrix RM must be [RMin (Lin x Lin), RMout (Lout x Lout)]")
        rm_in = rm_out = 0.0
    elif isinstance(RM, (list, tuple, np.ndarray)) and np.ndim(RM) > 0:
        RM = np.asarray(RM, dtype=np.float64)
        if RM.shape != (2,):
            raise ValueError("RM must be a scalar, [RM_in, RM_out] or two matrices (va_nnet.py:132-139)")
        rm_in, rm_out = float(RM[0]), float(RM[1])
    else:
        rm_in = rm_out = float(RM)
    if not isinstance(act, (int, np.integer)) and act not in ACTIVATION:      # int: an id from load_act_module
        raise NotImplementedError("activation %r is not built in (have %s)" % (act, sorted(ACTIVATION)))
    P = _f64(P)
    if P.ndim == 1:
        P = np.tile(P, (batch, 1))
    pidx = np.ascontiguousarray(Pidx, dtype=np.int32)
    d = NnetDesc()
    d.struct_size = C.sizeof(NnetDesc); d.device = device; d.batch = batch
    d.n_layers = st.size; d.structure = st.ctypes.data_as(c_ip); d.M = M
    d.L_in, d.L_out = lin.size, lout.size
    d.Lidx_in = lin.ctypes.data_as(c_ip); d.Lidx_out = lout.ctypes.data_as(c_ip)
    d.data_in = din.ctypes.data_as(c_dp); d.data_out = dout.ctypes.data_as(c_dp)
    d.rm_in, d.rm_out, d.rf0 = rm_in, rm_out, float(RF0)
    d.NP, d.NPest = P.shape[1], pidx.size
    d.Pidx = pidx.ctypes.data_as(c_ip); d.P = P.ctypes.data_as(c_dp)
    d.activation = int(act) if isinstance(act, (int, np.integer)) else ACTIVATION[act]; d.lbfgs_m = lbfgs_m; d.max_beta = max_beta; d.keep_paths = keep_paths
    d.stream = stream
    if rmm is not None:
        d.rm_in_matrix = rmm[0].ctypes.data_as(c_dp); d.rm_out_matrix = rmm[1].ctypes.data_as(c_dp)
    return d, (st, din, dout, lin, lout, P, pidx, rmm)


class NnetProblem(Problem):
    """va_handle of a feed-forward-network action; same S1/S2/S3 methods as Problem.  The
    path vector is [X (M*NDnet) | p_est]; `minpaths` rows from anneal() have that width."""

    def __init__(self, batch, structure, data_in, data_out, Lidx, RM, RF0, P, Pidx, **kw):
        self._L = lib()
        self.desc, self._keep = make_nnet_desc(batch, structure, data_in, data_out, Lidx, RM, RF0, P, Pidx, **kw)
        self.B = batch
        self.M, self.NDnet = self.desc.M, int(np.sum(structure))
        self.NDens = self.M * self.NDnet
        self.NP_net, self.NPest_net = self.desc.NP, self.desc.NPest
        self.n_var = self.NDens + self.NPest_net
        # to the shared solver the vector has no separate parameter tail
        self.N, self.D, self.NP, self.NPest = 1, self.n_var, 0, 0
        self.max_beta = self.desc.max_beta
        self._h = C.c_void_p()
        check(self._L.va_nnet_problem_create(C.byref(self.desc), C.byref(self._h)))
