"""va_ode.Annealer -- drop-in for `varanneal.va_ode.Annealer` on MI355X.

Same surface as the reference (varanneal/va_ode.py:43-905):

    set_model(f, D) / set_data(data, stim, t, nstart, N) / set_data_fromfile(...)
    anneal(X0, P0, alpha, beta_array, RM, RF0, Lidx, Pidx, dt_model=None,
           init_to_data=True, action='A_gaussian', disc='trapezoid',
           method='L-BFGS-B', bounds=None, opt_args=None, adolcID=0,
           track_paths=None, track_params=None, track_action_errors=None)
    anneal_init(...) / anneal_step()
    save_paths / save_params / save_action_errors / save_as_minAone
    attributes N_data, minpaths, A_array, me_array, fe_array, P, exitflags, ...

What differs underneath: the action, its gradient (hand-coded adjoint, no ADOL-C
tape -- `adolcID` is accepted and ignored) and the L-BFGS minimisation over the
whole RF ladder run as HIP kernels behind include/varanneal_amd.h; there is no
CPU fallback.  Extensions are keyword-only or shape-triggered so reference scripts
run unchanged:

  * batched seeds: pass X0 with shape (B, N_model, D) and P0 with shape (B, NP);
    every result array gains a leading B axis.  Seeds climb the ladder
    independently on the device.
  * `device=`, `verbose=`, `fused=` keyword-only arguments of anneal()/anneal_init().

A model function that is not one of the hand-written built-ins (varanneal_amd.rhs) is
traced once, differentiated symbolically and compiled into a device module
(varanneal_amd.codegen) -- including the reference's `f(t, x, (p, stim))` stimulus
convention (va_ode.py:345-375).

Time-dependent parameters (upstream: P0 of shape (N_model, NP) with a 2-D X0,
va_ode.py:170-188, 565-570) are supported for the discretisations that work upstream
(trapezoid, SimpsonHermite); the model then receives the rows' own parameters, p[:, k].
Here any subset Pidx may be estimated and bounds work (upstream's anneal_step and bounds
branches for this case are broken, va_ode.py:597-601, 715-732).  A batch uses P0 (B, N_model, NP).

Full measurement precision matrices (`RM` of shape (L,L) or (N_data,L,L), va_ode.py:149-152) and full
model-error precision matrices (`RF0` of shape (D,D) or (N_model-1,D,D), va_ode.py:211-217; contracted per
row, which is what upstream's Simpson-Hermite branch does and its other branches mean) are supported
(flat tile kernel).  Not implemented (raise NotImplementedError): user-defined action callables, method='LM'.
"""
from __future__ import print_function

import numpy as np

from . import _capi, rhs as _rhs
from ._ladder import LadderAnnealer

_DISCS = ("euler", "trapezoid", "SimpsonHermite", "forwardmap")


def hmc_box_inverse(X, lo, hi):
    """z with T(z) = X for the map of csrc/va_hmc_box.h, entry by entry (lo, hi (n_var,), infinite: no bound); X strictly
    inside.  One-sided: z = w - 1/w with w the distance to the bound; two-sided: z = u / sqrt((1 - u)(1 + u)),
    u = 2 (x - lo)/(hi - lo) - 1."""
    X = np.asarray(X, dtype=np.float64)
    has_lo, has_hi = np.isfinite(lo), np.isfinite(hi)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        w = np.where(has_lo, X - lo, hi - X)
        one = w - 1.0 / w
        u = 2.0 * (X - lo) / (hi - lo) - 1.0
        two = u / np.sqrt((1.0 - u) * (1.0 + u))
    return np.where(has_lo & has_hi, two, np.where(has_lo | has_hi, one, X))


def hmc_box_slope(Z, lo, hi):
    """dx/dz of the same map at Z"""
    Z = np.asarray(Z, dtype=np.float64)
    has_lo, has_hi = np.isfinite(lo), np.isfinite(hi)
    r = np.sqrt(Z * Z + 4.0)
    w = np.where(Z >= 0.0, (Z + r) / 2.0, 2.0 / (r - Z))
    q = np.sqrt(1.0 + Z * Z)
    with np.errstate(invalid="ignore", over="ignore"):
        two = (hi - lo) / (2.0 * (q * q * q))
    one = np.where(has_lo, w / r, -(w / r))
    return np.where(has_lo & has_hi, two, np.where(has_lo | has_hi, one, 1.0))


def hmc_box_pull_in(X, lo, hi):
    """(X with every entry on or outside a bound moved inside, how many per row): two-sided entries to 1e-6 (hi - lo) from
    the bound they crossed, one-sided ones to 1e-6 max(1, |bound|)"""
    X = np.array(X, dtype=np.float64)
    has_lo, has_hi = np.isfinite(lo), np.isfinite(hi)
    with np.errstate(invalid="ignore"):
        d_lo = np.where(has_hi, 1e-6 * (hi - lo), 1e-6 * np.maximum(1.0, np.abs(lo)))
        d_hi = np.where(has_lo, 1e-6 * (hi - lo), 1e-6 * np.maximum(1.0, np.abs(hi)))
        low, high = has_lo & (X <= lo), has_hi & (X >= hi)
        X = np.where(low, lo + d_lo, np.where(high, hi - d_hi, X))
    return X, (low | high).sum(axis=1)


def hmc_rescale_step(eps, accept_rate, target=0.8):
    """Warm-up rule of Annealer.sample: every chain's step size times 2^((rate - target) / (1 - target)) above the target
    acceptance rate and 2^((rate - target) / target) below it -- 1 at the target, monotone in the rate, never more than a
    factor 2 either way per block.  A pure function of (eps, accept_rate): new array, inputs untouched."""
    eps = np.asarray(eps, dtype=np.float64)
    rate = np.asarray(accept_rate, dtype=np.float64)
    if not 0.0 < target < 1.0 or np.any(rate < 0.0) or np.any(rate > 1.0) or np.any(~np.isfinite(rate)):
        raise ValueError("acceptance rates and the target lie in [0, 1] (target strictly inside)")
    d = rate - target
    return eps * np.exp2(np.where(d >= 0.0, d / (1.0 - target), d / target))


def kaplan_yorke(exponents):
    """Kaplan-Yorke dimension of a FULL spectrum in decreasing order (last axis): j + (l_1 + ... + l_j) / |l_{j+1}| with j the
    largest count whose sum is not negative; 0 when even l_1 is negative, the number of exponents when nothing contracts,
    NaN where an exponent is NaN."""
    lam = np.asarray(exponents, dtype=np.float64)
    K = lam.shape[-1]
    cs = np.cumsum(lam, axis=-1)
    j = np.sum(np.cumprod(cs >= 0.0, axis=-1), axis=-1)                          # leading run of non-negative partial sums
    jj = np.minimum(j, K - 1)
    head = np.where(j > 0, np.take_along_axis(cs, np.maximum(j - 1, 0)[..., None], axis=-1)[..., 0], 0.0)
    nxt = np.take_along_axis(lam, jj[..., None], axis=-1)[..., 0]
    with np.errstate(divide="ignore", invalid="ignore"):
        ky = np.where(j >= K, float(K), j + head / np.abs(nxt))
    return np.where(np.isnan(lam).any(axis=-1), np.nan, ky)[()]


class Annealer(LadderAnnealer):
    _print_exit_message = True

    def __init__(self):
        LadderAnnealer.__init__(self)
        self.stim = None

    # ------------------------------------------------------------------ model / data
    def set_model(self, f, D):
        """f(t, x, p) acting on time slices (va_ode.py:56-67), or a registry name."""
        self.f = f
        self.D = int(D)
        self._rhs_name = _rhs.recognise(f, self.D)

    def set_data_fromfile(self, data_file, stim_file=None, nstart=0, N=None):
        """va_ode.py:69-96 (which raises NameError upstream); here it simply works."""
        data = np.load(data_file) if data_file.endswith("npy") else np.loadtxt(data_file)
        stim = None
        if stim_file is not None:
            stim = np.load(stim_file) if stim_file.endswith("npy") else np.loadtxt(stim_file)
        self.set_data(data, stim=stim, nstart=nstart, N=N)

    def set_data(self, data, stim=None, t=None, nstart=0, N=None):
        """va_ode.py:98-124: with `t` given, `data` holds observations only; otherwise
        column 0 of `data` (and of `stim`) is time."""
        self.N_data = data.shape[0] if N is None else N
        sl = slice(nstart, nstart + self.N_data)
        if t is None:
            self.t_data = data[sl, 0]
            self.Y = data[sl, 1:]
            self.stim = stim[sl, 1:] if stim is not None else None
        else:
            self.t_data = t[sl]
            self.Y = data[sl]
            self.stim = stim[sl] if stim is not None else None
        self.dt_data = self.t_data[1] - self.t_data[0]

    # ------------------------------------------------------------------ annealing
    def anneal(self, X0, P0, alpha, beta_array, RM, RF0, Lidx, Pidx, dt_model=None,
               init_to_data=True, action='A_gaussian', disc='trapezoid',
               method='L-BFGS-B', bounds=None, opt_args=None, adolcID=0,
               track_paths=None, track_params=None, track_action_errors=None,
               *, device=None, verbose=True, fused=None, n_seeds=None, devices=None, gather=True,
               bounded_minimiser=None):
        """Full ladder (va_ode.py:459-528).  With no per-step tracking and the device
        minimiser, the whole ladder runs in one C-ABI call (`fused`).

        Keyword-only additions (reference scripts run unchanged without them):
          n_seeds  X0 / P0 carry `n_seeds` independent initial guesses on their leading axis.  Under an
                   initialised torch.distributed job (one process per GPU; backend "nccl" is RCCL) every
                   rank anneals the block [r*n/R, (r+1)*n/R) of them -- the reference's SGE array job
                   (examples/nnet_barimages/SGEcluster/submit_multiM.sh:14-30) without the cluster -- and
                   ONE all-gather leaves the per-seed tables of all seeds in `self.gathered` on every
                   rank.  A seed's results do not depend on how many ranks share the work.
          devices  device ordinals to use (rank r takes devices[r % len]); default LOCAL_RANK
          gather   False: skip the collective (`self.gathered` then holds this rank's seeds only)
          bounded_minimiser  with `bounds`: 'scipy' = SciPy's L-BFGS-B on the host around the device
                   evaluator, exactly the reference's call (_autodiffmin.py:85-86; one seed; the default
                   for a single seed); 'device' = L-BFGS-B itself on the device (generalised Cauchy point +
                   subspace minimisation, csrc/va_lbfgsb.hip): every seed at once, nothing leaves HBM, SciPy's
                   iterates step for step (the default for batched seeds)"""
        if n_seeds is not None:
            from . import parallel
            X0 = np.asarray(X0); P0 = np.asarray(P0, dtype=np.float64)
            if X0.ndim != 3 or X0.shape[0] != n_seeds or P0.shape[0] != n_seeds:
                raise ValueError("n_seeds=%d needs X0 of shape (n_seeds, N_model, D) and P0 with n_seeds rows" % n_seeds)
            rank, world = parallel.rank_world()
            lo, hi = parallel.seed_range(n_seeds, rank, world)
            self.n_seeds, self.seed_lo, self.seed_hi = n_seeds, lo, hi
            if device is None:
                device = parallel.local_device(devices, rank)
            local = None
            if hi > lo:
                # (views: init_to_data and the parameter write-back still reach the caller's arrays)
                self.anneal(X0[lo:hi], P0[lo:hi], alpha, beta_array, RM, RF0, Lidx, Pidx, dt_model,
                            init_to_data, action, disc, method, bounds, opt_args, adolcID,
                            track_paths, track_params, track_action_errors,
                            device=device, verbose=verbose, fused=fused, bounded_minimiser=bounded_minimiser)
                ND = self.N_model * self.D
                local = {"A": self._A, "me": self._me, "fe": self._fe, "params": self._mp[:, :, ND:],
                         "exitflags": self._flags, "nit": self._nit, "nfev": self._nfev}
            if world > 1 and gather:
                if local is None:                     # more ranks than seeds: an empty block still joins the collective
                    nb, npw = len(beta_array), P0.reshape(n_seeds, -1).shape[1]
                    local = {"A": np.zeros((0, nb)), "me": np.zeros((0, nb)), "fe": np.zeros((0, nb)),
                             "params": np.zeros((0, nb, npw)), "exitflags": np.zeros((0, nb), np.int8),
                             "nit": np.zeros((0, nb), np.int32), "nfev": np.zeros((0, nb), np.int64)}
                self.gathered = parallel.gather_tables(local, n_seeds, device=device)
            else:
                self.gathered = local
            return
        if device is None:
            device = 0
        if self.annealing_initialized is False:       # reference: flag is never set (va_ode.py:468,705)
            self.anneal_init(X0, P0, alpha, beta_array, RM, RF0, Lidx, Pidx, dt_model,
                             init_to_data, action, disc, method, bounds, opt_args, adolcID,
                             device=device, verbose=verbose, bounded_minimiser=bounded_minimiser)

        def track():
            if track_paths is not None:
                self.save_paths(track_paths['filename'], track_paths.get('dtype', np.float64),
                                track_paths.get('fmt', "%.8e"))
            if track_params is not None:
                self.save_params(track_params['filename'], track_params.get('dtype', np.float64),
                                 track_params.get('fmt', "%.8e"))
            if track_action_errors is not None:
                self.save_action_errors(track_action_errors['filename'],
                                        track_action_errors.get('cmpt', 0),
                                        track_action_errors.get('dtype', np.float64),
                                        track_action_errors.get('fmt', "%.8e"))
        tracking = any(t is not None for t in (track_paths, track_params, track_action_errors))
        self._run_ladder(fused, track if tracking else None)

    def anneal_init(self, X0, P0, alpha, beta_array, RM, RF0, Lidx, Pidx, dt_model=None,
                    init_to_data=True, action='A_gaussian', disc='trapezoid',
                    method='L-BFGS-B', bounds=None, opt_args=None, adolcID=0,
                    *, device=0, verbose=True, bounded_minimiser=None):
        """va_ode.py:531-705."""
        if method not in ('L-BFGS-B', 'NCG', 'LM', 'TNC'):
            print("ERROR: Optimization routine not recognized. Annealing not initialized.")
            return None
        if method == 'LM':
            raise NotImplementedError("method='LM' is dead code upstream (_autodiffmin.py:157)")
        self.method = method
        self.verbose = verbose
        if not hasattr(self, "f"):
            raise ValueError("set_model() has not been called")
        # separate dt_data and dt_model are not supported upstream with a stimulus (va_ode.py:544-547)
        if dt_model is not None and dt_model != self.dt_data and self.stim is not None:
            raise ValueError("Separate dt_data and dt_model currently not supported with an external stimulus.")
        if action != 'A_gaussian':
            raise NotImplementedError("only action='A_gaussian' is implemented")
        if disc not in _DISCS:
            raise ValueError("unknown discretisation %r (expected one of %s)" % (disc, _DISCS))
        self.disc_name = disc

        # time grid (va_ode.py:549-558)
        if dt_model is None:
            self.dt_model = self.dt_data
            self.N_model = self.N_data
            self.merr_nskip = 1
            self.t_model = np.copy(self.t_data)
        else:
            self.dt_model = dt_model
            self.merr_nskip = int(self.dt_data / self.dt_model)
            self.N_model = (self.N_data - 1) * self.merr_nskip + 1
            self.t_model = np.linspace(self.t_data[0], self.t_data[-1], self.N_model)
        self.opt_args = opt_args

        # seeds / parameters
        X0 = np.asarray(X0)
        P0 = np.asarray(P0, dtype=np.float64)
        self._batched = X0.ndim == 3
        if self._batched:
            if P0.ndim not in (2, 3) or P0.shape[0] != X0.shape[0]:
                raise ValueError("batched X0 (B,N,D) needs P0 of shape (B,NP), or (B,N_model,NP) for "
                                 "time-dependent parameters")
            self.B = X0.shape[0]
            self._tdp = P0.ndim == 3
        else:
            if P0.ndim not in (1, 2):
                raise ValueError("P0 must be 1-D (static) or (N_model, NP) (time-dependent, va_ode.py:565-570)")
            self.B = 1
            self._tdp = P0.ndim == 2
        if self._tdp:
            # upstream's euler / forwardmap branches slice p one row short (va_ode.py:345-349,
            # 443-447 against :174-175): only the discretisations that work there are offered
            if disc not in ("trapezoid", "SimpsonHermite"):
                raise NotImplementedError("time-dependent parameters with disc=%r (inconsistent upstream)" % disc)
            if P0.shape[-2] != self.N_model:
                raise ValueError("time-dependent P0 must have N_model = %d rows" % self.N_model)
        if X0.shape[-2:] != (self.N_model, self.D):
            raise ValueError("X0 must have shape (N_model, D) = (%d, %d)" % (self.N_model, self.D))
        self.P = P0                                   # reference keeps a reference to the caller's array
        self.NP = P0.shape[-1]
        self.Pidx = list(Pidx)
        self.NPest = len(self.Pidx)
        self.Lidx = list(Lidx)
        self.L = len(self.Lidx)
        if np.shape(self.Y)[1] != self.L:
            raise ValueError("data has %d observed columns but Lidx has %d entries" % (np.shape(self.Y)[1], self.L))
        stim = None
        if self.stim is not None:
            stim = np.asarray(self.stim, dtype=np.float64)
        colparams = None
        if self._rhs_name is not None and stim is None:
            impl, NPr, _ = _rhs.REGISTRY[self._rhs_name]
            if self.NP == NPr:
                rhs_id = self._rhs_name
            elif callable(self.f):
                # the built-in model called with a parameter vector (e.g. Lorenz-96 with a forcing per site): only the
                # built-in kernels need exactly NPr parameters -- the callable is generated, in column-parameter form
                rhs_id, colparams = None, True
            else:
                raise ValueError("RHS %r takes %d parameter(s), P0 has %d" % (self._rhs_name, NPr, self.NP))
        else:
            rhs_id = None                             # any other callable: a generated module, built below
                                                      # once the weights and bounds (its kernel variant) are known

        # RM / RF0 broadcasting (va_ode.py:612-640)
        if isinstance(RM, list):
            RM = np.array(RM)
        if isinstance(RM, np.ndarray) and RM.ndim > 0:
            if RM.shape == (self.L,):
                self.RM = np.resize(RM, (self.N_data, self.L))
            elif RM.shape == (self.N_data, self.L):
                self.RM = RM
            elif RM.shape == (self.L, self.L):
                self.RM = np.resize(RM, (self.N_data, self.L, self.L))      # va_ode.py:617-618
            elif RM.shape == (self.N_data, self.L, self.L):
                self.RM = RM
            else:
                raise ValueError("ERROR: RM has an invalid shape.")
        else:
            self.RM = float(RM)
        if isinstance(RF0, list):
            RF0 = np.array(RF0)
        if isinstance(RF0, np.ndarray) and RF0.ndim > 0:
            if RF0.shape == (self.D,):
                self.RF0 = np.resize(RF0, (self.N_model - 1, self.D))
            elif RF0.shape == (self.N_model - 1, self.D):
                self.RF0 = RF0
            elif RF0.shape == (self.D, self.D):
                # full matrices (va_ode.py:631-632): diff_n . (RF_n . diff_n) per time step, as upstream's
                # Simpson-Hermite branch contracts them (:211-217; the other branch, :218-222, slips to the
                # whole diff array -- the per-row contraction is what is computed for every discretisation)
                self.RF0 = np.resize(RF0, (self.N_model - 1, self.D, self.D))
            elif RF0.shape == (self.N_model - 1, self.D, self.D):
                self.RF0 = RF0
            else:
                raise ValueError("ERROR: RF0 has an invalid shape.")
        else:
            self.RF0 = float(RF0)

        # ladder (va_ode.py:643-650; beta is truncated to uint16 upstream, kept)
        self._ladder_init(alpha, np.array(beta_array, dtype=np.uint16))

        # bounds (va_ode.py:582-605): expanded exactly as upstream, used by the SciPy route
        if bounds is not None:
            state_b, param_b = list(bounds[:self.D]), list(bounds[self.D:])
            self.bounds = [state_b[i] for _ in range(self.N_model) for i in range(self.D)]
            # (upstream's time-dependent branch, va_ode.py:597-601, names undefined variables;
            # this is what it means: the parameter bounds repeated for every time point)
            self.bounds += [param_b[i] for _ in range(self.N_model if self._tdp else 1) for i in range(self.NPest)]
        else:
            self.bounds = None
        if bounded_minimiser is None:
            # L-BFGS-B itself on the device (csrc/va_lbfgsb.hip follows SciPy's iterates step for step:
            # tests/test_gpu_codegen.py); 'scipy' keeps SciPy on the host around the device evaluator
            bounded_minimiser = 'device'
        if bounded_minimiser not in ('scipy', 'device'):
            raise ValueError("bounded_minimiser must be 'scipy' or 'device'")
        self._device_bounds = bounds is not None and method == 'L-BFGS-B' and bounded_minimiser == 'device'
        self._device_minimiser = (method == 'L-BFGS-B' and (bounds is None or self._device_bounds))
        if not self._device_minimiser and self.B != 1:
            raise ValueError("NCG / TNC / bounded_minimiser='scipy' run SciPy on the host around the device "
                             "evaluator: one seed only")

        # initial path (va_ode.py:666-693); init_to_data overwrites the caller's X0 in place, as upstream
        if init_to_data is True:
            X0[..., ::self.merr_nskip, self.Lidx] = self.Y[:]
        Xf = np.reshape(np.asarray(X0, dtype=np.float64), (self.B, self.N_model * self.D))
        npw = self.N_model * self.NP if self._tdp else self.NP          # stored parameter block, time-major
        Pf = np.reshape(P0, (self.B, npw))
        # positions of the estimated entries inside that block, in path-vector order (va_ode.py:183-188)
        self._estpos = ([n * self.NP + k for n in range(self.N_model) for k in self.Pidx] if self._tdp
                        else list(self.Pidx))
        self._alloc_tables(Xf, Pf)
        self.adolcID = adolcID                        # accepted, unused: there is no tape

        if rhs_id is None:
            # trace the callable, differentiate it, emit HIP, compile a module.  A model with a column form
            # (codegen.column_form: stencils, small dense systems) or a ghosted form (codegen.ghost_form: wide
            # stencils) also gets the ONE instantiation of the column-run kernel this problem's geometry calls
            # for (va_eval_plan) -- the kernels the built-in Lorenz-96 runs on
            from . import codegen
            nstim = 0 if stim is None else (1 if stim.ndim == 1 else stim.shape[1])

            def variant(ne, ghost, reach=None):
                return _capi.eval_plan(self.B, self.D, self.N_model, disc, ne, ghost,
                                        rm_array=isinstance(self.RM, np.ndarray), rm_full=np.ndim(self.RM) == 3,
                                        rf_array=isinstance(self.RF0, np.ndarray), rf_full=np.ndim(self.RF0) == 3,
                                        merr_nskip=self.merr_nskip,
                                        bounded=self._device_bounds, p_time_dependent=self._tdp,
                                        reach=reach, Lidx=self.Lidx)
            mod = codegen.module_for(self.f, self.D, self.NP, nstim, 1 if stim is None else stim.ndim,
                                     p_rows=self._tdp, col_variant=variant, colparams=colparams)
            rhs_id = _capi.load_rhs_module(mod["so"])
            self._rhs_module = mod

        # device image
        self.close()
        self._pb = _capi.Problem(self.B, self.D, self.N_model, np.asarray(self.Y, dtype=np.float64),
                                 self.Lidx, float(self.dt_model), self.RM, self.RF0,
                                 self._Pfull.reshape(self.B, self.N_model, self.NP) if self._tdp else self._Pfull,
                                 self.Pidx, disc=disc, rhs=rhs_id, merr_nskip=self.merr_nskip,
                                 p_time_dependent=self._tdp,
                                 t_model=np.asarray(self.t_model, dtype=np.float64), stim=stim,
                                 lbfgs_m=int((opt_args or {}).get("maxcor", 10)),
                                 max_beta=self.Nbeta, keep_paths=1, device=device,
                                 bounds=self.bounds if self._device_bounds else None)
        self.initalized = True                        # sic (va_ode.py:705)

    def _fused_paths(self, k0, mp):
        if self._tdp:                                 # rows come back as [X | p_est], time-major
            LadderAnnealer._fused_paths(self, k0, mp)
        else:                                         # full [X | P] rows
            self._mp[:, k0:] = mp

    def _fused_summary(self, k0, dt):
        for k in range(k0, self.Nbeta):
            print('Step %d of %d  beta = %d  RF = %.8e  exit flag = %s  iterations = %s  A = %s'
                  % (k + 1, self.Nbeta, self.beta_array[k],
                     float(np.ravel(self.RF0)[0]) * self._rf_scale[k],
                     self._view(self._flags)[..., k], self._view(self._nit)[..., k],
                     self._view(self._A)[..., k]))
        print('')
        LadderAnnealer._fused_summary(self, k0, dt)

    # ------------------------------------------------------------------ forecast
    def _select(self, beta, seeds):
        """(seed indices, rung indices) of a selection: None = all; an int or a sequence of ints otherwise"""
        def pick(sel, n, what):
            idx = np.arange(n) if sel is None else np.atleast_1d(np.asarray(sel, dtype=np.intp))
            if idx.ndim != 1 or np.any(idx < -n) or np.any(idx >= n):
                raise IndexError("%s selection %r outside [0, %d)" % (what, sel, n))
            return idx % n
        if seeds is not None and not self._batched:
            raise ValueError("seeds= selects from a batch; this run has one seed")
        return pick(seeds, self.B, "seed"), pick(beta, self.Nbeta, "rung")

    def predict(self, n_steps, beta=None, seeds=None, substeps=1, every=1, stim=None):
        """Forecast from the estimates (after anneal()): the model integrated n_steps steps of dt_model forward from the
        LAST row of every selected (seed, rung)'s minimising path, with that rung's full parameter vector (the last row's
        with time-dependent parameters), t0 = t_model[-1]: classical RK4 at dt_model / substeps, on the device, all
        selected trajectories in one call.
          beta / seeds  indices into beta_array / the batch (an int or a sequence); None = all
          every         keep the model steps 0, every, 2 every, ...: n_out = n_steps // every + 1 rows, row 0 the last fitted state
          stim          (n_steps + 1, n_stim): the stimulus at t_model[-1] + n dt_model, for models that take one
        Returns (nbeta_sel, n_out, D), or (B_sel, nbeta_sel, n_out, D) for a batch."""
        if self._pb is None or not getattr(self, "initalized", False):
            raise ValueError("predict() works after anneal() / anneal_init()")
        sb, kb = self._select(beta, seeds)
        N, D, NP, NX = self.N_model, self.D, self.NP, self._NX
        rows = self._mp[sb][:, kb]                                   # (B_sel, nbeta_sel, NX + stored parameter block)
        x0 = rows[:, :, (N - 1) * D:N * D]
        p = rows[:, :, NX + (N - 1) * NP:NX + N * NP] if self._tdp else rows[:, :, NX:]
        out = self._pb.predict(x0.reshape(-1, D), p.reshape(-1, NP), n_steps, t0=float(self.t_model[-1]),
                               substeps=substeps, every=every, stim=stim)
        out = out.reshape(len(sb), len(kb), out.shape[1], D)
        return out if self._batched else out[0]

    def predict_vjp(self, G, n_steps, beta=None, seeds=None, substeps=1, every=1, stim=None):
        """Sensitivity of a forecast functional to the estimate: one backward sweep through predict()'s RK4 steps per
        cotangent set (csrc/va_predict_adj.h: the transpose of the derivative of the DISCRETE RK4 map).  G holds dJ / d(forecast
        row): (ncot, n_out, D) for every selected point alike, or with predict()'s leading axes in front.  Selection and the
        other arguments as predict().  Returns a dict: out, predict()'s forecast; gx0 (..., ncot, D) = dJ / d(last fitted
        state); gp (..., ncot, NPest) = dJ / d(estimated parameters).  Time-dependent parameters: NotImplementedError."""
        if self._pb is None or not getattr(self, "initalized", False):
            raise ValueError("predict_vjp() works after anneal() / anneal_init()")
        if self._tdp:
            raise NotImplementedError("predict_vjp: time-dependent parameters are not carried")
        sb, kb = self._select(beta, seeds)
        N, D, NP, NX = self.N_model, self.D, self.NP, self._NX
        npts = len(sb) * len(kb)
        rows = self._mp[sb][:, kb].reshape(npts, -1)
        G = np.asarray(G, dtype=np.float64)
        if G.ndim == 3:
            G = np.broadcast_to(G, (npts,) + G.shape)
        G = np.ascontiguousarray(G.reshape((npts, -1) + G.shape[-2:]))
        r = self._pb.predict_adjoint(rows[:, (N - 1) * D:N * D], rows[:, NX:], n_steps, G=G, t0=float(self.t_model[-1]),
                                     substeps=substeps, every=every, stim=stim)
        lead = (len(sb), len(kb)) if self._batched else (len(kb),)
        return {k: v.reshape(lead + v.shape[1:]) for k, v in r.items()}

    SHOOT_OPT_ARGS = dict(ftol=1e-15, gtol=1e-9)

    def _shoot_weights(self):
        """weights (L,) with which va_predict_adjoint's cost is the action's measurement term as the package normalises it"""
        if np.ndim(self.RM) == 3:
            raise NotImplementedError("shoot: full RM matrices are not carried (the adjoint kernel's misfit takes one weight "
                                      "per observed column)")
        if isinstance(self.RM, np.ndarray):
            if np.any(self.RM != self.RM[:1]):
                raise NotImplementedError("shoot: RM changes along the data window; the adjoint kernel's misfit takes one "
                                          "weight per observed column")
            w = np.array(self.RM[0], dtype=np.float64)
        else:
            w = np.full(self.L, float(self.RM))
        return w / (self.L * self.N_data)

    _SHOOT_DEVICE_OPTS = dict(ftol="ftol", gtol="gtol", maxiter="maxiter", maxfun="maxfun", maxcor="m", maxls="maxls")

    def shoot(self, beta=-1, seeds=None, substeps=1, opt_args=None, device=False, box=False):
        """The RF -> infinity limit, done exactly: strong-constraint 4D-Var refinement of the selected (seed, rung)s.  A
        stored minimiser is a path, not a model orbit; this fits an actual model trajectory x(t; x(t_0), p) to the data
        window.  From the first row of the stored minimiser and that rung's parameters, SciPy's L-BFGS-B (host, one point at a
        time, the annealer's state and parameter bounds passed on) minimises over x(t_0) and the estimated parameters the
        measurement term of the model trajectory -- the action's, as the package normalises it -- whose value and gradient
        come from ONE device call per evaluation: the adjoint of the RK4 predictor in misfit mode (csrc/va_predict_adj.h).
        Returns a dict with predict()'s leading axes: x0 (..., D), params (..., NP) the full vectors, path (..., N, D) the
        model trajectory (predict()'s bits), cost, cost_start, grad_norm (largest gradient entry at the end), nfev, status
        (SciPy's: 0 converged), path_distance: the RMS distance between the annealed path and the trajectory -- how far
        from a model orbit that rung still is.  opt_args are SciPy's options on top of SHOOT_OPT_ARGS (the cost carries the
        action's 1 / (L N_data), and SciPy's default ftol, relative to max(|f|, 1), would stop a well-fitted trajectory at
        decreases of 2e-9).  Time-dependent parameters and full RM matrices: NotImplementedError.
        device=True: the minimiser runs on the device too -- all selected (seed, rung)s go through ONE Problem.shoot call
        (csrc/va_shoot.h: every point's L-BFGS from the first evaluation to the last inside one launch), then one predict()
        call for path.  The same keys, shapes and meanings, plus nit (iterations); nfev counts the kernel's evaluations;
        status 1 budget, 2 abnormal line search, 3 non-finite cost at the start.  opt_args: ftol, gtol, maxiter, maxfun,
        maxcor, maxls (any other key: ValueError).  Annealer bounds: NotImplementedError unless box=True; D <= 512.
        device=True, box=True: the device minimiser is L-BFGS-B (csrc/va_shoot_box.h, Problem.shoot_box): the annealer's
        bounds on x(t_0) and on the estimated parameters -- self.bounds[:D] + self.bounds[NX:NX + NPest], what the host route
        hands SciPy -- are one box for all selected points, in ONE shoot_box call, then one predict() call.  The same keys as
        device=True; the start is projected onto the box (cost_start is the projected start's cost), grad_norm is the
        projected-gradient norm, every returned entry lies inside its bounds exactly.  An annealer without bounds runs
        with an all-infinite box.  box=True without device=True: ValueError."""
        if box and not device:
            raise ValueError("shoot(box=True) is the device route's L-BFGS-B: pass device=True (device=False already hands the bounds to SciPy)")
        if device:
            return self._shoot_device(beta, seeds, substeps, opt_args, box)
        from scipy.optimize import minimize
        if self._pb is None or not getattr(self, "initalized", False):
            raise ValueError("shoot() works after anneal() / anneal_init()")
        if self._tdp:
            raise NotImplementedError("shoot: time-dependent parameters have no single model trajectory to fit")
        w = self._shoot_weights()
        sb, kb = self._select(beta, seeds)
        N, D, NP, NPe, NX = self.N_model, self.D, self.NP, self.NPest, self._NX
        Y = np.ascontiguousarray(self.Y, dtype=np.float64)
        stim = None if self.stim is None else np.asarray(self.stim, dtype=np.float64)
        t0, every, Pidx = float(self.t_model[0]), self.merr_nskip, list(self.Pidx)
        bounds = None
        if self.bounds is not None:
            bounds = list(self.bounds[:D]) + list(self.bounds[NX:NX + NPe])
        rows = self._mp[sb][:, kb].reshape(len(sb) * len(kb), -1)
        res = dict(x0=[], params=[], path=[], cost=[], cost_start=[], grad_norm=[], nfev=[], status=[], path_distance=[])
        for row in rows:
            P = np.array(row[NX:NX + NP])

            def fun(z):
                P[Pidx] = z[D:]
                r = self._pb.predict_adjoint(z[:D], P, N - 1, Y=Y, weights=w, t0=t0, substeps=substeps, every=every, stim=stim)
                return float(r["cost"][0]), np.append(r["gx0"][0, 0], r["gp"][0, 0])
            z0 = np.append(row[:D], P[Pidx])
            c0 = fun(z0)[0]
            opt = minimize(fun, z0, method="L-BFGS-B", jac=True, bounds=bounds, options=dict(self.SHOOT_OPT_ARGS, **(opt_args or {})))
            c1, g1 = fun(opt.x)
            path = self._pb.predict(opt.x[:D], P, N - 1, t0=t0, substeps=substeps, stim=stim)[0]
            res["x0"].append(opt.x[:D]); res["params"].append(P.copy()); res["path"].append(path)
            res["cost"].append(c1); res["cost_start"].append(c0); res["grad_norm"].append(np.abs(g1).max())
            res["nfev"].append(opt.nfev + 2); res["status"].append(opt.status)
            res["path_distance"].append(np.sqrt(np.mean((row[:NX].reshape(N, D) - path) ** 2)))
        lead = (len(sb), len(kb)) if self._batched else (len(kb),)
        out = {}
        for k, v in res.items():
            v = np.array(v, dtype=np.int64 if k in ("nfev", "status") else np.float64)
            out[k] = v.reshape(lead + v.shape[1:])
        return out

    def _shoot_device(self, beta, seeds, substeps, opt_args, box=False):
        if self._pb is None or not getattr(self, "initalized", False):
            raise ValueError("shoot() works after anneal() / anneal_init()")
        if self._tdp:
            raise NotImplementedError("shoot: time-dependent parameters have no single model trajectory to fit")
        if self.bounds is not None and not box:
            raise NotImplementedError("shoot(device=True): bounds are not carried by the unbounded device minimiser (it takes no "
                                      "projected step); pass box=True for L-BFGS-B on the device, or use device=False")
        kw = {}
        for k, v in dict(self.SHOOT_OPT_ARGS, **(opt_args or {})).items():
            if k not in self._SHOOT_DEVICE_OPTS:
                raise ValueError("shoot(device=True): option %r is not carried (known: %s)" % (k, ", ".join(sorted(self._SHOOT_DEVICE_OPTS))))
            kw[self._SHOOT_DEVICE_OPTS[k]] = v
        w = self._shoot_weights()
        sb, kb = self._select(beta, seeds)
        N, D, NP, NX = self.N_model, self.D, self.NP, self._NX
        stim = None if self.stim is None else np.asarray(self.stim, dtype=np.float64)
        t0 = float(self.t_model[0])
        rows = self._mp[sb][:, kb].reshape(len(sb) * len(kb), -1)
        if box:
            bounds = [(None, None)] * (D + self.NPest)
            if self.bounds is not None:
                bounds = list(self.bounds[:D]) + list(self.bounds[NX:NX + self.NPest])
            r = self._pb.shoot_box(rows[:, :D], rows[:, NX:NX + NP], N - 1, np.ascontiguousarray(self.Y, dtype=np.float64), w,
                                   [b[0] for b in bounds], [b[1] for b in bounds], t0=t0, substeps=substeps, every=self.merr_nskip,
                                   stim=stim, **kw)
        else:
            r = self._pb.shoot(rows[:, :D], rows[:, NX:NX + NP], N - 1, np.ascontiguousarray(self.Y, dtype=np.float64), w, t0=t0,
                               substeps=substeps, every=self.merr_nskip, stim=stim, **kw)
        path = self._pb.predict(r["x0"], r["p"], N - 1, t0=t0, substeps=substeps, stim=stim)
        res = dict(x0=r["x0"], params=r["p"], path=path, cost=r["cost"], cost_start=r["cost_start"], grad_norm=r["grad_max"],
                   nfev=r["nfev"], nit=r["nit"], status=r["status"],
                   path_distance=np.sqrt(np.mean((rows[:, :NX].reshape(-1, N, D) - path) ** 2, axis=(1, 2))))
        lead = (len(sb), len(kb)) if self._batched else (len(kb),)
        out = {}
        for k, v in res.items():
            v = np.array(v, dtype=np.int64 if k in ("nfev", "nit", "status") else np.float64)
            out[k] = v.reshape(lead + v.shape[1:])
        return out

    def prediction_error(self, Y_future, **predict_kwargs):
        """RMS error of the forecast against held-back observations: Y_future (n_out, L), the Lidx columns at the output
        times of predict(n_steps = (n_out - 1) * every, ...), row 0 being the last fitted time (not counted).  Per
        (seed, rung): shape (nbeta_sel,), or (B_sel, nbeta_sel) for a batch."""
        Yf = np.asarray(Y_future, dtype=np.float64)
        if Yf.ndim != 2 or Yf.shape[0] < 2 or Yf.shape[1] != self.L:
            raise ValueError("Y_future must have shape (n_out >= 2, L = %d), got %s" % (self.L, Yf.shape))
        every = int(predict_kwargs.get("every", 1))
        if "n_steps" not in predict_kwargs:
            predict_kwargs = dict(predict_kwargs, n_steps=(Yf.shape[0] - 1) * every)
        pred = self.predict(**predict_kwargs)
        if pred.shape[-2] != Yf.shape[0]:
            raise ValueError("the forecast has %d output rows, Y_future %d" % (pred.shape[-2], Yf.shape[0]))
        diff = pred[..., 1:, self.Lidx] - Yf[1:]
        return np.sqrt(np.mean(diff * diff, axis=(-2, -1)))

    # ------------------------------------------------------------------ second derivatives at the minimisers
    def _minimiser(self, beta, seed):
        """(xp [n_var], P [NP], rf_scale) of the stored minimiser of (seed, rung)"""
        if self._pb is None or not getattr(self, "initalized", False):
            raise ValueError("second derivatives are taken at the minimisers: call anneal() first")
        if self._tdp:
            raise NotImplementedError("hess_vec: time-dependent parameters are not carried")
        sb, kb = self._select([beta], [seed] if self._batched else None)
        row = self._mp[sb[0], kb[0]]
        P = np.array(row[self._NX:])
        return np.concatenate([row[:self._NX], P[self.Pidx]]), P, float(self._rf_scale[kb[0]])

    def hess_vec(self, V, beta=-1, seed=0, gauss_newton=False):
        """(d^2 A / d[X | p_est]^2) V at the stored minimiser of (seed, rung beta), with that rung's RF, on the device
        (csrc/va_hvp.h).  V: (n_var,) or (nvec, n_var), packed like the path vector.  gauss_newton: 2 J^T W J only."""
        xp, P, rf = self._minimiser(beta, seed)
        V = np.asarray(V, dtype=np.float64)
        out = self._pb.hess_vec(xp[None, :], V.reshape(1, -1, xp.size), rf, P=P[None, :], gauss_newton=gauss_newton)[0]
        return out[0] if V.ndim == 1 else out

    def _hessian_blocks(self, beta, seed, gauss_newton):
        """(ab, H_xp, H_pp): the path block in SciPy's upper banded layout (ab[u + i - j, j] = H[i, j], u = (hb + 1) D - 1
        superdiagonals), the border (N D, NPest) and the parameter block.  ONE batched call of (2 hb + 1) D + NPest
        directions: the Hessian couples time rows at most hb apart (hb = 1; 2 for Simpson-Hermite), so the rows n with
        equal n mod (2 hb + 1) are probed together -- coloured direction c has ones at all path entries (n, j) with
        (n mod (2 hb + 1)) D + j == c -- plus one unit direction per estimated parameter."""
        N, D, NPe = self.N_model, self.D, self.NPest
        hb = 2 if self.disc_name == "SimpsonHermite" else 1
        nc, ND = 2 * hb + 1, N * D
        V = np.zeros((nc * D + NPe, ND + NPe))
        rows = np.arange(N)
        for c in range(nc * D):
            V[c, (rows[rows % nc == c // D]) * D + c % D] = 1.0
        V[nc * D + np.arange(NPe), ND + np.arange(NPe)] = 1.0
        HV = self.hess_vec(V, beta=beta, seed=seed, gauss_newton=gauss_newton)
        u = (hb + 1) * D - 1
        ab = np.zeros((u + 1, ND))
        for n in range(N):
            for j in range(D):
                col = HV[(n % nc) * D + j]                     # column (n, j) of H on the rows within hb of n
                lo = max(0, n - hb) * D
                i = np.arange(lo, n * D + j + 1)               # upper triangle
                ab[u + i - (n * D + j), n * D + j] = col[i]
        H_xp = HV[nc * D:, :ND].T.copy()                       # (the parameter rows of the coloured products are discarded)
        H_pp = HV[nc * D:, ND:].copy()
        return ab, H_xp, 0.5 * (H_pp + H_pp.T)

    def action_hessian(self, beta=-1, seed=0, gauss_newton=False, form='dense'):
        """The Hessian of the action at the stored minimiser of (seed, rung), assembled from one batched device call
        (see hess_vec).  form='banded': (ab, H_xp, H_pp) with ab in SciPy's upper banded layout; form='dense': the
        (n_var, n_var) matrix (ValueError past 2 GiB)."""
        if form not in ('dense', 'banded'):
            raise ValueError("form must be 'dense' or 'banded'")
        n = self.N_model * self.D + self.NPest
        if form == 'dense' and 8.0 * n * n > 2.0 * 1024 ** 3:
            raise ValueError("the dense Hessian of %d variables takes %.1f GiB (> 2 GiB): ask for form='banded'"
                             % (n, 8.0 * n * n / 1024 ** 3))
        ab, H_xp, H_pp = self._hessian_blocks(beta, seed, gauss_newton)
        if form == 'banded':
            return ab, H_xp, H_pp
        ND, u = self.N_model * self.D, ab.shape[0] - 1
        H = np.zeros((n, n))
        for k in range(u + 1):                                # superdiagonal k
            d = ab[u - k, k:]
            H[np.arange(ND - k), np.arange(k, ND)] = d
            H[np.arange(k, ND), np.arange(ND - k)] = d
        H[:ND, ND:] = H_xp
        H[ND:, :ND] = H_xp.T
        H[ND:, ND:] = H_pp
        return H

    def param_covariance(self, beta=-1, seeds=None, gauss_newton=False):
        """Laplace approximation of the estimated parameters' covariance at the stored minimisers: the parameter block
        of the inverse Hessian, (H_pp - H_px H_xx^-1 H_xp)^-1, with H_xx factored in banded form (SciPy).  It is the
        inverse Hessian of the action AS THE PACKAGE NORMALISES IT (measurement term / (L N_data), model term /
        (D (N - 1))): for a negative log-likelihood A' = c A the covariance is this one divided by c.
        Returns (NPest, NPest), or (B_sel, NPest, NPest) for a batch.  numpy.linalg.LinAlgError if H_xx is not positive
        definite (not at a minimum, or a flat direction): gauss_newton=True is positive semi-definite by construction."""
        import scipy.linalg as sla
        sb, _ = self._select(None, seeds)
        out = []
        for b in sb:
            ab, H_xp, H_pp = self._hessian_blocks(beta, int(b), gauss_newton)
            try:
                cb = sla.cholesky_banded(ab, lower=False)
            except np.linalg.LinAlgError as e:
                raise np.linalg.LinAlgError("the path block of the Hessian (seed %d) is not positive definite (%s): not a minimum, "
                                            "or a flat direction; gauss_newton=True gives the positive semi-definite part" % (b, e))
            S = H_pp - np.dot(H_xp.T, sla.cho_solve_banded((cb, False), H_xp))
            try:
                out.append(np.linalg.inv(S))
            except np.linalg.LinAlgError as e:
                raise np.linalg.LinAlgError("the Schur complement H_pp - H_px H_xx^-1 H_xp (seed %d) is singular (%s): the data do "
                                            "not determine the estimated parameters at this point" % (b, e))
        out = np.array(out)
        return out if self._batched else out[0]

    def laplace(self, beta=None, seeds=None, gauss_newton=False, full=False):
        """Laplace approximation at the stored minimisers of every selected (seed, rung), each with its own rung's RF, in
        ONE device call (va_laplace; csrc/va_selinv.h): the Hessian from coloured Hessian-vector products, its
        block-tridiagonal Cholesky factor with the parameter border carried along, and the inverse on the factor's own
        sparsity pattern.  Returns a dict:
          state_var   (..., N, D)          marginal variance of every state, observed or not
          param_cov   (..., NPest, NPest)  what param_covariance computes on the host
          logdet      (...)                log det H: with the action value, the evidence of a minimiser
          status      (...)                0, or where the Hessian stopped being positive definite: k + 1 in block k of the
                                           path (hb = 1 time row per block, 2 with Simpson-Hermite), -1 in the parameters'
                                           Schur complement; the other entries of such a point are NaN.  Never raises for it.
        and with full=True also
          state_cov        (..., N, D, D)        the same-time covariance blocks
          state_param_cov  (..., NPest, N, D)    covariance of parameters and states.
        Leading axes as predict(): (nbeta_sel,), or (B_sel, nbeta_sel) for a batch.  beta / seeds: an int or a sequence;
        None = all.  It is the inverse Hessian of the action AS THE PACKAGE NORMALISES IT (measurement term / (L N_data),
        model term / (D (N - 1))): for a negative log-likelihood A' = c A the covariances are these divided by c, and
        logdet grows by n_var log c.  States wider than 64 (32 with Simpson-Hermite) or more than 32 estimated parameters:
        NotImplementedError; param_covariance's host route remains."""
        if self._pb is None or not getattr(self, "initalized", False):
            raise ValueError("second derivatives are taken at the minimisers: call anneal() first")
        if self._tdp:
            raise NotImplementedError("laplace: time-dependent parameters are not carried")
        sb, kb = self._select(beta, seeds)
        N, D, NPe, NX = self.N_model, self.D, self.NPest, self._NX
        rows = self._mp[sb][:, kb].reshape(len(sb) * len(kb), -1)                # (points, NX + NP)
        P = np.ascontiguousarray(rows[:, NX:])
        XP = np.concatenate([rows[:, :NX], P[:, self.Pidx]], axis=1)
        rf = np.tile(np.asarray(self._rf_scale, dtype=np.float64)[kb], len(sb))
        r = self._pb.laplace(XP, rf, P=P, gauss_newton=gauss_newton, full=full)
        lead = (len(sb), len(kb)) if self._batched else (len(kb),)
        out = dict(state_var=r["var_x"].reshape(lead + (N, D)), param_cov=r["cov_pp"].reshape(lead + (NPe, NPe)),
                   logdet=r["logdet"].reshape(lead), status=r["status"].reshape(lead))
        if full:
            out["state_cov"] = r["cov_xx"].reshape(lead + (N, D, D))
            out["state_param_cov"] = r["cov_px"].reshape(lead + (NPe, N, D))
        return out

    def state_stderr(self, beta=-1, seeds=None, gauss_newton=False):
        """One standard deviation of every estimated state at the selected rung(s): sqrt(laplace()['state_var']), shape
        (nbeta_sel, N, D) or (B_sel, nbeta_sel, N, D); NaN where the Hessian is not positive definite."""
        return np.sqrt(self.laplace(beta=beta, seeds=seeds, gauss_newton=gauss_newton)["state_var"])

    def _laplace_factor(self, beta, seeds, gauss_newton):
        """(seed indices, rung indices, status (npts,), F (npts, D + NPest, D + NPest)): one laplace(full=True) call gives the joint
        covariance Sigma_0 of the last fitted state and the estimated parameters of every selected point (the last time row's
        blocks of state_cov and state_param_cov, and param_cov); F is its lower Cholesky factor (host), zeros where there is
        none: status is laplace()'s, or -2 where Sigma_0 has no factor."""
        lap = self.laplace(beta=beta, seeds=seeds, gauss_newton=gauss_newton, full=True)
        sb, kb = self._select(beta, seeds)
        N, D, NPe = self.N_model, self.D, self.NPest
        npts, nw = len(sb) * len(kb), D + NPe
        status = np.array(lap["status"], dtype=np.int32).reshape(npts)
        Sxx = lap["state_cov"].reshape(npts, N, D, D)[:, N - 1]
        Spx = lap["state_param_cov"].reshape(npts, NPe, N, D)[:, :, N - 1]
        Spp = lap["param_cov"].reshape(npts, NPe, NPe)
        F = np.zeros((npts, nw, nw))
        for j in range(npts):
            if status[j] != 0:
                continue
            S0 = np.empty((nw, nw))
            S0[:D, :D], S0[D:, :D], S0[:D, D:], S0[D:, D:] = Sxx[j], Spx[j], Spx[j].T, Spp[j]
            try:
                if not np.all(np.isfinite(S0)):
                    raise np.linalg.LinAlgError("not finite")
                F[j] = np.linalg.cholesky(S0)
            except np.linalg.LinAlgError:
                status[j] = -2
        return sb, kb, status, F

    def predict_spread(self, n_steps, beta=None, seeds=None, substeps=1, every=1, stim=None, gauss_newton=False, full=False):
        """The forecast of predict() with its error bar: the LINEARISED spread of the model forecast under the Laplace
        posterior of every selected (seed, rung).  One laplace(full=True) call gives the joint covariance Sigma_0 of the
        last fitted state and the estimated parameters (the last time row's blocks of state_cov and state_param_cov, and
        param_cov); the columns of its Cholesky factor (host; at most 96 x 96) are carried along the forecast by the
        tangent-linear model of the RK4 integrator, all selected points in one device call (csrc/va_predict_tlm.h), and
        summed: the covariance at output row n is M_n Sigma_0 M_n^T, M_n the derivative of the forecast with respect to
        (x_{N-1}, p_est).  Returns a dict:
          mean    (..., n_out, D)      predict()'s output
          std     (..., n_out, D)      one standard deviation of every forecast state; row 0 is state_stderr()'s last row
          status  (...)                laplace()'s status, or -2 where Sigma_0 has no Cholesky factor; std (and cov) of such
                                       a point are NaN, its mean is the forecast as usual.  Never raises for it.
        and with full=True also
          cov     (..., n_out, D, D)   the same-time covariance blocks.
        Arguments and leading axes as predict(); gauss_newton as laplace().  What this is and is not: a linearisation, valid
        while the spread is small against the attractor (tangents of a chaotic model grow without bound; the true spread
        saturates); the covariance of the action AS THE PACKAGE NORMALISES IT (see laplace(): for a negative
        log-likelihood A' = c A divide variances by c); the spread of the MODEL forecast only -- no observation noise is
        added, so held-back data scatter around the band by their own error as well.  Refusals as laplace(): before
        anneal() ValueError; time-dependent parameters, states wider than 64 (32 with Simpson-Hermite) or more than 32
        estimated parameters NotImplementedError."""
        sb, kb, status, F = self._laplace_factor(beta, seeds, gauss_newton)
        N, D, NP, NPe, NX = self.N_model, self.D, self.NP, self.NPest, self._NX
        npts, nw = len(sb) * len(kb), D + NPe
        V0 = np.ascontiguousarray(F.transpose(0, 2, 1))                  # direction c of point j: column c of the factor
        rows = self._mp[sb][:, kb].reshape(npts, -1)
        r = self._pb.predict_tangent(rows[:, (N - 1) * D:N * D], rows[:, NX:], V0, n_steps, t0=float(self.t_model[-1]),
                                     substeps=substeps, every=every, stim=stim, want=("var", "cov") if full else ("var",))
        lead = (len(sb), len(kb)) if self._batched else (len(kb),)
        n_out = r["out"].shape[1]
        bad = status != 0
        std = np.sqrt(r["var"])
        std[bad] = np.nan
        out = dict(mean=r["out"].reshape(lead + (n_out, D)), std=std.reshape(lead + (n_out, D)), status=status.reshape(lead))
        if full:
            cov = np.array(r["cov"])
            cov[bad] = np.nan
            out["cov"] = cov.reshape(lead + (n_out, D, D))
        return out

    # ------------------------------------------------------------------ Lyapunov spectra of the fitted model
    def _lyap_points(self, n_steps, k, beta, seeds, qr_every, transient, what):
        """the selected points' (seed indices, rung indices, x0 (npts, D), p (npts, NP), K, n_skip)"""
        if self._pb is None or not getattr(self, "initalized", False):
            raise ValueError("%s() works after anneal() / anneal_init()" % what)
        sb, kb = self._select(beta, seeds)
        N, D, NP, NX = self.N_model, self.D, self.NP, self._NX
        K = D if k is None else int(k)
        n_steps, qr_every, transient = int(n_steps), int(qr_every), int(transient)
        if K < 1 or K > D:
            raise ValueError("%s: k=%d outside 1 .. D=%d" % (what, K, D))
        if n_steps < 1 or qr_every < 1 or n_steps % qr_every:
            raise ValueError("%s: n_steps=%d must be a positive multiple of qr_every=%d" % (what, n_steps, qr_every))
        n_skip = -(-max(transient, 0) // qr_every)                                # whole QR intervals, rounded up
        if n_skip >= n_steps // qr_every:
            raise ValueError("%s: a transient of %d steps leaves none of the %d steps to average over" % (what, transient, n_steps))
        rows = self._mp[sb][:, kb].reshape(len(sb) * len(kb), -1)
        x0 = rows[:, (N - 1) * D:N * D]
        p = rows[:, NX + (N - 1) * NP:NX + N * NP] if self._tdp else rows[:, NX:]
        return sb, kb, x0, p, K, n_skip

    def lyapunov(self, n_steps, k=None, beta=-1, seeds=None, substeps=1, qr_every=4, transient=0, coupling=None, stim=None):
        """Lyapunov exponents of the ESTIMATED model at the estimates (after anneal()): from the LAST row of every selected
        (seed, rung)'s minimising path with that rung's full parameter vector (the last row's with time-dependent
        parameters), t0 = t_model[-1], the k leading exponents (None: all D) over n_steps steps of dt_model by Benettin's
        method on the device (csrc/va_lyap.h): tangents carried by the tangent-linear RK4 map at dt_model / substeps and
        re-orthonormalised every qr_every steps, all selected points in one call.
          beta / seeds  as predict(); the default is the last rung
          transient     model steps left out of the average while the tangents align (rounded up to whole QR intervals)
          coupling      (D,) non-negative gains g: the CONDITIONAL exponents of v' = (J(x) - diag(g)) v (sync_exponents builds
                        them from Lidx)
          stim          (n_steps + 1, n_stim), as predict()
        Returns a dict, leading axes (nbeta_sel,) or (B_sel, nbeta_sel):
          exponents     (..., k)   in decreasing order as the QR orders them, per unit of model time
          logsum        (..., k)   the sums of log R_jj they are formed from
          horizon       (...)      1 / l_1: the time over which a small forecast error grows e-fold; inf where l_1 <= 0
          kaplan_yorke  (...)      the Kaplan-Yorke dimension (only when the whole spectrum was asked for)
          x_end (..., D), Q_end (..., k, D)   state and orthonormal tangents at the end (to continue from)
          status        (...)      0, or j + 1 where the QR met a zero or non-finite R_jj: that point's exponents are NaN
        These are finite-time exponents of the discrete RK4 map of the estimated model from the estimate -- not of the data."""
        sb, kb, x0, p, K, n_skip = self._lyap_points(n_steps, k, beta, seeds, qr_every, transient, "lyapunov")
        g = None
        if coupling is not None:
            g = np.asarray(coupling, dtype=np.float64)
            if g.shape != (self.D,) or not np.all(np.isfinite(g)) or np.any(g < 0):
                raise ValueError("lyapunov: coupling holds D = %d finite non-negative gains" % self.D)
            g = np.ascontiguousarray(np.broadcast_to(g, x0.shape))
        r = self._pb.lyapunov(x0, p, K, int(n_steps), t0=float(self.t_model[-1]), substeps=substeps, qr_every=int(qr_every),
                              n_skip=n_skip, coupling=g, stim=stim)
        lead = (len(sb), len(kb)) if self._batched else (len(kb),)
        lam = np.asarray(r["exponents"]).reshape(lead + (K,))
        l1 = lam[..., 0]
        with np.errstate(divide="ignore", invalid="ignore"):
            horizon = np.where(np.isnan(l1), np.nan, np.where(l1 > 0, 1.0 / l1, np.inf))
        out = dict(exponents=lam, logsum=np.asarray(r["logsum"]).reshape(lead + (K,)), horizon=horizon,
                   x_end=np.asarray(r["x_end"]).reshape(lead + (self.D,)), Q_end=np.asarray(r["Q_end"]).reshape(lead + (K, self.D)),
                   status=np.asarray(r["status"]).reshape(lead))
        if K == self.D:
            out["kaplan_yorke"] = np.asarray(kaplan_yorke(lam)).reshape(lead)
        return out

    def sync_exponents(self, n_steps, gains, k=1, beta=-1, seeds=None, substeps=1, qr_every=4, transient=0, stim=None):
        """Are the measured columns enough?  The k largest CONDITIONAL Lyapunov exponents of the estimated model coupled to
        its own trajectory through the measured columns: gain c on the Lidx columns and 0 elsewhere, for every c in gains,
        (selected points x gains) as one device batch (lyapunov() says how).  The synchronisation manifold y = x of
        y' = f(y) + g o (x - y) is stable where the largest of them is negative.  Returns a dict:
          exponents      (..., len(gains), k)
          critical_gain  (...)  the smallest listed gain whose largest conditional exponent is negative; NaN if none is
          gains          (len(gains),)
          status         (..., len(gains))
        The drive here is the model itself, started at the estimate; measured data drive the real thing."""
        gains = np.atleast_1d(np.asarray(gains, dtype=np.float64))
        if gains.ndim != 1 or gains.size < 1 or not np.all(np.isfinite(gains)) or np.any(gains < 0):
            raise ValueError("sync_exponents: gains is a list of finite non-negative numbers")
        sb, kb, x0, p, K, n_skip = self._lyap_points(n_steps, k, beta, seeds, qr_every, transient, "sync_exponents")
        npts, G, D = x0.shape[0], gains.size, self.D
        one = np.zeros((G, D))
        one[:, np.asarray(self.Lidx, dtype=np.intp)] = gains[:, None]
        r = self._pb.lyapunov(np.repeat(x0, G, axis=0), np.repeat(p, G, axis=0), K, int(n_steps), t0=float(self.t_model[-1]),
                              substeps=substeps, qr_every=int(qr_every), n_skip=n_skip, coupling=np.tile(one, (npts, 1)), stim=stim)
        lead = (len(sb), len(kb)) if self._batched else (len(kb),)
        lam = np.asarray(r["exponents"]).reshape(lead + (G, K))
        neg = lam[..., 0] < 0.0
        order = np.argsort(gains, kind="stable")
        crit = np.full(lead, np.nan)
        for gi in order[::-1]:                                                    # (the smallest such gain is written last)
            crit = np.where(neg[..., gi], gains[gi], crit)
        return dict(exponents=lam, critical_gain=crit, gains=gains, status=np.asarray(r["status"]).reshape(lead + (G,)))

    # ------------------------------------------------------------------ sampling exp(-A) at a rung
    def _hmc_mass(self, mass, k):
        """(minv (B, n_var) or None for identity, reason or None) for rung k"""
        n_var = self._NX + len(self._estpos)
        if isinstance(mass, str):
            if mass == 'identity':
                return None, None
            if mass != 'laplace':
                raise ValueError("mass must be 'laplace', 'identity' or an array of inverse masses")
            try:
                lap = self.laplace(beta=[int(k)])
            except (NotImplementedError, _capi.VaError) as e:
                return None, "identity mass: laplace() refused (%s)" % e
            sv = np.asarray(lap["state_var"]).reshape(self.B, self._NX)
            pc = np.asarray(lap["param_cov"]).reshape(self.B, self.NPest, self.NPest)
            minv = np.concatenate([sv, np.diagonal(pc, axis1=1, axis2=2)], axis=1)
            bad = ~np.all(np.isfinite(minv) & (minv > 0.0), axis=1)
            if bad.all():
                return None, "identity mass: the Hessian is not positive definite at any selected minimiser"
            minv[bad] = 1.0
            return minv, ("identity mass for seed(s) %s: the Hessian is not positive definite there" % [int(b) for b in np.flatnonzero(bad)]
                          if bad.any() else None)
        minv = np.asarray(mass, dtype=np.float64)
        if minv.shape not in [(n_var,), (self.B, n_var)]:
            raise ValueError("mass array must have shape (n_var,) = (%d,) or (B, n_var)" % n_var)
        return minv, None

    def sample(self, n_samples, beta=-1, seeds=None, n_leap=10, step_size=None, jitter=0.1, mass='laplace', warmup=0, thin=1,
               seed=0, keep=None, warmup_block=25):
        """Sample exp(-A(X, p)) at a rung of the ladder (after anneal()): Hamiltonian Monte Carlo on the device
        (csrc/va_hmc.h), one chain per seed, started at the stored minimisers.  With `beta` a sequence, each rung continues
        from the previous rung's final state (precision-annealing Monte Carlo); every rung has warm-up and statistics of
        its own.  n_samples states are kept per chain, one every `thin` iterations of n_leap leapfrog steps.
          step_size  a number or one per seed; None: n_var^-1/4 with mass='laplace', a hundredth of it otherwise -- use warmup
          mass       'laplace': 1 / mass = laplace()'s state_var and parameter variances (identity, with the reason in
                     'mass_note', wherever laplace refuses or is not finite); 'identity'; or an array (n_var,) / (B, n_var)
          warmup     iterations before the statistics, in blocks of warmup_block; after each block every chain's step is
                     rescaled by hmc_rescale_step(its acceptance rate).  They enter no statistic.
          keep       path-vector entries kept per sample; None: the last time row and the estimated parameters
        A is the action AS THE PACKAGE NORMALISES IT (see laplace()).  Returns a dict; leading axes as predict():
          mean, std (..., n_var)   accept_rate, n_divergent, step_size (...)   A, dH (..., n_samples * thin)
          x_last (..., n_samples, D), params (..., n_samples, NPest)  (keep=None)   or   kept (..., n_samples, len(keep))
          x (..., n_var) the final states;  seeds, rungs: the selection;  mass_note: per rung, None or why identity was used.
        With `bounds` on the annealer the chains run through Problem.hmc_box (csrc/va_hmc_box.h): an unconstrained z with
        x = T(z), every state inside its (closed) box and distributed as exp(-A) cut to it, whichever minimiser ran
        (bounded_minimiser='scipy' too).  Everything returned speaks of x.  Far out in z an x rounds ONTO its bound: a
        chain is continued through its z (as the rungs here are), not by passing such an x back as a start.  What differs:
          starts     a minimiser entry on (or outside) a bound is pulled inside by 1e-6 (hi - lo), one-sided bounds by
                     1e-6 max(1, |bound|); 'n_pulled_in' (...) counts the entries, per seed and rung (later rungs continue
                     in z: 0)
          mass       masses are those OF z: 'laplace' divides its variances by (dx/dz)^2 at the rung's start; an array is
                     taken as given, in z
          tails      T is algebraic, exp(-U) has polynomial tails in z: fine for bounds that guard, slow where the
                     posterior piles up on a bound (watch accept_rate and the spread of kept values there)."""
        if self._pb is None or not getattr(self, "initalized", False):
            raise ValueError("sample() works after anneal() / anneal_init()")
        n_samples, n_leap, thin, warmup, warmup_block = int(n_samples), int(n_leap), int(thin), int(warmup), int(warmup_block)
        if n_samples < 1 or warmup < 0 or warmup_block < 1:
            raise ValueError("n_samples and warmup_block must be at least 1, warmup not negative")
        sb, kb = self._select(np.atleast_1d(beta), seeds)
        B, NX, npe = self.B, self._NX, len(self._estpos)
        n_var = NX + npe
        if keep is None:
            last = np.arange((self.N_model - 1) * self.D, self.N_model * self.D)
            keep_idx = np.concatenate([last, NX + (np.arange(npe - self.NPest, npe) if self._tdp else np.arange(npe))])
        else:
            keep_idx = np.asarray(keep, dtype=np.int64).reshape(-1)
        XP = None
        calls = [0]

        def call_seed():
            calls[0] += 1
            return (int(seed) + 0x9E3779B97F4A7C15 * calls[0]) & (2 ** 64 - 1)
        res, notes = [], []
        boxed = self.bounds is not None
        Z, pulled = None, np.zeros(B, np.int64)
        if boxed:
            lo = np.array([-np.inf if b[0] is None else b[0] for b in self.bounds], dtype=np.float64)
            hi = np.array([np.inf if b[1] is None else b[1] for b in self.bounds], dtype=np.float64)
        for k in kb:
            rf = float(self._rf_scale[k])
            if XP is None:
                src = self._mp[:, k]
                XP = np.concatenate([src[:, :NX], src[:, NX:][:, self._estpos]], axis=1)
                if boxed:
                    XP, pulled = hmc_box_pull_in(XP, lo, hi)
            minv, note = self._hmc_mass(mass, k)
            notes.append(note)
            if boxed and isinstance(mass, str) and minv is not None:
                # laplace()'s variances are of x: var_z = var_x / (dx/dz)^2 at the rung's start (rows left at identity stay)
                slope = hmc_box_slope(hmc_box_inverse(XP, lo, hi) if Z is None else Z, lo, hi)
                with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
                    conv = minv / (slope * slope)
                laplace_row = ~np.all(minv == 1.0, axis=1)
                ok = np.all(np.isfinite(conv) & (conv > 0.0), axis=1)
                minv = np.where((laplace_row & ok)[:, None], conv, np.where(laplace_row[:, None], 1.0, minv))
                if np.any(laplace_row & ~ok):
                    why = ("identity mass for seed(s) %s: the Laplace variance over (dx/dz)^2 is not finite at the start"
                           % [int(b) for b in np.flatnonzero(laplace_row & ~ok)])
                    notes[-1] = why if notes[-1] is None else notes[-1] + "; " + why
            if step_size is None:
                eps = np.full(B, float(n_var) ** -0.25 * (1.0 if minv is not None else 0.01))
            else:
                eps = np.array(np.broadcast_to(np.asarray(step_size, dtype=np.float64).reshape(-1), (B,)))
            done = 0
            while done < warmup:
                nb = min(warmup_block, warmup - done)
                if boxed:
                    w = self._pb.hmc_box(XP, rf, nb, n_leap, eps, bounds=self.bounds, z0=Z, jitter=jitter, minv=minv, seed=call_seed())
                    Z = w["z"]
                else:
                    w = self._pb.hmc(XP, rf, nb, n_leap, eps, jitter=jitter, minv=minv, seed=call_seed())
                XP, done = w["x"], done + nb
                eps = hmc_rescale_step(eps, w["accepted"].mean(axis=1))
            if boxed:
                r = self._pb.hmc_box(XP, rf, n_samples * thin, n_leap, eps, bounds=self.bounds, z0=Z, jitter=jitter, minv=minv,
                                     seed=call_seed(), thin=thin, keep_idx=keep_idx)
                Z = r["z"]
                r["n_pulled_in"], pulled = pulled, np.zeros(B, np.int64)
            else:
                r = self._pb.hmc(XP, rf, n_samples * thin, n_leap, eps, jitter=jitter, minv=minv, seed=call_seed(), thin=thin, keep_idx=keep_idx)
            XP = r["x"]
            r["step_size"] = eps
            res.append(r)
        lead = (len(sb), len(kb)) if self._batched else (len(kb),)
        stack = lambda f: np.stack([f(r)[sb] for r in res], axis=1).reshape(lead + np.shape(f(res[0]))[1:])
        out = dict(mean=stack(lambda r: r["mean"]), std=stack(lambda r: np.sqrt(r["var"])), accept_rate=stack(lambda r: r["accepted"].mean(axis=1)),
                   A=stack(lambda r: r["A"]), dH=stack(lambda r: r["dH"]), n_divergent=stack(lambda r: r["n_divergent"]),
                   step_size=stack(lambda r: r["step_size"]), x=stack(lambda r: r["x"]), seeds=sb, rungs=kb, mass_note=notes)
        if boxed:
            out["n_pulled_in"] = stack(lambda r: r["n_pulled_in"])
        kept = stack(lambda r: r["kept"])
        if keep is None:
            out["x_last"], out["params"] = kept[..., :self.D], kept[..., self.D:]
        else:
            out["kept"] = kept
        return out

    def predict_ensemble(self, n_steps, samples, q=(0.025, 0.5, 0.975), **predict_kwargs):
        """The non-linear counterpart of predict_spread(): every kept (x_last, params) of a sample() result (keep=None)
        integrated forward by predict()'s RK4 kernel, all members in ONE device call.  The fixed parameters are the
        sampled rung's.  Returns a dict: members (..., n_samples, n_out, D) and quantiles (len(q), ..., n_out, D) over the
        members; leading axes as sample().  predict_kwargs: substeps, every, stim."""
        if "x_last" not in samples:
            raise ValueError("predict_ensemble needs a sample() result with keep=None (x_last and params)")
        if self._tdp:
            raise NotImplementedError("predict_ensemble: time-dependent parameters are not carried")
        sb, kb = samples["seeds"], samples["rungs"]
        D, NP, NX = self.D, self.NP, self._NX
        x_last = np.asarray(samples["x_last"]).reshape(len(sb), len(kb), -1, D)
        S = x_last.shape[2]
        P = np.repeat(self._mp[sb][:, kb][:, :, None, NX:], S, axis=2)           # (B_sel, nbeta_sel, S, NP)
        if self.NPest:
            P[..., self.Pidx] = np.asarray(samples["params"]).reshape(len(sb), len(kb), S, self.NPest)
        out = self._pb.predict(x_last.reshape(-1, D), P.reshape(-1, NP), n_steps, t0=float(self.t_model[-1]), **predict_kwargs)
        lead = (len(sb), len(kb)) if self._batched else (len(kb),)
        members = out.reshape(lead + (S, out.shape[1], D))
        return dict(members=members, quantiles=np.quantile(members, q, axis=len(lead)))

    # ------------------------------------------------------------------ tracking new data: the ensemble Kalman filter
    def _track_obs_var(self, obs_var):
        L = self.L
        if obs_var is None:
            if np.ndim(self.RM) == 3:
                raise ValueError("track: full RM matrices say nothing about one variance per observed column: pass obs_var")
            if isinstance(self.RM, np.ndarray):
                if np.any(self.RM != self.RM[:1]):
                    raise ValueError("track: RM changes along the data window: pass obs_var for the rows to come")
                return 1.0 / np.array(self.RM[0], dtype=np.float64)
            return np.full(L, 1.0 / float(self.RM))
        ov = np.asarray(obs_var, dtype=np.float64)
        if ov.shape not in ((), (L,)) or not np.all(np.isfinite(ov)) or np.any(ov <= 0):
            raise ValueError("track: obs_var is a positive finite number, or L = %d of them" % L)
        return np.ascontiguousarray(np.broadcast_to(ov, (L,)))

    def track(self, Y_future, obs_every=1, members=32, samples=None, obs_var=None, inflation=1.0, substeps=1, beta=-1, seeds=None,
              stim=None, estimate_params=True, seed=0, gauss_newton=False):
        """Carry the estimate and its uncertainty through observations that arrive AFTER the fitted window (after anneal()):
        an ensemble Kalman filter on the device (csrc/va_enkf.h), all selected (seed, rung)s in ONE call.  Per observation
        row every member moves obs_every steps of dt_model by predict()'s RK4 (dt_model / substeps), then the row's
        observations are assimilated one after the other by the serial ensemble square-root filter (Whitaker & Hamill 2002).
          Y_future   (n_obs, L), the Lidx columns; row k is at t_model[-1] + (k + 1) obs_every dt_model -- row 0 is NOT the last
                     fitted time, unlike prediction_error's.  NaN: a missing observation.  Every selected point gets the same data.
          members    M: the initial ensemble is drawn from the Laplace posterior -- one laplace(full=True) call gives the joint
                     covariance of the last state and the estimated parameters, as predict_spread() assembles it; member m =
                     estimate + (its Cholesky factor) . normals, the normals from the counter-based generator of sample()
                     (_capi.hmc_noise(seed, chain = point index, iteration 0)).  A point whose covariance has no factor keeps
                     predict_spread()'s status (-2, or laplace()'s own) and NaN outputs; nothing raises.
          samples    a sample() result (keep=None) instead: its kept x_last / params are the members (predict_ensemble()'s
                     bookkeeping); beta / seeds / members / seed are then not used
          obs_var    (L,) or a number: the observation error variance; None: 1 / RM per observed column for a scalar or
                     per-column RM (RM = 1 / sigma^2, the convention of the reference's examples).  RM arrays that change
                     along the window and full RM matrices need an explicit obs_var (ValueError)
          inflation  >= 1: every member's distance from the forecast mean is multiplied by it before each analysis
          estimate_params  False: states only; the parameters stay as the members have them
          stim       (n_obs obs_every + 1, n_stim), from t_model[-1] on, as predict()
        Returns a dict, leading axes as predict():
          mean, std (..., n_obs, D)                     the analysis mean and standard deviation after every row
          mean_forecast, std_forecast (..., n_obs, D)   the same before the row was assimilated
          params, params_std (..., n_obs, NPest)        the analysis statistics of the estimated parameters
          innovation (..., n_obs, L)                    Y_future - mean_forecast[..., Lidx]
          x_end (..., M, D), p_end (..., M, NP)         the members after the last row (to continue from)
          status (...)   0; k + 1: row k's forecast was not finite (NaN from there on).  A point without an initial ensemble
                         has predict_spread()'s status (-2, or laplace()'s own, which is positive inside the path) and NaN in
                         every row, row 0 included
          seeds, rungs   the selection
        Bounds are NOT enforced on filtered states or parameters.  Not built: localisation, a full R, adaptive inflation.
        Time-dependent parameters: NotImplementedError."""
        if self._pb is None or not getattr(self, "initalized", False):
            raise ValueError("track() works after anneal() / anneal_init()")
        if self._tdp:
            raise NotImplementedError("track: time-dependent parameters are not carried")
        Yf = np.asarray(Y_future, dtype=np.float64)
        if Yf.ndim != 2 or Yf.shape[0] < 1 or Yf.shape[1] != self.L:
            raise ValueError("Y_future must have shape (n_obs >= 1, L = %d), got %s" % (self.L, Yf.shape))
        ov = self._track_obs_var(obs_var)
        if not float(inflation) >= 1.0:
            raise ValueError("track: inflation is at least 1")
        D, NP, NPe, NX, N = self.D, self.NP, self.NPest, self._NX, self.N_model
        est = list(self.Pidx) if estimate_params else []
        if samples is not None:
            if "x_last" not in samples:
                raise ValueError("track needs a sample() result with keep=None (x_last and params)")
            sb, kb = samples["seeds"], samples["rungs"]
            npts = len(sb) * len(kb)
            x0 = np.asarray(samples["x_last"], dtype=np.float64).reshape(npts, -1, D)
            M = x0.shape[1]
            p = np.repeat(self._mp[sb][:, kb][:, :, None, NX:], M, axis=2).reshape(npts, M, NP)
            if NPe:
                p[..., self.Pidx] = np.asarray(samples["params"]).reshape(npts, M, NPe)
            status0 = np.zeros(npts, dtype=np.int32)
        else:
            M = int(members)
            if M < 2:
                raise ValueError("track: an ensemble has at least 2 members")
            sb, kb, status0, F = self._laplace_factor(beta, seeds, gauss_newton)
            npts, nw = len(sb) * len(kb), D + NPe
            rows = self._mp[sb][:, kb].reshape(npts, -1)
            x0 = np.repeat(rows[:, None, (N - 1) * D:N * D], M, axis=1)
            p = np.repeat(rows[:, None, NX:], M, axis=1)
            for j in range(npts):
                if status0[j] != 0:
                    continue
                z = _capi.hmc_noise(seed, j, 0, M * nw)[1].reshape(M, nw)
                dz = np.dot(z, F[j].T)
                x0[j] += dz[:, :D]
                if NPe:
                    p[j][:, self.Pidx] += dz[:, D:]
        r = self._pb.enkf(np.ascontiguousarray(x0), np.ascontiguousarray(p), Yf, ov, obs_every=int(obs_every), est=est,
                          inflation=float(inflation), t0=float(self.t_model[-1]), substeps=substeps, stim=stim)
        lead = (len(sb), len(kb)) if self._batched else (len(kb),)
        status = np.where(status0 != 0, status0, np.asarray(r["status"], dtype=np.int32))
        bad = status0 != 0
        n_obs, nq = Yf.shape[0], len(est)
        stat = {k: np.array(r[k]) for k in ("mean_f", "sd_f", "mean_a", "sd_a")}
        for v in stat.values():
            v[bad] = np.nan
        x_end, p_end = np.array(r["x_end"]), np.array(r["p_end"])
        x_end[bad] = np.nan
        p_end[bad] = np.nan
        par = lambda a: a[..., D:] if nq else np.empty((npts, n_obs, 0))
        out = dict(mean=stat["mean_a"][..., :D], std=stat["sd_a"][..., :D], mean_forecast=stat["mean_f"][..., :D],
                   std_forecast=stat["sd_f"][..., :D], params=par(stat["mean_a"]), params_std=par(stat["sd_a"]),
                   innovation=Yf - stat["mean_f"][..., self.Lidx], x_end=x_end, p_end=p_end, status=status)
        out = {k: np.ascontiguousarray(v).reshape(lead + v.shape[1:]) for k, v in out.items()}
        out["seeds"], out["rungs"] = sb, kb
        return out

    def me_gaussian(self, X):
        """Measurement error of a path (va_ode.py:138-158); X may omit the parameters."""
        X = np.asarray(X, dtype=np.float64)
        if X.shape[-1] == self._NX:
            pad = self._Pfull[:, self._estpos] if X.ndim == 2 else self._Pfull[0, self._estpos]
            X = np.concatenate([X, pad], axis=-1)
        return self._eval(X, False)[1]

    # ------------------------------------------------------------------ savers (va_ode.py:794-889)
    def save_paths(self, filename, dtype=np.float64, fmt="%.8e"):
        ND = self.N_model * self.D
        sav = np.reshape(self._mp[:, :, :ND], (self.B, self.Nbeta, self.N_model, self.D))
        ts = np.resize(np.reshape(self.t_model, (self.N_model, 1)), (self.B, self.Nbeta, self.N_model, 1))
        self._save_array(filename, self._view(np.concatenate((ts, sav), axis=3)), dtype, fmt, self.D + 1)

    def save_params(self, filename, dtype=np.float64, fmt="%.8e"):
        if self.NPest == 0:
            print("WARNING: You did not estimate any parameters.  Writing fixed "
                  "parameter values to file anyway.")
        ND = self.N_model * self.D
        sav = self._mp[:, :, ND:]
        if self._tdp:                                 # (Nbeta, N_model, NP), va_ode.py:824-840
            sav = sav.reshape(self.B, self.Nbeta, self.N_model, self.NP)
        self._save_array(filename, self._view(sav), dtype, fmt, self.NP)

    def save_as_minAone(self, savedir='', savefile=None, seed=0):
        """minAone-style text rows [beta, exitflag, A, path..., params...] (va_ode.py:875-889).
        Upstream saves never-written exitflags; here they hold the minimiser's status."""
        if savedir.endswith('/') is False:
            savedir += '/'
        if savefile is None:
            savefile = savedir + 'D%d_M%d_PATH%d.dat' % (self.D, self.L, self.adolcID)
        else:
            savefile = savedir + savefile
        betaR = self.beta_array.reshape((self.Nbeta, 1))
        exitR = self._flags[seed].reshape((self.Nbeta, 1))
        AR = self._A[seed].reshape((self.Nbeta, 1))
        np.savetxt(savefile, np.hstack((betaR, exitR, AR, self._mp[seed])))
