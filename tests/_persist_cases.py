"""The cases of tests/test_persist_cases.py (CPU: the planner accepts each slicing, the oracle alone is stable on it,
the case reaches the branch it is there for) and tests/test_gpu_persist_geometry.py (GPU: the persistent ladder kernel
k_seed, csrc/va_persist.h, and the three-launch cycle against the oracle, step for step).

A case names its problem (D, N, B, disc, lbfgs_m, nskip, Lidx, Pidx, weights, model), its slicing (persist_rows: rows
per workgroup asked of `tune`, 0 = the planner's own choice; G, T: the geometry the planner must then report) and its
minimisation (rf, maxiter).  `problem(case)` builds the arrays, `oracle(case)` runs the reference minimiser once per
seed and keeps the result for every test that asks.

Slicings the planner refuses by construction (csrc/va_persist_geo.h: every slice holds two rows at least,
Simpson-Hermite slices are even and N is odd there, so T = 2 always leaves a last slice of one row) are replaced by
the nearest admissible ones with the same property:
  Simpson-Hermite T = 2             ->  T = 4 (N = 43: G = 11; N = 67: G = 17, past 16)
  Simpson-Hermite N = 37, T = 4     ->  N = 39 (G = 10, past one chunk of 8)
  Simpson-Hermite full last slice   ->  N = 47, T = 8: a last slice of T - 1 rows, the fullest an odd N allows
  full matrices N = 21, T = 4       ->  T = 6 (21 = 5 * 4 + 1 leaves one row; T = 6: G = 4, last slice 3 rows)
  nskip = 5, T = 4                  ->  N = 46 (N_data = 10); N = 41 leaves one row
  Simpson-Hermite rf_vec T = 6      ->  nskip = 5, N = 41 (nskip = 3 gives N = 6k + 1: one row left)
"""
import collections
import functools

import numpy as np

Case = collections.namedtuple("Case", "name group D N B disc lbfgs_m persist_rows nskip Lidx Pidx weights model rf maxiter G T reach")

OPTS = {'gtol': 1e-8, 'ftol': 1e-8, 'maxfun': 1000000}
PZ_MREG = 10            # csrc/va_persist_geo.h
PZ_WAVES = 16
DISCS = ("trapezoid", "SimpsonHermite", "euler", "forwardmap")
SHORT = {"trapezoid": "trap", "SimpsonHermite": "sh", "euler": "euler", "forwardmap": "fmap"}

# branches of csrc/va_persist.h a case can be there for (checked on the CPU by tests/test_persist_cases.py)
COL_GT_MREG = "col > PZ_MREG"       # pz_coeffs' LDS path
HALO_HL2 = "G > 1, HL = 2"          # the left halo poll of two rows (Simpson-Hermite)
NDN0 = "ndn = 0"                    # a slice without a data row
RF0_FULL = "rf0_full"               # tile_qfull and the qs / fs swap
NPE0 = "NPe = 0"                    # no parameter block
IDLE_WAVES = "wave*64 >= RD"        # waves without an element of the staged rows
BRANCHES = (COL_GT_MREG, HALO_HL2, NDN0, RF0_FULL, NPE0, IDLE_WAVES)

CASES = []


def _add(name, group, D, N, disc, G, T, persist_rows=0, B=1, lbfgs_m=10, nskip=1, Lidx=None, Pidx=(0,), weights="scalar",
         model="l96", rf=1.5 ** 8, maxiter=25, reach=()):
    reach = set(reach)
    HL = 2 if disc == "SimpsonHermite" else 1
    if G > 1 and HL == 2:
        reach.add(HALO_HL2)
    if PZ_WAVES * 64 - 64 >= (T + HL + 1) * D:
        reach.add(IDLE_WAVES)
    if len(Pidx) == 0:
        reach.add(NPE0)
    if weights == "full":
        reach.add(RF0_FULL)
    if lbfgs_m > PZ_MREG:
        reach.add(COL_GT_MREG)
    if any(data_rows(N, T, nskip, w) == 0 for w in range(G)):
        reach.add(NDN0)
    CASES.append(Case(name, group, D, N, B, disc, lbfgs_m, persist_rows, nskip, None if Lidx is None else tuple(Lidx),
                      tuple(Pidx), weights, model, rf, maxiter, G, T, tuple(sorted(reach))))


def data_rows(N, T, nskip, w):
    """data rows that fall on the model rows of slice w (k_seed's ndn)"""
    n0 = w * T
    rows = min(T, N - n0)
    nd_lo = (n0 + nskip - 1) // nskip
    nd_hi = min((n0 + rows - 1) // nskip, (N - 1) // nskip)
    return max(0, nd_hi - nd_lo + 1)


# ---- width x discretisation, the planner's own slicing: one workgroup while the LDS holds the path (Simpson-Hermite: N is
# odd and slices are even, so two); at D = 36 and 64 the planner itself cuts the path
WIDTH_GEO = {4: ((1, 40), (2, 38)), 5: ((1, 40), (2, 38)), 7: ((1, 40), (2, 38)), 36: ((3, 16), (3, 14)), 64: ((5, 8), (7, 6))}
for _D in (4, 5, 7, 36, 64):
    for _disc in DISCS:
        _sh = _disc == "SimpsonHermite"
        _G, _T = WIDTH_GEO[_D][_sh]
        _add("width_D%d_%s" % (_D, SHORT[_disc]), "width", _D, 41 if _sh else 40, _disc, _G, _T)

# ---- forced slices, at D = 20 (one seed) and D = 5 (two seeds)
for _D, _B in ((20, 1), (5, 2)):
    for _disc in DISCS:
        _sh = _disc == "SimpsonHermite"
        _n = "D%d_%s" % (_D, SHORT[_disc])
        if _sh:
            _add("forced_T4_G17_" + _n, "forced", _D, 67, _disc, 17, 4, 4, B=_B)
            _add("forced_T4_G10_" + _n, "forced", _D, 39, _disc, 10, 4, 4, B=_B)
            _add("forced_last3_" + _n, "forced", _D, 43, _disc, 6, 8, 8, B=_B)
            _add("forced_last7of8_" + _n, "forced", _D, 47, _disc, 6, 8, 8, B=_B)
            _add("forced_G2_" + _n, "forced", _D, 41, _disc, 2, 22, 22, B=_B)
        else:
            _add("forced_T2_G20_" + _n, "forced", _D, 40, _disc, 20, 2, 2, B=_B)
            _add("forced_T4_G9_" + _n, "forced", _D, 36, _disc, 9, 4, 4, B=_B)
            _add("forced_last2_" + _n, "forced", _D, 42, _disc, 6, 8, 8, B=_B)
            _add("forced_lastfull_" + _n, "forced", _D, 40, _disc, 5, 8, 8, B=_B)
            _add("forced_G2_" + _n, "forced", _D, 40, _disc, 2, 20, 20, B=_B)

# ---- history length: a stiff rung, so that the history fills and wraps (m <= 17) or passes 20 columns (m = 32).
# (G, T) of the automatic slicing: what the planner gives at these sizes, by the LDS the 2m history vectors take
HIST = {  # m: (rf, maxiter)
    3: (1.5 ** 12, 30), 10: (1.5 ** 12, 30), 11: (1.5 ** 12, 30), 17: (1.5 ** 12, 35), 32: (1.5 ** 12, 45)}
HIST_GEO_TRAP = {3: (1, 60), 10: (2, 31), 11: (3, 29), 17: (4, 19), 32: (7, 9)}
HIST_GEO_SH = {3: (2, 58), 10: (2, 58), 11: (2, 58), 17: (2, 58), 32: (2, 44)}
for _m, (_rf, _mi) in HIST.items():
    _add("hist_m%d_D20_trap" % _m, "history", 20, 60, "trapezoid", HIST_GEO_TRAP[_m][0], HIST_GEO_TRAP[_m][1], lbfgs_m=_m, rf=_rf, maxiter=_mi)
    _add("hist_m%d_D5_sh" % _m, "history", 5, 61, "SimpsonHermite", HIST_GEO_SH[_m][0], HIST_GEO_SH[_m][1], lbfgs_m=_m, rf=_rf, maxiter=_mi)
_add("hist_m11_D20_trap_T6", "history", 20, 60, "trapezoid", 10, 6, 6, lbfgs_m=11, rf=HIST[11][0], maxiter=HIST[11][1])
_add("hist_m11_D5_sh_T8", "history", 5, 61, "SimpsonHermite", 8, 8, 8, lbfgs_m=11, rf=HIST[11][0], maxiter=HIST[11][1])

# ---- sparse data and weight arrays at slice edges: N = (N_data - 1) * nskip + 1
for _w in ("scalar", "rm_vec", "rf_vec"):
    _add("sparse_nskip3_T2_" + _w, "sparse", 20, 40, "trapezoid", 20, 2, 2, nskip=3, weights=_w)        # slices without a data row
    _add("sparse_nskip5_T4_" + _w, "sparse", 20, 46, "trapezoid", 12, 4, 4, nskip=5, weights=_w)        # the same
    _add("sparse_nskip3_T8_" + _w, "sparse", 20, 40, "trapezoid", 5, 8, 8, nskip=3, weights=_w)         # edges 8, 16, .. off the data grid
_add("sparse_sh_nskip3_T4_rf_vec", "sparse", 20, 43, "SimpsonHermite", 11, 4, 4, nskip=3, weights="rf_vec")
_add("sparse_sh_nskip5_T6_rf_vec", "sparse", 20, 41, "SimpsonHermite", 7, 6, 6, nskip=5, weights="rf_vec")
_add("sparse_euler_nskip3_T8_rm_vec", "sparse", 20, 40, "euler", 5, 8, 8, nskip=3, weights="rm_vec")
_add("sparse_euler_nskip3_T2_rm_vec", "sparse", 20, 40, "euler", 20, 2, 2, nskip=3, weights="rm_vec")

# ---- observed columns / parameters, forced T = 8
_add("obs_unsorted", "obs", 20, 40, "trapezoid", 5, 8, 8, Lidx=[19, 0, 3])
_add("obs_unsorted_sh", "obs", 20, 43, "SimpsonHermite", 6, 8, 8, Lidx=[19, 0, 3])
_add("obs_L1", "obs", 20, 40, "trapezoid", 5, 8, 8, Lidx=[7])
_add("obs_LD", "obs", 20, 40, "trapezoid", 5, 8, 8, Lidx=range(20), rf=1.5 ** 12)      # (everything observed: a stiffer rung, or the first step converges)
_add("obs_NPest0", "obs", 20, 40, "trapezoid", 5, 8, 8, Pidx=())
_add("obs_NPest0_sh", "obs", 20, 43, "SimpsonHermite", 6, 8, 8, Pidx=())
_add("obs_B3", "obs", 20, 40, "trapezoid", 5, 8, 8, B=3)

# ---- full matrices: RM (N_data, L, L) and RF0 (N - 1, D, D); the oracle is lbfgs_generic on complex-step gradients
for _disc in ("trapezoid", "SimpsonHermite"):
    _sh = _disc == "SimpsonHermite"
    _add("full_%s_auto" % SHORT[_disc], "full", 5, 21, _disc, 2 if _sh else 1, 18 if _sh else 21, weights="full", rf=4e-6 * 1.5 ** 8, maxiter=15)
    _add("full_%s_T6" % SHORT[_disc], "full", 5, 21, _disc, 4, 6, 6, weights="full", rf=4e-6 * 1.5 ** 8, maxiter=15)

# ---- generated model, three parameters, the middle one fixed
_add("generated_damped3_T8", "generated", 6, 40, "trapezoid", 5, 8, 8, Pidx=(0, 2), model="damped3", rf=1.5 ** 6, maxiter=25)

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
GROUPS = ("width", "forced", "history", "sparse", "obs", "full", "generated")


def damped3(t, x, p):
    """the damped Lorenz-96 of tests/test_gpu_persist.py with a third parameter (a quadratic drag)"""
    return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - p[1] * x + p[0] - p[2] * x * x


def n_params(case):
    return 3 if case.model == "damped3" else 1


def opts(case):
    return dict(OPTS, maxiter=case.maxiter, maxcor=case.lbfgs_m)


def problem(case):
    """the arrays of a case: Y (N_data, L), Lidx, XP (B, N*D + NPest), P (B, NP), dt, RM, RF0 (as both the C-ABI and
    the oracle take them).  Cached and shared by the cases that differ in their slicing only: nobody writes to them."""
    return _problem(_unsliced(case))


def _unsliced(case):
    return case._replace(name="", group="", persist_rows=0, G=0, T=0, reach=())


@functools.lru_cache(maxsize=None)
def _problem(case):
    from varanneal_amd import twin
    D, N, B, nskip = case.D, case.N, case.B, case.nskip
    t, Y, _, Lidx = twin.make_twin(D, N, Lidx=None if case.Lidx is None else list(case.Lidx))
    Y = np.ascontiguousarray(Y[::nskip])
    NP, Pidx = n_params(case), list(case.Pidx)
    XP = np.empty((B, N * D + len(Pidx))); P = np.empty((B, NP))
    for b in range(B):
        if case.model == "damped3":
            rng = np.random.RandomState(5 + b)
            X0 = 20.0 * rng.rand(N, D) - 10.0
            X0[::nskip, Lidx] = Y
            P[b] = [7.0 + 0.5 * b, 1.0, 0.01]
        else:
            X0, P0 = twin.initial_guess(N, D, b, Y, Lidx, nskip)
            P[b] = P0
        XP[b, :N * D] = X0.ravel(); XP[b, N * D:] = P[b, Pidx]
    RM, RF0 = 4.0, 4e-6
    rng = np.random.RandomState(77)
    L = len(Lidx)
    if case.weights == "rm_vec":            # (row- and column-dependent: a wrong data-row offset shows)
        RM = 4.0 * (0.5 + rng.rand(Y.shape[0], L))
    elif case.weights == "rf_vec":
        RF0 = 4e-6 * (0.5 + rng.rand(N - 1, D))
    elif case.weights == "full":            # (as tests/test_gpu_fuzz.py builds them; neither kernel nor oracle assumes symmetry)
        RM = np.array([2.0 * np.eye(L) + 0.5 * rng.randn(L, L) for _ in range(Y.shape[0])])
        RF0 = np.array([2.0 * np.eye(D) + 0.5 * rng.randn(D, D) for _ in range(N - 1)])
    for a in (Y, XP, P, RM, RF0):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return dict(Y=Y, Lidx=Lidx, XP=XP, P=P, dt=twin.DT, RM=RM, RF0=RF0, Pidx=Pidx)


def generic(case):
    return case.weights == "full" or case.model != "l96"


def oracle_minimize(case, b, x0):
    """the reference minimiser on seed b of the case from x0: (x, A, status, nit, nfev)"""
    import va_oracle
    from varanneal_amd import twin
    p = problem(case)
    if not generic(case):
        opb = va_oracle.Problem(case.D, case.N, p["Y"], p["Lidx"], p["dt"], p["RM"], p["RF0"], p["P"][b], p["Pidx"], disc=case.disc,
                                merr_nskip=case.nskip)
        return opb.minimize_lbfgs(x0, case.rf, opts(case))
    f = damped3 if case.model == "damped3" else twin.l96
    RFs = p["RF0"] * case.rf
    fun = lambda z: va_oracle.numpy_action_generic(f, z, case.D, case.N, p["Y"], p["Lidx"], p["dt"], p["RM"], RFs, n_params(case),
                                                   p["Pidx"], p["P"][b], case.disc, nskip=case.nskip)
    return va_oracle.lbfgs_generic(lambda x: (fun(x)[0], va_oracle.complex_step_grad(fun, x)), x0, opts(case))


def oracle(case):
    """the oracle's minimisation of every seed of the case, computed once (and once for the cases that differ in their
    slicing only): a list of (x, A, status, nit, nfev)"""
    return _oracle(_unsliced(case))


@functools.lru_cache(maxsize=None)
def _oracle(case):
    p = problem(case)
    out = []
    for b in range(case.B):
        r = oracle_minimize(case, b, p["XP"][b])
        r[0].setflags(write=False)
        out.append(r)
    return out
