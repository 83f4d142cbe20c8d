"""The zoo's cases and references (TEST INFRASTRUCTURE): for every model of tests/models/zoo.py the inputs of the trajectory
tests (T = 7 starts, parameters of their own, a stimulus where the model has one, t0 = 3), the NumPy references of predict /
predict_tangent / lyapunov from the complex-safe binding (_predict_ref.rk4, _tlm_ref.tlm_rk4, _lyap_ref.lyap_ref), the record
of the switching arguments along those runs, references with a wrong stage time or t0 = 0 (what the inputs must be able to
show), the Hessian-vector cases with their torch reference, and the tolerances with their derivation.  Shared by
tests/test_zoo_cpu.py, tests/test_hvp_cpu.py (host) and tests/test_gpu_generated_tangents.py (device); nothing here is
measured against the device, and nothing here is modified by a test."""
import functools

import numpy as np

import _hess_ref as hr
from _lyap_ref import gain_every_second, lyap_ref
from _predict_ref import DT, K_TRUE, STEPS, attractor_starts, rk4
from _tlm_ref import row_error, tlm_rk4
from models import zoo

T = 7
T0 = 3.0
T_HVP = 1.7                           # t_model of the Hessian-vector cases starts here
PAIRS_TLM = ((1, 1), (2, 3))          # (substeps, every) of tests/test_gpu_predict.py and tests/test_gpu_predict_tlm.py
PAIRS_LYAP = ((1, 1), (2, 4))         # (substeps, qr_every) of tests/test_gpu_lyap.py
MARGIN = 1e-6                         # every switching argument of every stage evaluation stays this far from its threshold
MARGIN_POINT = 1e-3                   # ... of the single points the emitted functions are evaluated at
NAMES = ("kinked_small", "kinked_stencil", "timed_mix9", "timed_mix0", "l96_damped20", "l96_damped67", "l96_colparams")
SEEDS = dict(kinked_small=0, kinked_stencil=7, timed_mix9=2, timed_mix0=3, l96_damped20=4, l96_damped67=5, l96_colparams=11)


def model(name):
    return zoo.all_models()[name]


@functools.lru_cache(maxsize=None)
def traj_case(name):
    """dict(x0 (T, D), P (T, NP), Pidx, stim (steps + 1, 1) or None, V (nvec, D + NPe), Ks, steps)"""
    m = model(name)
    D, NP = m.D, m.NP
    rng = np.random.RandomState(500 + SEEDS[name])
    j = np.arange(T)
    if name.startswith("l96_damped"):
        x0, P, Pidx = attractor_starts(D, T).copy(), np.stack([K_TRUE * (1.0 + 0.02 * j), 1.0 + 0.01 * j], axis=1), [0, 1]
    elif m.colparams:
        x0, P, Pidx = attractor_starts(D, T).copy(), K_TRUE + 0.5 * rng.randn(T, D), list(range(D))
    elif m.kinked:
        x0, P, Pidx = 0.8 * rng.randn(T, D), np.array([1.0, 0.5]) * (1.0 + 0.05 * rng.randn(T, 2)), [1, 0]
    else:
        x0, P, Pidx = 0.6 * rng.randn(T, D), 0.5 + rng.rand(T, NP), ([NP - 1, 0] if NP > 1 else [0])
    tt = DT * np.arange(STEPS + 1)
    stim = (np.sin(4.0 * tt) ** 2 + 0.5 * tt)[:, None] if m.nstim else None
    nw = D + len(Pidx)
    if D <= 20:
        V = np.eye(nw)
    else:                                 # D = 67: a few directions -- the ends of the ring, both parameters, a mixed one
        V = np.zeros((5, nw))
        V[0, 0] = V[1, D - 1] = V[2, D] = V[3, D + 1] = 1.0
        V[4] = rng.randn(nw)
    Ks = [D] if D <= 12 else ([3, 20] if D == 20 else [])
    c = dict(name=name, D=D, NP=NP, x0=x0, P=P, Pidx=Pidx, stim=stim, V=V, Ks=Ks, steps=STEPS, dt=DT, t0=T0)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def safe_points(name, n, seed, t=2.3):
    """n single points (t, x (n, D), p (NP,), st (n,) or None) whose switching arguments are all at least MARGIN_POINT from
    their thresholds (a row that is not is drawn again), and the (n, n_switch) arguments themselves (None: no kinks)"""
    m = model(name)
    rng = np.random.RandomState(seed)
    p = 0.6 + 0.8 * rng.rand(m.NP)
    st = rng.randn(n) if m.nstim else None
    x = np.empty((n, m.D))
    for r in range(n):
        while True:
            x[r] = 0.9 * rng.randn(m.D)
            if not m.kinked or np.abs(m.switch_row(t, x[r], p)).min() >= MARGIN_POINT:
                break
    sw = m.switch_slices(np.full(n, t), x, p, st) if m.kinked else None
    return t, x, p, st, sw


# ---------------------------------------------------------------------------------------------------------------
class Kinks(object):
    """the record of a model's switching arguments over every stage evaluation of a reference run: the smallest distance
    from a threshold, and per trajectory the sign patterns met (more than one: a switching surface was crossed)"""

    def __init__(self, m, ntraj):
        self.m, self.margin, self.patterns = m, np.inf, [set() for _ in range(ntraj)]

    def f(self, j):
        def f(t, x, p, st=None):
            s = self.m.switch_row(t, x, p, st)
            self.margin = min(self.margin, float(np.abs(s).min()))
            self.patterns[j].add(tuple(s > 0))
            return self.m.row(t, x, p, st)
        return f

    def crossed(self):
        return [len(s) > 1 for s in self.patterns]


def _mistimed(fn, h):
    """fn called stage after stage, with the two midpoint stages moved back to the start of the step: stage times
    t + 0, 0, 0, h -- what a kernel that drops the h / 2 would compute"""
    n = [0]

    def g(t, *a):
        c = n[0] % 4
        n[0] += 1
        return fn(t - (0.5 * h if c in (1, 2) else 0.0), *a)
    return g


def _fns(m, Pidx, substeps, wrong, dt):
    if wrong == "midpoint":
        return (lambda: _mistimed(m.row, dt / substeps)), (lambda: _mistimed(m.jvp(Pidx), dt / substeps))
    return (lambda: m.row), (lambda: m.jvp(Pidx))


@functools.lru_cache(maxsize=None)
def predict_reference(name, substeps, every, wrong=None):
    """(ref (T, n_out, D) from _predict_ref.rk4, Kinks or None).  wrong: None, 'midpoint' (stage times t + 0, 0, 0, h) or 't0'
    (the run started at time 0)"""
    m, c = model(name), traj_case(name)
    kinks = Kinks(m, T) if (m.kinked and wrong is None) else None
    f, _ = _fns(m, c["Pidx"], substeps, wrong, c["dt"])
    t0 = 0.0 if wrong == "t0" else c["t0"]
    ref = np.array([rk4(kinks.f(j) if kinks else f(), c["x0"][j], c["P"][j], c["steps"], c["dt"], t0=t0, substeps=substeps, every=every,
                        stim=c["stim"]) for j in range(T)])
    ref.setflags(write=False)
    return ref, kinks


@functools.lru_cache(maxsize=None)
def tangent_reference(name, substeps, every, wrong=None, dtype=np.float64):
    """(out (T, n_out, D), dX (T, nvec, n_out, D)) from _tlm_ref.tlm_rk4 driven by the complex-safe jvp"""
    m, c = model(name), traj_case(name)
    f, jvp = _fns(m, c["Pidx"], substeps, wrong, c["dt"])
    t0 = 0.0 if wrong == "t0" else c["t0"]
    res = [tlm_rk4(f(), jvp(), c["x0"][j], c["P"][j], c["V"], c["steps"], c["dt"], t0=t0, substeps=substeps, every=every, stim=c["stim"],
                   dtype=dtype) for j in range(T)]
    out, dX = np.array([r[0] for r in res]), np.array([r[1] for r in res])
    out.setflags(write=False)
    dX.setflags(write=False)
    return out, dX


@functools.lru_cache(maxsize=None)
def lyap_reference(name, K, substeps, qr_every, gain=False, wrong=None, dtype=np.float64):
    """dict of stacked _lyap_ref.lyap_ref outputs; the tangents move by the complex-safe jvp (its parameter part empty)"""
    m, c = model(name), traj_case(name)
    f, jvp = _fns(m, [], substeps, wrong, c["dt"])
    t0 = 0.0 if wrong == "t0" else c["t0"]
    g = gain_every_second(c["D"]) if gain else None
    res = [lyap_ref(f(), jvp(), c["x0"][j], c["P"][j], K, c["steps"], c["dt"], t0=t0, substeps=substeps, qr_every=qr_every, gain=g,
                    stim=c["stim"], dtype=dtype) for j in range(T)]
    out = {k: np.array([r[k] for r in res]) for k in res[0]}
    for a in out.values():
        a.setflags(write=False)
    return out


def lyap_cases(name):
    """(K, substeps, qr_every, gain) the tests run: every K at both pairs, and the largest K once with the gain"""
    Ks = traj_case(name)["Ks"]
    return [(K, s, q, False) for K in Ks for s, q in PAIRS_LYAP] + [(K, 2, 4, True) for K in Ks[-1:]]


def lyap_error(a, b):
    return max(float(np.abs(np.asarray(a[k], dtype=np.longdouble) - b[k]).max()) for k in ("logsum", "Q_end", "trace"))


# ---------------------------------------------------------------------------------------------------------------
# |device or host C++ - NumPy| <= TOL[name][quantity]:  x absolute on the states, tlm relative per row (_tlm_ref.row_error),
# lyap absolute on logsum, trace and Q_end.  250 x the figures of derive_zoo_tol (its docstring), rounded up to two digits.
TOL = {
    "kinked_small": dict(x=3.5e-13, tlm=9.5e-13, lyap=5.0e-13),
    "kinked_stencil": dict(x=2.3e-13, tlm=3.4e-13, lyap=6.7e-13),
    "timed_mix9": dict(x=2.1e-13, tlm=5.6e-13, lyap=3.8e-13),
    "timed_mix0": dict(x=8.3e-13, tlm=3.5e-13, lyap=4.1e-13),
    "l96_damped20": dict(x=3.9e-12, tlm=1.1e-12, lyap=2.8e-12),
    "l96_damped67": dict(x=6.3e-12, tlm=2.6e-12, lyap=None),
    "l96_colparams": dict(x=3.5e-12, tlm=1.2e-12, lyap=1.2e-12),
}


def derive_zoo_tol(name, verbose=True):
    """TOL[name] as _predict_ref.TOL, _tlm_ref.TOL and _lyap_ref.TOL are derived, for this model and the inputs of
    traj_case(name): the references in float64 against the same references carried in np.longdouble (the complex-safe
    binding both times; never the device), the largest difference over the cases the tests run -- both (substeps, every)
    pairs; for lyap every (K, substeps, qr_every, gain) of lyap_cases -- times the project's 250-fold margin for FMA
    contraction and summation order.  Measured (float64 against longdouble), and 250 x that:

        model            x (absolute)          tlm (relative per row)  lyap (absolute)
        kinked_small     1.38e-15 -> 3.5e-13   3.79e-15 -> 9.5e-13     2.00e-15 -> 5.0e-13     states up to 2.2
        kinked_stencil   8.91e-16 -> 2.3e-13   1.36e-15 -> 3.4e-13     2.67e-15 -> 6.7e-13     states up to 1.9
        timed_mix9       8.23e-16 -> 2.1e-13   2.22e-15 -> 5.6e-13     1.51e-15 -> 3.8e-13
        timed_mix0       3.30e-15 -> 8.3e-13   1.37e-15 -> 3.5e-13     1.61e-15 -> 4.1e-13
        l96_damped20     1.53e-14 -> 3.9e-12   4.30e-15 -> 1.1e-12     1.10e-14 -> 2.8e-12     states of size 10-15
        l96_damped67     2.48e-14 -> 6.3e-12   1.00e-14 -> 2.6e-12     (k_lyap stops at D = 64)
        l96_colparams    1.38e-14 -> 3.5e-12   4.51e-15 -> 1.2e-12     4.65e-15 -> 1.2e-12

    The kinked models' float64 and longdouble runs take the same branches: their switching arguments stay 1.3e-5 (stencil)
    and 1.9e-4 (small) from every threshold (Kinks, asserted >= MARGIN by the tests), far more than the two runs differ by.
    The horizon is the neighbouring files' 40 steps of dt = 0.025 for every model; do not lengthen it without deriving again.
    Returns dict(x=, tlm=, lyap=) of the measured figures (lyap None where the model has no Lyapunov case)."""
    ex = et = 0.0
    for s, e in PAIRS_TLM:
        a, b = tangent_reference(name, s, e), tangent_reference(name, s, e, dtype=np.longdouble)
        ex = max(ex, float(np.abs(np.asarray(a[0], dtype=np.longdouble) - b[0]).max()))
        et = max(et, row_error(np.asarray(a[1], dtype=np.longdouble), b[1]))
    el = None
    for K, s, q, g in lyap_cases(name):
        el = max(el or 0.0, lyap_error(lyap_reference(name, K, s, q, g), lyap_reference(name, K, s, q, g, dtype=np.longdouble)))
    if verbose:
        print("%s: float64 vs longdouble  x %.2e  tlm (relative per row) %.2e  lyap %s   x 250 = %.2e  %.2e  %s"
              % (name, ex, et, "-" if el is None else "%.2e" % el, 250 * ex, 250 * et, "-" if el is None else "%.2e" % (250 * el)))
    return dict(x=ex, tlm=et, lyap=el)


# ---------------------------------------------------------------------------------------------------------------
# Hessian-vector cases: a case dict as tests/_hvp_run.host_hv and the device tests take them
def hvp_case_N(name):
    return 9 if model(name).D == 67 else 7


@functools.lru_cache(maxsize=None)
def hvp_case(name, disc, t_start=T_HVP):
    """N = 7 (9 at D = 67), observed columns [0, 2], t_model = t_start + dt arange(N), a stimulus where the model has one, two
    points with fixed parameters of their own, directions: two random ones and the unit vector of every estimated parameter;
    `want`, `want_gn` from tests/_hess_torch_ref.TorchAction through the torch binding"""
    import _hess_torch_ref as htr
    m, tc = model(name), traj_case(name)
    D, NP, N, Pidx = m.D, m.NP, hvp_case_N(name), tc["Pidx"]
    rng = np.random.RandomState(900 + SEEDS[name])
    n, npts = N * D + len(Pidx), 2
    big = name.startswith("l96")
    P = (K_TRUE + 0.5 * rng.randn(npts, NP) if m.colparams else np.array([K_TRUE, 1.0]) + 0.1 * rng.rand(npts, 2)) if big \
        else 0.6 + 0.8 * rng.rand(npts, NP)
    X = (3.0 if big else 0.8) * rng.randn(npts, n)
    X[:, N * D:] = P[:, Pidx] + 0.1 * rng.rand(npts, len(Pidx))
    V = np.zeros((npts, 2 + len(Pidx), n))
    V[:, :2] = rng.randn(npts, 2, n)
    for e in range(len(Pidx)):
        V[:, 2 + e, N * D + e] = 1.0
    stim = np.sin(0.7 * np.arange(N)) + 0.3 if m.nstim else None
    c = dict(name=name, D=D, N=N, disc=disc, nskip=1, Lidx=[0, 2], Pidx=Pidx, Y=(3.0 if big else 1.0) * rng.randn(N, 2), RM=2.0, RF0=0.7,
             P=P, X=X, V=V, rf_scale=2.0, dt=hr.DT, stim=stim, t_model=t_start + hr.DT * np.arange(N))
    ta = htr.TorchAction(m.torch, D, N, c["Y"], c["Lidx"], c["dt"], c["RM"], c["RF0"] * c["rf_scale"], P[0], Pidx, disc,
                         t_model=c["t_model"], stim=stim)
    c["want"], c["want_gn"] = ta.products(X, V, P)
    if m.kinked:
        Pfull = P.copy()
        Pfull[:, Pidx] = X[:, N * D:]
        c["margin"] = min(float(np.abs(m.switch_slices(c["t_model"], X[k, :N * D].reshape(N, D), Pfull[k], stim)).min())
                          for k in range(npts))
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c
