"""The shooting kernel's problem family and its reference (shared by tests/test_shoot_cpu.py and
tests/test_gpu_shoot_device.py).

Lorenz-96 with the constants of _predict_ref; N = 21 rows (20 steps of DT), all columns observed, weights 1 / (L N).  Point
j of a case: truth = attractor state j, data = the truth's trajectory + 0.05 randn, start = truth + 1e-2 randn with k = 8.0,
both drawn from RandomState(100 + j), the data first.  T = 7 points (2 at D = 130).

Reference: SciPy's L-BFGS-B with Annealer.SHOOT_OPT_ARGS around _adj_ref.misfit_rk4, one point at a time, computed once per
process and left unchanged.  reference(D) returns per point: x (n,), cost, nfev, nit, status, and gmax, the largest
gradient entry at x recomputed by misfit_rk4."""
import numpy as np
from scipy.optimize import minimize

import _adj_ref
from _predict_ref import DT, K_TRUE, attractor_starts, l96, rk4

SHOOT_OPT_ARGS = dict(ftol=1e-15, gtol=1e-9)      # va_ode.Annealer.SHOOT_OPT_ARGS (test_gpu_shoot_device.py checks that they agree)
N_ROWS, K_START, NOISE, OFF = 21, 8.0, 0.05, 1e-2
WIDTHS = {5: 7, 20: 7, 33: 7, 130: 2}             # D -> points

_cases, _refs = {}, {}


def _build(D, T):
    truth = attractor_starts(D, T)
    Y, x0 = np.empty((T, N_ROWS, D)), np.empty((T, D))
    for j in range(T):
        rng = np.random.RandomState(100 + j)
        Y[j] = rk4(l96, truth[j], K_TRUE, N_ROWS - 1, DT) + NOISE * rng.randn(N_ROWS, D)
        x0[j] = truth[j] + OFF * rng.randn(D)
    c = dict(truth=np.array(truth), Y=Y, x0=x0, k=np.full(T, K_START), w=np.full(D, 1.0 / (D * N_ROWS)))
    for v in c.values():
        v.setflags(write=False)
    return c


def case(D):
    """dict: truth (T, D), Y (T, N, D), x0 (T, D) the starts, k (T,), w (D,)"""
    if D not in _cases:
        _cases[D] = _build(D, WIDTHS[D])
    return _cases[D]


_wide = {}


def wide_case(D, T=2):
    """the same family at a width outside WIDTHS (the wide lane geometries of _forecast_shapes.SHOOT_WIDE), for runs that
    stop at a budget: there is no convergence reference at these widths and reference() does not take them"""
    if (D, T) not in _wide:
        _wide[(D, T)] = _build(D, T)
    return _wide[(D, T)]


def misfit(D, z, Y):
    """(cost, gradient (D + 1,)) at z = [x0 | k] by the NumPy adjoint"""
    w = np.full(D, 1.0 / (D * N_ROWS))                # (case(D)["w"], at any width)
    c, gx, gp, _ = _adj_ref.misfit_rk4(l96, _adj_ref.l96_vjp, _adj_ref.l96_pgrad, z[:D], z[D], Y, range(D), w, N_ROWS - 1, DT)
    return c, np.append(gx, gp)


def reference(D):
    if D not in _refs:
        _adj_ref.self_check()
        c = case(D)
        out = []
        for j in range(len(c["x0"])):
            opt = minimize(lambda z: misfit(D, z, c["Y"][j]), np.append(c["x0"][j], c["k"][j]), method="L-BFGS-B", jac=True,
                           options=dict(SHOOT_OPT_ARGS))
            out.append(dict(x=opt.x, cost=float(opt.fun), nfev=int(opt.nfev), nit=int(opt.nit), status=int(opt.status),
                            gmax=float(np.abs(misfit(D, opt.x, c["Y"][j])[1]).max())))
        _refs[D] = out
    return _refs[D]


# What reference() gives on these inputs (measured once on the CPU, printed by `python tests/_shoot_cases.py`); the tests'
# bounds are built from these three quantities per point, never from the code under test:
#   GRAD_FACTOR   the returned point's largest gradient entry may be this many times the largest the reference leaves on
#                 the same case (test_gpu_shoot.py's practice with CPU_X0_ERR)
#   NFEV_FACTOR   evaluations against the reference's on the same point.  A cap, so that a degenerate minimiser (steepest
#                 descent inside the large budget) cannot pass: the method is the same, only the rounding differs.
#   cost margin   the stop rule ends an iteration whose decrease is <= ftol max(|f|, 1) = 1e-15, so two runs of the same
#                 method that both stopped by it differ by a few 1e-15 per iteration actually taken: 4e-15 x the larger of
#                 the two iteration counts.
GRAD_FACTOR, NFEV_FACTOR, COST_PER_ITER = 10.0, 2.0, 4e-15


def check_point(D, j, got, label=""):
    """criteria (1) of one point: got = dict(x0, k, cost, cost_start, nit, nfev, status)"""
    ref = reference(D)
    rj = ref[j]
    z = np.append(got["x0"], got["k"])
    c, g = misfit(D, z, case(D)["Y"][j])
    gmax, ref_gmax = float(np.abs(g).max()), max(r["gmax"] for r in ref)
    margin = COST_PER_ITER * max(int(got["nit"]), rj["nit"], 1)
    print("%sD=%d point %d: status %d, cost %.17g from %.6g (reference %.17g, margin %.1e), largest gradient entry %.3e (reference's "
          "largest on the case %.3e), nfev %d (reference %d), nit %d (reference %d)"
          % (label, D, j, got["status"], got["cost"], got["cost_start"], rj["cost"], margin, gmax, ref_gmax, got["nfev"], rj["nfev"],
             got["nit"], rj["nit"]))
    assert got["status"] == 0
    assert got["cost"] <= got["cost_start"]
    assert got["cost"] <= rj["cost"] + margin
    assert abs(got["cost"] - c) <= _adj_ref.TOL_ADJ * c
    assert gmax <= GRAD_FACTOR * ref_gmax
    assert got["nfev"] <= NFEV_FACTOR * rj["nfev"]


if __name__ == "__main__":
    for D in WIDTHS:
        r = reference(D)
        print("D=%d: status %s, nfev %s, nit %s, largest gradient entry %.2e, cost %.3e .. %.3e from %.3e .. %.3e"
              % (D, [q["status"] for q in r], [q["nfev"] for q in r], [q["nit"] for q in r], max(q["gmax"] for q in r),
                 min(q["cost"] for q in r), max(q["cost"] for q in r),
                 min(misfit(D, np.append(case(D)["x0"][j], K_START), case(D)["Y"][j])[0] for j in range(len(r))),
                 max(misfit(D, np.append(case(D)["x0"][j], K_START), case(D)["Y"][j])[0] for j in range(len(r)))))
