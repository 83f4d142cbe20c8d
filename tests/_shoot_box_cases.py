"""The boxed shooting kernel's problem family and its reference (shared by tests/test_shoot_box_cpu.py and
tests/test_gpu_shoot_box.py).

The family is _shoot_cases.case(D) with a box per point j (n = D + 1 entries: the D start values, then k):
    lower[0:D:2] = x0_start[0:D:2] - 0.005      (every second state from below)
    upper[1:D:4] = x0_start[1:D:4] + 0.02       (every fourth from above)
    7.0 <= k <= 8.05                            (the truth is K_TRUE = 8.17, the start 8.0: the fit ends ON the upper bound)
    everything else unbounded (-inf / +inf)

Reference: SciPy's L-BFGS-B with these bounds and SHOOT_OPT_ARGS around _shoot_cases.misfit, one point at a time, computed
once per process and left unchanged.  What it gives on these inputs (measured on the CPU, printed by
`python tests/_shoot_box_cases.py`): every point ends with status 0 and k == 8.05, and

    D    state entries on a bound   nfev        nit         largest projected-gradient entry left
    5    1 to 4                     12 to 33    9 to 26     3.4e-9
    20   4 to 7                     31 to 49    29 to 44    1.4e-8
    33   5 to 11                    60 to 121   58 to 107   9.1e-8

check_point's caps are _shoot_cases' three factors around these reference quantities, never around the code under test.

One box is not the recipe's (REPLACED).  D = 5, point 0, with the recipe's box: the reference and the host emulation of the
kernel (tests/test_shoot_box_cpu.py) take the same 27 evaluations to the same iterate with the same active set (entry 1 on
its upper bound, k on 8.05; cost 2.5454282889658324e-3 by NumPy, ...825e-3 by the emulation), where the projected
gradient has fallen from 2.7e-7 to 1.42e-9 in one step: above gtol = 1e-9, with any further decrease (about 1e-19) below
the cost's rounding noise (1e-18).  The line search from there works on noise.  SciPy's sixth trial happens to return the
iterate's cost to the last bit and is accepted (nfev 33, nit 22, status 0); the emulation's trials do not, it uses up
maxls twice and ends with status 2 at the same point, its cost 7e-18 BELOW the reference's, after 67 evaluations
(the cap is 2 x 33).  That is the two roundings parting at the noise floor, not in the active set; the remedy is the one
for roundings that part: no cap is widened, and that point's lower offset is 0.004 instead of 0.005, the first of
(0.004, 0.006, 0.003) tried.  With it the reference ends with the same active set, status 0, nfev 28, nit 22, largest
projected-gradient entry 3.4e-10 (so D = 5's ranges become nfev 12 to 31, nit 9 to 26), and the emulation follows it
evaluation for evaluation."""
import numpy as np
from scipy.optimize import minimize

import _adj_ref
import _shoot_cases as sc
from _shoot_cases import COST_PER_ITER, GRAD_FACTOR, NFEV_FACTOR, SHOOT_OPT_ARGS

K_LO, K_HI = 7.0, 8.05
LO_OFF, HI_OFF = 0.005, 0.02
WIDTHS = {5: 7, 20: 7, 33: 7}             # D -> points (reference widths)
REPLACED = {(5, 0): 0.004}                # (D, point) -> lower offset in LO_OFF's place (the docstring says why)

_boxes, _refs = {}, {}


def box_of(x0):
    """(lower, upper), each (T, D + 1), by the recipe above around the starts x0 (T, D)"""
    T, D = x0.shape
    lo, hi = np.full((T, D + 1), -np.inf), np.full((T, D + 1), np.inf)
    lo[:, 0:D:2] = x0[:, 0:D:2] - LO_OFF
    hi[:, 1:D:4] = x0[:, 1:D:4] + HI_OFF
    lo[:, D], hi[:, D] = K_LO, K_HI
    return lo, hi


def box(D):
    if D not in _boxes:
        x0 = sc.case(D)["x0"] if D in sc.WIDTHS else sc.wide_case(D)["x0"]
        lo, hi = box_of(x0)
        for (Dr, j), off in REPLACED.items():
            if Dr == D:
                lo[j, 0:D:2] = x0[j, 0:D:2] - off
        lo.setflags(write=False)
        hi.setflags(write=False)
        _boxes[D] = (lo, hi)
    return _boxes[D]


def projected_gradient(z, g, lo, hi):
    """L-BFGS-B's projgr, entry by entry"""
    return np.where(g < 0.0, np.maximum(z - hi, g), np.minimum(z - lo, g))


def on_bound(z, lo, hi):
    return (z == lo) | (z == hi)


def reference(D):
    """per point: x (n,), cost, nfev, nit, status, pgmax (largest projected-gradient entry at x by the NumPy adjoint),
    active (boolean (n,): entries on a bound)"""
    if D not in _refs:
        _adj_ref.self_check()
        c = sc.case(D)
        lo, hi = box(D)
        out = []
        for j in range(len(c["x0"])):
            opt = minimize(lambda z: sc.misfit(D, z, c["Y"][j]), np.append(c["x0"][j], c["k"][j]), method="L-BFGS-B", jac=True,
                           bounds=list(zip(lo[j], hi[j])), options=dict(SHOOT_OPT_ARGS))
            g = sc.misfit(D, opt.x, c["Y"][j])[1]
            out.append(dict(x=opt.x, cost=float(opt.fun), nfev=int(opt.nfev), nit=int(opt.nit), status=int(opt.status),
                            pgmax=float(np.abs(projected_gradient(opt.x, g, lo[j], hi[j])).max()), active=on_bound(opt.x, lo[j], hi[j])))
        _refs[D] = out
    return _refs[D]


def check_point(D, j, got, label=""):
    """one point under the reference's caps: got = dict(x0, k, cost, cost_start, nit, nfev, status)"""
    ref = reference(D)
    rj = ref[j]
    lo, hi = box(D)
    z = np.append(got["x0"], got["k"])
    c, g = sc.misfit(D, z, sc.case(D)["Y"][j])
    pgmax, ref_pgmax = float(np.abs(projected_gradient(z, g, lo[j], hi[j])).max()), max(r["pgmax"] for r in ref)
    margin = COST_PER_ITER * max(int(got["nit"]), rj["nit"], 1)
    act = on_bound(z, lo[j], hi[j])
    print("%sD=%d point %d: status %d, cost %.17g from %.6g (reference %.17g, margin %.1e), largest projected-gradient entry %.3e "
          "(reference's largest on the case %.3e), nfev %d (reference %d), nit %d (reference %d), k %.17g, on a bound %s (reference %s)"
          % (label, D, j, got["status"], got["cost"], got["cost_start"], rj["cost"], margin, pgmax, ref_pgmax, got["nfev"], rj["nfev"],
             got["nit"], rj["nit"], got["k"], list(np.flatnonzero(act)), list(np.flatnonzero(rj["active"]))))
    assert got["status"] == 0
    assert np.all(z >= lo[j]) and np.all(z <= hi[j])
    assert got["k"] == K_HI
    assert got["cost"] <= got["cost_start"]
    assert got["cost"] <= rj["cost"] + margin
    assert abs(got["cost"] - c) <= _adj_ref.TOL_ADJ * c
    assert pgmax <= GRAD_FACTOR * ref_pgmax
    assert got["nfev"] <= NFEV_FACTOR * rj["nfev"]


if __name__ == "__main__":
    for D in WIDTHS:
        r = reference(D)
        print("D=%d: status %s, k %s, state entries on a bound %s, nfev %s, nit %s, largest projected-gradient entry %.2e, cost %.3e .. %.3e"
              % (D, [q["status"] for q in r], sorted(set(q["x"][D] for q in r)), [int(q["active"][:D].sum()) for q in r],
                 [q["nfev"] for q in r], [q["nit"] for q in r], max(q["pgmax"] for q in r), min(q["cost"] for q in r), max(q["cost"] for q in r)))
