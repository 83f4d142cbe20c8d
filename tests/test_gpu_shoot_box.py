"""GPU: the boxed shooting kernel k_shoot_box (csrc/va_shoot_box.h) through _capi.Problem.shoot_box and
va_ode.Annealer.shoot(device=True, box=True): the problem family, boxes, reference and caps of tests/_shoot_box_cases.py (the
ones tests/test_shoot_box_cpu.py holds the host emulation to), the E = 2 geometry under a budget, a generated module with a
stimulus and a gate started on its bound, and the annealer's route against the host route.  Each device call of the kernel
stands in a test of its own (the repeat calls of (c) apart)."""
import numpy as np
import pytest

import _shoot_box_cases as bc
import _shoot_cases as sc
from _adj_ref import TOL_ADJ
from _predict_ref import DT, K_TRUE, STEPS
from models.nakl import nakl
from test_gpu_predict_tlm import PIDX_NAKL, _nakl_case
from test_gpu_shoot import _l96_user
from varanneal_amd import _capi, codegen, va_ode

pytestmark = pytest.mark.gpu

KEYS = ("x0", "p", "cost", "cost_start", "grad_max", "nit", "nfev", "status")
OPTS = dict(sc.SHOOT_OPT_ARGS)
WIDE_D = 130


def _handle(D):
    N = sc.N_ROWS
    return _capi.Problem(1, D, N, np.zeros((N, D)), list(range(D)), DT, 4.0, 1e-2, np.array([[K_TRUE]]), [0])


def _case(D):
    return sc.case(D) if D in bc.WIDTHS else sc.wide_case(D)


def _shoot_box(D, **kw):
    c = _case(D)
    lo, hi = bc.box(D)
    with _handle(D) as pb:
        return pb.shoot_box(c["x0"], c["k"].reshape(-1, 1), sc.N_ROWS - 1, c["Y"], c["w"], lo, hi, **dict(OPTS, **kw))


def _point(r, j):
    return dict(x0=r["x0"][j], k=r["p"][j, 0], cost=r["cost"][j], cost_start=r["cost_start"][j], nit=r["nit"][j], nfev=r["nfev"][j],
                status=r["status"][j])


_first = {}


def _case_run(D):
    if D not in _first:
        _first[D] = _shoot_box(D, **({"maxfun": 40} if D == WIDE_D else {}))
    return _first[D]


@pytest.mark.parametrize("D", [5, 20, 33])
def test_convergence(D):
    """(a) the cases and criteria of tests/test_shoot_box_cpu.py::test_convergence on the device: D = 5 a wave of six points
    and one beside idle slots, D = 20 one wave per point, D = 33 128 threads with barriers.  The reference's figures on these
    inputs stand in _shoot_box_cases' docstring."""
    r = _case_run(D)
    assert sorted(r) == sorted(KEYS) and r["x0"].shape == (bc.WIDTHS[D], D) and r["p"].shape == (bc.WIDTHS[D], 1)
    for j in range(bc.WIDTHS[D]):
        bc.check_point(D, j, _point(r, j), "device ")


def test_wide_geometry_under_a_budget():
    """(b) D = 130, two points, the same box recipe, maxfun = 40: 256 threads, E = 2.  There is no convergence reference at
    this width (none was run): status 1, feasible points, cost <= cost_start, and a cost that is predict_adjoint's at the
    returned point within TOL_ADJ."""
    D = WIDE_D
    c, r = _case(D), _case_run(D)
    lo, hi = bc.box(D)
    with _handle(D) as pb:
        a = pb.predict_adjoint(r["x0"], r["p"], sc.N_ROWS - 1, Y=c["Y"], weights=c["w"])
    z = np.hstack([r["x0"], r["p"]])
    print("D=%d: status %s nfev %s nit %s, cost %s from %s, entries on a bound %s, |cost - predict_adjoint's| / cost %.3e"
          % (D, r["status"], r["nfev"], r["nit"], r["cost"], r["cost_start"], bc.on_bound(z, lo, hi).sum(axis=1),
             (np.abs(a["cost"] - r["cost"]) / a["cost"]).max()))
    assert np.all(r["status"] == 1) and np.all(r["nfev"] <= 41)
    assert np.all(z >= lo) and np.all(z <= hi)
    assert np.all(r["cost"] <= r["cost_start"])
    assert np.all(np.abs(a["cost"] - r["cost"]) <= TOL_ADJ * a["cost"])


@pytest.mark.parametrize("D", [5, 20, 33, WIDE_D])
def test_second_call_gives_the_same_bits(D):
    """(c)"""
    r = _case_run(D)
    again = _shoot_box(D, **({"maxfun": 40} if D == WIDE_D else {}))
    for k in KEYS:
        assert np.array_equal(r[k], again[k]), k


def test_generated_module_with_a_gate_on_its_bound():
    """(d) NaKL (D = 4, a moving stimulus, four estimated parameters reached through PIDX_NAKL = Vtm, gNa, ENa, t2n),
    maxfun = 30: the gates m, h, n boxed to [0, 1], gNa and the time constant t2n to [0, inf), the voltage and the other two
    parameters free; every start has its m gate put ON 0.  The data are the model's own trajectories from parameters 1 % off
    (from the unmodified starts).  Feasible, cost <= cost_start, status 0 or 1, the parameters that are not estimated
    untouched."""
    k = _nakl_case()
    D, NP, dt = k["D"], k["NP"], k["dt"]
    T = len(k["x0"])
    m = codegen.module_for(nakl, D, NP, nstim=1, stim_ndim=1)
    Nh = 5
    Lidx = [0]
    w = np.array([1.0 / (STEPS + 1)])
    Ptrue = k["P"].copy()
    Ptrue[:, PIDX_NAKL] *= 1.01
    lo = [None, 0.0, 0.0, 0.0, None, 0.0, None, 0.0]
    hi = [None, 1.0, 1.0, 1.0, None, None, None, None]
    x0 = k["x0"].copy()
    x0[:, 1] = 0.0
    with _capi.Problem(1, D, Nh, np.zeros((Nh, 1)), Lidx, dt, 1.0, 1.0, k["P"][:1], PIDX_NAKL, rhs=_capi.load_rhs_module(m["so"]),
                       t_model=dt * np.arange(Nh), stim=np.zeros(Nh)) as pb:
        Y = np.ascontiguousarray(pb.predict(k["x0"], Ptrue, STEPS, t0=k["t0"], stim=k["stim"])[:, :, Lidx])
        r = pb.shoot_box(x0, k["P"], STEPS, Y, w, lo, hi, t0=k["t0"], stim=k["stim"], maxfun=30, **OPTS)
    z = np.hstack([r["x0"], r["p"][:, PIDX_NAKL]])
    flo = np.array([-np.inf if v is None else v for v in lo])
    fhi = np.array([np.inf if v is None else v for v in hi])
    print("NaKL in its box: status %s nfev %s nit %s, cost %s from %s, m gate %s, entries on a bound %s"
          % (r["status"], r["nfev"], r["nit"], r["cost"], r["cost_start"], r["x0"][:, 1], bc.on_bound(z, flo, fhi).sum(axis=1)))
    assert r["p"].shape == (T, NP) and np.all(r["nfev"] <= 31)
    other = [i for i in range(NP) if i not in PIDX_NAKL]
    assert np.array_equal(r["p"][:, other], k["P"][:, other])
    assert np.all(z >= flo) and np.all(z <= fhi) and np.all(np.isfinite(z))
    assert np.all(r["cost"] <= r["cost_start"]) and np.all(np.isin(r["status"], (0, 1)))


def test_annealer_route_matches_the_host_route():
    """(e) the two-seed, two-rung anneal of tests/test_gpu_shoot.py, then a.bounds = a box whose k interval, 0.01 wide, lies
    0.2 above every annealed k: the fit of every point ends on one of its ends.  shoot(beta=None, device=True, box=True)
    against shoot(beta=None, device=False), which hands SciPy the same bounds around the same device evaluations: params on
    the same bound as the host's (and the host's ARE on a bound), every entry inside the bounds, and
    cost <= host cost + COST_PER_ITER max(|cost|, 1) x iterations: check_point's margin, scaled as the stop rule
    ftol max(|f|, 1) scales it (these costs are not below 1 by construction), the iterations the larger of the device's nit
    and the host's nfev (the host route reports no nit; nfev bounds it from above).  box=True without device=True raises
    ValueError; without box=True the bounded annealer still raises NotImplementedError naming box=True."""
    D, N, B = 5, 9, 2
    rng = np.random.RandomState(6)
    Lidx, RM, RF0, alpha = [0, 2, 3], 4.0, 0.5, 2.0
    Y = 2.0 * rng.randn(N, len(Lidx))
    a = va_ode.Annealer()
    a.set_model(_l96_user, D)
    a.set_data(Y, t=DT * np.arange(N))
    a.anneal(rng.randn(B, N, D), np.array([[8.0], [8.5]]), alpha, [0, 1], RM, RF0, Lidx, [0], disc="trapezoid", verbose=False,
             opt_args={'gtol': 1e-10, 'ftol': 1e-14})
    with pytest.raises(ValueError, match="device=True"):
        a.shoot(box=True)
    free = a.shoot(beta=None, device=True, box=True)            # no bounds: an all-infinite box
    assert free["x0"].shape == (B, 2, D) and np.all(free["cost"] <= free["cost_start"])
    k_lo = float(np.max(a._mp[..., N * D:N * D + 1])) + 0.2
    k_hi = k_lo + 0.01
    a.bounds = [(-20.0, 20.0)] * (N * D) + [(k_lo, k_hi)]
    with pytest.raises(NotImplementedError, match="box=True"):
        a.shoot(device=True)
    r = a.shoot(beta=None, device=True, box=True)
    host = a.shoot(beta=None, device=False)
    assert sorted(r) == sorted(["x0", "params", "path", "cost", "cost_start", "grad_norm", "nfev", "nit", "status", "path_distance"])
    assert r["path"].shape == (B, 2, N, D) and r["x0"].shape == (B, 2, D) and r["params"].shape == (B, 2, 1)
    for j in range(B * 2):
        g = {k: v.reshape((B * 2,) + v.shape[2:])[j] for k, v in r.items()}
        hj = {k: v.reshape((B * 2,) + v.shape[2:])[j] for k, v in host.items()}
        margin = sc.COST_PER_ITER * max(abs(hj["cost"]), 1.0) * max(int(g["nit"]), int(hj["nfev"]), 1)
        print("point %d: device status %d nfev %d nit %d cost %.17g k %.17g | host status %d nfev %d cost %.17g k %.17g | margin %.2e"
              % (j, g["status"], g["nfev"], g["nit"], g["cost"], g["params"][0], hj["status"], hj["nfev"], hj["cost"], hj["params"][0], margin))
        assert hj["params"][0] in (k_lo, k_hi)
        assert g["params"][0] == hj["params"][0]
        assert np.all(np.abs(g["x0"]) <= 20.0)
        assert g["cost"] <= g["cost_start"] and g["cost"] <= hj["cost"] + margin
    assert np.array_equal(r["path"].reshape(-1, N, D), a._pb.predict(r["x0"].reshape(-1, D), r["params"].reshape(-1, 1), N - 1))
    a.bounds = None
    a.close()
