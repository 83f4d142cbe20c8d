"""GPU: the shooting kernel k_shoot (csrc/va_shoot.h) through _capi.Problem.shoot and va_ode.Annealer.shoot(device=True):
the problem family, reference and bounds of tests/_shoot_cases.py (the ones tests/test_shoot_cpu.py holds the host emulation
to), a generated module with a stimulus and more estimated parameters than lanes per point, and the annealer's route.  Each
device call of the kernel stands in a test of its own."""
import numpy as np
import pytest

import _shoot_cases as sc
from _adj_ref import TOL_ADJ
from _predict_ref import DT, K_TRUE, STEPS, l96, rk4
from models.nakl import nakl
from test_gpu_predict_adj import NAKL_ADJ_TOL
from test_gpu_predict_tlm import PIDX_NAKL, _nakl_case
from test_gpu_shoot import CPU_K_ERR, CPU_X0_ERR, D_TWIN, K_START, N_TWIN, _l96_user, _twin
from varanneal_amd import _capi, codegen, va_ode

pytestmark = pytest.mark.gpu

KEYS = ("x0", "p", "cost", "cost_start", "grad_max", "nit", "nfev", "status")
OPTS = dict(sc.SHOOT_OPT_ARGS)


def _handle(D):
    N = sc.N_ROWS
    return _capi.Problem(1, D, N, np.zeros((N, D)), list(range(D)), DT, 4.0, 1e-2, np.array([[K_TRUE]]), [0])


def _shoot(D, x0, k, Y, **kw):
    with _handle(D) as pb:
        return pb.shoot(x0, np.asarray(k, dtype=np.float64).reshape(-1, 1), sc.N_ROWS - 1, Y, sc.case(D)["w"], **dict(OPTS, **kw))


def _point(r, j):
    return dict(x0=r["x0"][j], k=r["p"][j, 0], cost=r["cost"][j], cost_start=r["cost_start"][j], nit=r["nit"][j], nfev=r["nfev"][j],
                status=r["status"][j])


_first = {}


def _case_run(D):
    if D not in _first:
        c = sc.case(D)
        _first[D] = _shoot(D, c["x0"], c["k"], c["Y"])
    return _first[D]


def test_options_are_the_annealers():
    assert sc.SHOOT_OPT_ARGS == va_ode.Annealer.SHOOT_OPT_ARGS


@pytest.mark.parametrize("D", [5, 20, 33, 130])
def test_convergence(D):
    """(a) the cases and criteria of tests/test_shoot_cpu.py::test_convergence on the device: D = 5 a wave of six points and
    one beside idle slots, D = 20 one wave per point, D = 33 128 threads with barriers, D = 130 (two points) E = 2.  The
    reference's figures on these inputs stand in that test's docstring."""
    r = _case_run(D)
    assert sorted(r) == sorted(KEYS) and r["x0"].shape == (sc.WIDTHS[D], D) and r["p"].shape == (sc.WIDTHS[D], 1)
    for j in range(sc.WIDTHS[D]):
        sc.check_point(D, j, _point(r, j), "device ")


@pytest.mark.parametrize("D", [5, 20, 33, 130])
def test_second_call_gives_the_same_bits(D):
    c, r = sc.case(D), _case_run(D)
    again = _shoot(D, c["x0"], c["k"], c["Y"])
    for k in KEYS:
        assert np.array_equal(r[k], again[k]), k


@pytest.mark.parametrize("D", [5, 20, 33, 130])
def test_cost_is_predict_adjoints_at_the_returned_point(D):
    c, r = sc.case(D), _case_run(D)
    with _handle(D) as pb:
        a = pb.predict_adjoint(r["x0"], r["p"], sc.N_ROWS - 1, Y=c["Y"], weights=c["w"])
    gmax = np.maximum(np.abs(a["gx0"][:, 0]).max(axis=1), np.abs(a["gp"][:, 0]).max(axis=1))
    print("D=%d: cost bit-equal to predict_adjoint's at the returned point: %s (largest relative difference %.3e); grad_max bit-equal: %s"
          % (D, np.array_equal(a["cost"], r["cost"]), (np.abs(a["cost"] - r["cost"]) / a["cost"]).max(), np.array_equal(gmax, r["grad_max"])))
    assert np.all(np.abs(a["cost"] - r["cost"]) <= TOL_ADJ * a["cost"])


def test_a_finished_point_is_frozen():
    """(b) tests/test_shoot_cpu.py's (3) on the device: point 2 of the D = 5 wave starts at its minimum and stops at the
    first evaluation, unchanged bit for bit, while its wave goes on; the others still meet (1)"""
    c = sc.case(5)
    x0, k, Y = c["x0"].copy(), c["k"].copy(), c["Y"].copy()
    x0[2], k[2] = c["truth"][2], K_TRUE
    Y[2] = rk4(l96, c["truth"][2], K_TRUE, sc.N_ROWS - 1, DT)
    r = _shoot(5, x0, k, Y)
    print("point 2: status %d nit %d nfev %d cost %.3e grad_max %.3e" % (r["status"][2], r["nit"][2], r["nfev"][2], r["cost"][2], r["grad_max"][2]))
    assert (r["status"][2], r["nit"][2], r["nfev"][2]) == (0, 0, 1)
    assert np.array_equal(r["x0"][2], x0[2]) and r["p"][2, 0] == k[2] and r["cost"][2] == r["cost_start"][2]
    for j in (0, 1, 3, 4, 5, 6):
        sc.check_point(5, j, _point(r, j), "device, beside a frozen point ")


def test_non_finite_start():
    """(b) tests/test_shoot_cpu.py's (5) on the device: status 3, the point unchanged, the neighbours' bits those of the clean run"""
    c, clean = sc.case(5), _case_run(5)
    x0 = c["x0"].copy()
    x0[1, 0] = 1e200
    r = _shoot(5, x0, c["k"], c["Y"])
    assert r["status"][1] == 3 and r["nit"][1] == 0 and r["nfev"][1] == 1 and not np.isfinite(r["cost"][1])
    assert np.array_equal(r["x0"][1], x0[1]) and r["p"][1, 0] == c["k"][1]
    for j in (0, 2, 3, 4, 5, 6):
        for k in KEYS:
            assert np.array_equal(r[k][j], clean[k][j]), (j, k)


def test_budget():
    """tests/test_shoot_cpu.py's (4) on the device: maxfun = 5"""
    c = sc.case(5)
    r = _shoot(5, c["x0"], c["k"], c["Y"], maxfun=5)
    for j in range(7):
        cost = sc.misfit(5, np.append(r["x0"][j], r["p"][j, 0]), c["Y"][j])[0]
        assert r["status"][j] == 1 and r["nfev"][j] <= 6 and r["cost"][j] <= r["cost_start"][j]
        assert abs(r["cost"][j] - cost) <= TOL_ADJ * cost


def test_generated_module_with_stimulus_and_many_parameters():
    """(c) NaKL (D = 4: eight lanes a point, eight points to a wave, seven live) with a moving stimulus and four estimated
    parameters reached through PIDX_NAKL, maxfun = 30; the data are the model's own trajectories from parameters 1 % off.
    cost <= cost_start, and cost and the largest gradient entry the kernel reports at the returned point are
    predict_adjoint's there within NAKL_ADJ_TOL relative: a stimulus lane, a partial sum or a cost share that is not
    re-armed between evaluations shows in either."""
    k = _nakl_case()
    D, NP, dt = k["D"], k["NP"], k["dt"]
    T = len(k["x0"])
    m = codegen.module_for(nakl, D, NP, nstim=1, stim_ndim=1)
    Nh = 5
    Lidx = [0]
    w = np.array([1.0 / (STEPS + 1)])
    Ptrue = k["P"].copy()
    Ptrue[:, PIDX_NAKL] *= 1.01
    with _capi.Problem(1, D, Nh, np.zeros((Nh, 1)), Lidx, dt, 1.0, 1.0, k["P"][:1], PIDX_NAKL, rhs=_capi.load_rhs_module(m["so"]),
                       t_model=dt * np.arange(Nh), stim=np.zeros(Nh)) as pb:
        Y = np.ascontiguousarray(pb.predict(k["x0"], Ptrue, STEPS, t0=k["t0"], stim=k["stim"])[:, :, Lidx])
        r = pb.shoot(k["x0"], k["P"], STEPS, Y, w, t0=k["t0"], stim=k["stim"], maxfun=30, **OPTS)
        a = pb.predict_adjoint(r["x0"], r["p"], STEPS, Y=Y, weights=w, t0=k["t0"], stim=k["stim"])
    gmax = np.maximum(np.abs(a["gx0"][:, 0]).max(axis=1), np.abs(a["gp"][:, 0]).max(axis=1))
    print("NaKL: status %s nfev %s nit %s, cost %s from %s; |cost - predict_adjoint's| / cost <= %.3e, |grad_max - predict_adjoint's| / it <= %.3e"
          % (r["status"], r["nfev"], r["nit"], r["cost"], r["cost_start"], (np.abs(r["cost"] - a["cost"]) / a["cost"]).max(),
             (np.abs(r["grad_max"] - gmax) / gmax).max()))
    assert r["p"].shape == (T, NP) and np.all(r["nfev"] <= 31)
    other = [i for i in range(NP) if i not in PIDX_NAKL]
    assert np.array_equal(r["p"][:, other], k["P"][:, other])
    assert np.all(r["cost"] <= r["cost_start"]) and np.all(r["nit"] >= 1)
    assert np.all(np.abs(r["cost"] - a["cost"]) <= NAKL_ADJ_TOL * a["cost"])
    assert np.all(np.abs(r["grad_max"] - gmax) <= NAKL_ADJ_TOL * gmax)


def test_annealer_twin_problem_on_the_device():
    """(d) tests/test_gpu_shoot.py's twin problem through Annealer.shoot(beta=0, device=True): x0 and k recovered within that
    test's 10 CPU_X0_ERR and 10 CPU_K_ERR, path bit-equal to predict()"""
    truth, Y, start = _twin()
    X0 = np.array(Y)
    X0[0] = start
    a = va_ode.Annealer()
    a.set_model(_l96_user, D_TWIN)
    a.set_data(Y, t=DT * np.arange(N_TWIN))
    a.anneal_init(X0, np.array([K_START]), 2.0, [0], 1.0, 1.0, list(range(D_TWIN)), [0], disc="trapezoid")
    r = a.shoot(beta=0, device=True)
    assert r["x0"].shape == (1, D_TWIN) and r["params"].shape == (1, 1) and r["path"].shape == (1, N_TWIN, D_TWIN)
    ex, ek = np.abs(r["x0"][0] - truth).max(), abs(r["params"][0, 0] - K_TRUE)
    print("twin on the device: status %d after %d evaluations and %d iterations, cost %.3e from %.3e, |x0 - truth| = %.3e, |k - 8.17| = %.3e, "
          "largest gradient entry %.3e" % (r["status"][0], r["nfev"][0], r["nit"][0], r["cost"][0], r["cost_start"][0], ex, ek, r["grad_norm"][0]))
    assert r["status"][0] == 0 and r["cost"][0] < r["cost_start"][0]
    assert np.array_equal(r["path"][0], a._pb.predict(r["x0"][0], r["params"][0], N_TWIN - 1)[0])
    assert ex <= 10 * CPU_X0_ERR and ek <= 10 * CPU_K_ERR
    assert np.isfinite(r["path_distance"][0])
    a.close()


def test_annealer_after_a_small_anneal_on_the_device():
    """(e) the two-seed, two-rung anneal of tests/test_gpu_shoot.py: shoot(beta=None, device=True) has the documented shapes
    and keys (the host route's plus nit), cost is the action's measurement term at [path | params] within 1e-12 relative;
    an unknown opt_args key raises ValueError naming it; an annealer with bounds raises NotImplementedError"""
    D, N, B = 5, 9, 2
    rng = np.random.RandomState(6)
    Lidx, RM, RF0, alpha = [0, 2, 3], 4.0, 0.5, 2.0
    Y = 2.0 * rng.randn(N, len(Lidx))
    a = va_ode.Annealer()
    a.set_model(_l96_user, D)
    a.set_data(Y, t=DT * np.arange(N))
    a.anneal(rng.randn(B, N, D), np.array([[8.0], [8.5]]), alpha, [0, 1], RM, RF0, Lidx, [0], disc="trapezoid", verbose=False,
             opt_args={'gtol': 1e-10, 'ftol': 1e-14})
    r = a.shoot(beta=None, device=True)
    assert sorted(r) == sorted(["x0", "params", "path", "cost", "cost_start", "grad_norm", "nfev", "nit", "status", "path_distance"])
    assert r["path"].shape == (B, 2, N, D) and r["x0"].shape == (B, 2, D) and r["params"].shape == (B, 2, 1)
    for k in ("cost", "cost_start", "grad_norm", "nfev", "nit", "status", "path_distance"):
        assert r[k].shape == (B, 2), k
    XP = np.concatenate([r["path"].reshape(B * 2, N * D), r["params"].reshape(B * 2, 1)], axis=1)
    for j in range(B * 2):
        me = a._pb.action_grad(np.tile(XP[j], (B, 1)), 1.0, want_grad=False)[1][0]
        c = r["cost"].reshape(-1)[j]
        print("point %d: status %d, cost %.17g, the action's measurement term %.17g, cost_start %.6g"
              % (j, r["status"].reshape(-1)[j], c, me, r["cost_start"].reshape(-1)[j]))
        assert abs(c - me) <= 1e-12 * me
    assert np.all(r["cost"] <= r["cost_start"]) and np.all(np.isfinite(r["path_distance"]))
    with pytest.raises(ValueError, match="maxfev"):
        a.shoot(device=True, opt_args={"maxfev": 10})
    a.bounds = [(-20.0, 20.0)] * (N * D + 1)
    with pytest.raises(NotImplementedError, match="bounds"):
        a.shoot(device=True)
    a.bounds = None
    a.close()
