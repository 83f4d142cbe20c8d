"""GPU: va_ode.Annealer.shoot -- the strong-constraint refinement around the adjoint predictor's misfit mode
(csrc/va_predict_adj.h) -- on a twin problem and after a small anneal, and Annealer.predict_vjp."""
import numpy as np
import pytest
from scipy.optimize import minimize

import _adj_ref
from _predict_ref import DT, K_TRUE, attractor_starts, l96, rk4
from varanneal_amd import va_ode

pytestmark = pytest.mark.gpu


def _l96_user(t, x, k):
    return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - x + k


D_TWIN, N_TWIN, K_START = 5, 21, 8.0


def _twin():
    """(truth x(t_0), noise-free data (N, D), the start: truth + 1e-3 randn)"""
    truth = attractor_starts(D_TWIN, 3)[2]
    Y = rk4(l96, truth, K_TRUE, N_TWIN - 1, DT)
    return truth, Y, truth + 1e-3 * np.random.RandomState(8).randn(D_TWIN)


def cpu_twin_recovery():
    """what SciPy's L-BFGS-B (shoot's options) reaches on the twin problem when driven by the NumPy adjoint of _adj_ref:
    (largest |x0 - truth|, |k - K_TRUE|, final cost)"""
    truth, Y, start = _twin()
    w = np.full(D_TWIN, 1.0 / (D_TWIN * N_TWIN))

    def fun(z):
        c, gx, gp, _ = _adj_ref.misfit_rk4(l96, _adj_ref.l96_vjp, _adj_ref.l96_pgrad, z[:D_TWIN], z[D_TWIN], Y, range(D_TWIN), w,
                                           N_TWIN - 1, DT)
        return c, np.append(gx, gp)
    opt = minimize(fun, np.append(start, K_START), method="L-BFGS-B", jac=True, options=dict(va_ode.Annealer.SHOOT_OPT_ARGS))
    return np.abs(opt.x[:D_TWIN] - truth).max(), abs(opt.x[D_TWIN] - K_TRUE), opt.fun


CPU_X0_ERR, CPU_K_ERR = 6.8e-9, 8.2e-9


def test_twin_problem_is_recovered():
    """Lorenz-96, D = 5, N = 21, all columns observed, noise-free data from an attractor state with k = 8.17; the start is
    that state plus 1e-3 randn with k = 8.0 (rung 0 of an initialised annealer holds it).  shoot reports success,
    cost < cost_start, path is Problem.predict's bit for bit, and x0 and k are recovered within ten times what the same SciPy
    call (shoot's stopping options) reaches when driven by the NumPy adjoint on the CPU (cpu_twin_recovery(), measured:
    |x0 - truth| <= 6.8e-9, |k - 8.17| = 8.2e-9, cost 4.8e-18, from a start 2.3e-3 and 0.17 away), i.e. 6.8e-8 and 8.2e-8."""
    truth, Y, start = _twin()
    X0 = np.array(Y)
    X0[0] = start
    a = va_ode.Annealer()
    a.set_model(_l96_user, D_TWIN)
    a.set_data(Y, t=DT * np.arange(N_TWIN))
    a.anneal_init(X0, np.array([K_START]), 2.0, [0], 1.0, 1.0, list(range(D_TWIN)), [0], disc="trapezoid")
    r = a.shoot(beta=0)
    assert r["x0"].shape == (1, D_TWIN) and r["params"].shape == (1, 1) and r["path"].shape == (1, N_TWIN, D_TWIN)
    ex, ek = np.abs(r["x0"][0] - truth).max(), abs(r["params"][0, 0] - K_TRUE)
    print("twin: status %d after %d evaluations, cost %.3e from %.3e, |x0 - truth| = %.3e, |k - 8.17| = %.3e, largest gradient entry %.3e"
          % (r["status"][0], r["nfev"][0], r["cost"][0], r["cost_start"][0], ex, ek, r["grad_norm"][0]))
    assert r["status"][0] == 0 and r["cost"][0] < r["cost_start"][0]
    assert np.array_equal(r["path"][0], a._pb.predict(r["x0"][0], r["params"][0], N_TWIN - 1)[0])
    assert ex <= 10 * CPU_X0_ERR and ek <= 10 * CPU_K_ERR
    assert np.isfinite(r["path_distance"][0])
    a.close()


def test_after_a_small_anneal():
    """the D = 5, N = 9 anneal of test_gpu_predict_tlm.py's end-to-end test (two seeds, two rungs): cost is the measurement
    term the action evaluator reports for [path | params], cost <= cost_start, path_distance is finite; predict_vjp agrees
    with Problem.predict_adjoint from the last row; time-dependent parameters are refused"""
    D, N, B = 5, 9, 2
    rng = np.random.RandomState(6)
    Lidx, RM, RF0, alpha = [0, 2, 3], 4.0, 0.5, 2.0
    Y = 2.0 * rng.randn(N, len(Lidx))
    a = va_ode.Annealer()
    a.set_model(_l96_user, D)
    a.set_data(Y, t=DT * np.arange(N))
    a.anneal(rng.randn(B, N, D), np.array([[8.0], [8.5]]), alpha, [0, 1], RM, RF0, Lidx, [0], disc="trapezoid", verbose=False,
             opt_args={'gtol': 1e-10, 'ftol': 1e-14})
    r = a.shoot(beta=None)
    assert r["path"].shape == (B, 2, N, D) and r["cost"].shape == r["status"].shape == (B, 2)
    XP = np.concatenate([r["path"].reshape(B * 2, N * D), r["params"].reshape(B * 2, 1)], axis=1)
    for j in range(B * 2):
        me = a._pb.action_grad(np.tile(XP[j], (B, 1)), 1.0, want_grad=False)[1][0]
        c = r["cost"].reshape(-1)[j]
        print("point %d: cost %.17g, the action's measurement term %.17g, cost_start %.6g, path_distance %.3g"
              % (j, c, me, r["cost_start"].reshape(-1)[j], r["path_distance"].reshape(-1)[j]))
        assert abs(c - me) <= 1e-12 * me
    assert np.all(r["cost"] <= r["cost_start"]) and np.all(np.isfinite(r["path_distance"]))
    one = a.shoot(beta=1, seeds=[1])
    assert np.array_equal(one["path"][0, 0], r["path"][1, 1]) and one["cost"][0, 0] == r["cost"][1, 1]
    # predict_vjp: cotangent mode from the last fitted row
    n_fc, every = 12, 4
    G = np.random.RandomState(3).randn(2, n_fc // every + 1, D)
    v = a.predict_vjp(G, n_fc, every=every)
    mp = a.minpaths.reshape(B * 2, -1)
    ref = a._pb.predict_adjoint(mp[:, (N - 1) * D:N * D], mp[:, N * D:], n_fc, G=np.ascontiguousarray(np.broadcast_to(G, (B * 2,) + G.shape)),
                                t0=float(a.t_model[-1]), every=every)
    assert v["gx0"].shape == (B, 2, 2, D) and v["gp"].shape == (B, 2, 2, 1)
    for k in ("out", "gx0", "gp"):
        assert np.array_equal(v[k].reshape(ref[k].shape), ref[k])
    assert np.array_equal(v["out"], a.predict(n_fc, every=every))
    # time-dependent parameters (the flag anneal_init sets for a parameter array with a time axis) have no single model
    # trajectory: refused before anything is launched
    a._tdp = True
    with pytest.raises(NotImplementedError, match="time-dependent"):
        a.shoot()
    with pytest.raises(NotImplementedError, match="time-dependent"):
        a.predict_vjp(G, n_fc, every=every)
    a._tdp = False
    a.close()
