"""CPU: the model zoo of tests/models/zoo.py before anything of it is compared with a kernel -- the three bindings of every
model (NumPy as the user writes it, complex-safe NumPy, torch) against each other; the references of tests/_zoo_ref.py against
each other; the conditions on the inputs of tests/test_gpu_generated_tangents.py, checked on the references alone: the
kinked models' switching arguments stay away from their thresholds along every trajectory and every trajectory changes
branch; explicit time matters (a reference with a wrong stage time, or started at t = 0, is 1e4 tolerances away); and the
tolerances are what derive_zoo_tol measures."""
import numpy as np
import pytest

import _hess_ref as hr
import _zoo_ref as zr
from _lyap_ref import complex_jvp
from _tlm_ref import complex_step, row_error, tlm_rk4

TIMED = [n for n in zr.NAMES if zr.model(n).timed]
KINKED = [n for n in zr.NAMES if zr.model(n).kinked]


def test_the_zoo_is_what_the_tests_assume():
    assert TIMED == ["kinked_small", "kinked_stencil", "timed_mix9", "timed_mix0", "l96_damped20", "l96_damped67"]
    assert KINKED == ["kinked_small", "kinked_stencil"]
    m9, m0 = zr.model("timed_mix9"), zr.model("timed_mix0")
    assert m9.nstim == 1 and 4 in m9.kinds and set(m9.kinds) | set(m0.kinds) == {0, 1, 2, 3, 4}
    assert sorted(zr.TOL) == sorted(zr.NAMES)


@pytest.mark.parametrize("name", zr.NAMES)
def test_bindings_agree(name):
    """f at random points (the kinked models' at least 1e-3 from every threshold): NumPy, complex-safe NumPy on real
    input and torch to 1e-14 of the largest entry; complex-safe in longdouble; the torch jvp against the complex-step jvp
    along state and parameter directions to 1e-12; the batched complex-step jvp against _lyap_ref.complex_jvp"""
    import torch
    m = zr.model(name)
    n = 6
    t, x, p, st, _ = zr.safe_points(name, n, 31)
    tt = np.full(n, t)
    pin = lambda a, b: (a, b) if m.nstim else a
    f_np = np.asarray(m.numpy(tt, x, pin(p, st)), dtype=np.float64)
    f_cs = np.array([m.row(t, x[r], p, None if st is None else st[r:r + 1]) for r in range(n)])
    f_ld = np.array([m.row(np.longdouble(t), x[r].astype(np.longdouble), p.astype(np.longdouble),
                           None if st is None else st[r:r + 1].astype(np.longdouble)) for r in range(n)])
    f_to = m.torch(torch.tensor(tt), torch.tensor(x), pin(torch.tensor(p), None if st is None else torch.tensor(st))).numpy()
    scale = np.abs(f_np).max()
    assert f_np.shape == f_cs.shape == f_to.shape == (n, m.D) and f_ld.dtype == np.longdouble and scale > 0.1
    e_cs, e_to, e_ld = np.abs(f_cs - f_np).max() / scale, np.abs(f_to - f_np).max() / scale, float(np.abs(f_ld - f_np).max()) / scale
    rng = np.random.RandomState(32)
    full = m.jvp(range(m.NP))
    e_j = e_b = 0.0
    for r in range(n):
        sr = None if st is None else st[r:r + 1]
        vx, vp = rng.randn(3, m.D), rng.randn(3, m.NP)
        got = full(t, x[r], p, sr, vx, vp)
        want = np.array([m.torch_jvp(t, x[r], p, sr, vx[c], vp[c]) for c in range(3)])
        e_j = max(e_j, np.abs(got - want).max() / np.abs(want).max())
        one_by_one = complex_jvp(m.row)(t, x[r], p, sr, vx, None)
        e_b = max(e_b, np.abs(m.jvp([])(t, x[r], p, sr, vx, None) - one_by_one).max() / np.abs(one_by_one).max())
    print("%s: f complex-safe %.1e torch %.1e longdouble %.1e; jvp torch vs complex step %.1e; batched vs one by one %.1e"
          % (name, e_cs, e_to, e_ld, e_j, e_b))
    assert e_cs <= 1e-14 and e_to <= 1e-14 and e_ld <= 1e-14
    assert e_j <= 1e-12 and e_b <= 1e-14


@pytest.mark.parametrize("name", ["kinked_small", "timed_mix9", "l96_damped20"])
def test_tangent_reference_agrees_with_the_complex_step_of_rk4(name):
    """as _tlm_ref.self_check, for zoo models: tlm_rk4 driven by the complex-safe jvp against the complex-step derivative of
    _predict_ref.rk4 itself, a state direction, a parameter direction and a mixed one, 10 steps from t0 = 3"""
    m, c = zr.model(name), zr.traj_case(name)
    D, Pidx = m.D, c["Pidx"]
    V = np.vstack([np.eye(D + len(Pidx))[1], np.eye(D + len(Pidx))[D], np.random.RandomState(5).randn(D + len(Pidx))])
    stim = None if c["stim"] is None else c["stim"][:11]
    for substeps, every in zr.PAIRS_TLM:
        n_steps = 9 if every == 3 else 10
        _, dX = tlm_rk4(m.row, m.jvp(Pidx), c["x0"][1], c["P"][1], V, n_steps, c["dt"], t0=c["t0"], substeps=substeps, every=every,
                        stim=stim)
        for k in range(len(V)):
            vp = np.zeros(m.NP)
            vp[Pidx] = V[k, D:]
            cs = complex_step(m.row, c["x0"][1], c["P"][1], V[k, :D], vp, n_steps, c["dt"], t0=c["t0"], substeps=substeps, every=every,
                              stim=stim)
            assert row_error(dX[k], cs) <= 1e-13, (name, substeps, k)


@pytest.mark.parametrize("name", zr.NAMES)
def test_nominal_of_the_tangent_reference_is_rk4(name):
    for s, e in zr.PAIRS_TLM:
        assert np.array_equal(zr.tangent_reference(name, s, e)[0], zr.predict_reference(name, s, e)[0])


@pytest.mark.parametrize("name", KINKED)
def test_kinked_trajectories_keep_their_margin_and_change_branch(name):
    """over every stage evaluation of every trajectory, at every (substeps, every | qr_every) the device tests run"""
    for s, e in zr.PAIRS_TLM + zr.PAIRS_LYAP[1:]:
        _, kinks = zr.predict_reference(name, s, e)
        print("%s substeps=%d: smallest |switching argument - threshold| = %.2e; branch patterns per trajectory %s"
              % (name, s, kinks.margin, [len(q) for q in kinks.patterns]))
        assert kinks.margin >= zr.MARGIN
        assert all(kinks.crossed())


def _far(a, b, tol):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max()) > 1e4 * tol


@pytest.mark.parametrize("name", TIMED)
def test_explicit_time_matters_to_the_references(name):
    """a reference whose midpoint stages run at the step's start time, and one started at t = 0, differ from the true one by
    more than 1e4 tolerances in every quantity the device tests compare -- so a device that made either slip cannot pass"""
    tol = zr.TOL[name]
    for wrong in ("midpoint", "t0"):
        for s, e in zr.PAIRS_TLM:
            good, bad = zr.predict_reference(name, s, e)[0], zr.predict_reference(name, s, e, wrong)[0]
            assert _far(good, bad, tol["x"]), (wrong, s)
            assert not _far(good, good.copy(), tol["x"])
            dg, db = zr.tangent_reference(name, s, e)[1], zr.tangent_reference(name, s, e, wrong)[1]
            err = row_error(db, dg)
            print("%s %s substeps=%d: states %.2e (1e4 tol = %.1e)  tangents per row %.2e (1e4 tol = %.1e)"
                  % (name, wrong, s, np.abs(good - bad).max(), 1e4 * tol["x"], err, 1e4 * tol["tlm"]))
            assert err > 1e4 * tol["tlm"], (wrong, s)
        for K, s, q, g in zr.lyap_cases(name)[-1:]:
            a, b = zr.lyap_reference(name, K, s, q, g), zr.lyap_reference(name, K, s, q, g, wrong)
            assert zr.lyap_error(a, b) > 1e4 * tol["lyap"], (wrong, K)


@pytest.mark.parametrize("disc", ["trapezoid", "SimpsonHermite"])
@pytest.mark.parametrize("name", TIMED)
def test_t_model_matters_to_the_hessian_reference(name, disc):
    c, c0 = zr.hvp_case(name, disc), zr.hvp_case(name, disc, 0.0)
    assert c["t_model"][0] == zr.T_HVP and c0["t_model"][0] == 0.0 and np.array_equal(c["X"], c0["X"])
    for key in ("want", "want_gn"):
        scale = np.abs(c[key]).max(axis=-1)
        diff = np.abs(c[key] - c0[key]).max(axis=-1)
        assert np.all(diff > 1e4 * hr.REL * scale), (key, float((diff / scale).min()))
    if zr.model(name).kinked:
        assert c["margin"] >= zr.MARGIN_POINT


@pytest.mark.parametrize("name", zr.NAMES)
def test_tolerances_are_the_derived_ones(name):
    """derive_zoo_tol runs, and TOL[name] is 250 x what it measures, rounded up to two digits (10 % either way for another
    libm's longdouble functions)"""
    got = zr.derive_zoo_tol(name)
    for k, v in got.items():
        if v is None:
            assert zr.TOL[name][k] is None
        else:
            assert 0.9 * 250.0 * v <= zr.TOL[name][k] <= 1.1 * 250.0 * v * 1.05, (k, v)
