"""GPU: the forecast spread -- the tangent-linear predictor k_predict_tlm and the reduction k_spread (csrc/va_predict_tlm.h)
through va_predict_tangent: the built-in Lorenz-96 against the tangent-linear RK4 written in NumPy (tests/_tlm_ref.py,
where the tolerance is derived), a generated module with a stimulus against the complex-step derivative of
_predict_ref.rk4, the sums over directions, the refusals, the handle left alone, and va_ode.Annealer.predict_spread end to
end.  T = 7 trajectories, 40 steps."""
import numpy as np
import pytest

from _predict_ref import DT, K_TRUE, STEPS
from _predict_ref import TOL as TOL_X
from _predict_ref import l96
from _tlm_ref import TOL, complex_step, l96_jvp, l96_tlm_reference, ordered_sums, row_error, tlm_rk4
from _util import load_npz_cases
from models.nakl import nakl
from varanneal_amd import _capi, codegen, twin, va_ode

pytestmark = pytest.mark.gpu

T = 7


def _l96_user(t, x, k):
    return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - x + k


def _handle(D, N=5):
    Lidx = list(range(0, D, 2))
    return _capi.Problem(1, D, N, np.zeros((N, len(Lidx))), Lidx, DT, 4.0, 1e-2, np.array([[K_TRUE]]), [0])


def _same(a, b):
    return sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("D", [5, 20, 64, 67])
@pytest.mark.parametrize("substeps,every", [(1, 1), (2, 3)])
def test_lorenz96_matches_numpy_tlm(D, substeps, every):
    """nvec = D + 1, an identity on the states plus the forcing.  D = 5: the nominal and its 6 directions in 35 lanes of
    one wave; D = 20: three slots to a wave, 11 chunks per trajectory, the last with one direction (21 is no multiple of
    2); D = 64: workgroups of 256 threads x 4 elements, 13 directions each; D = 67: 14 directions each, idle lanes and, in
    the last chunk, idle slots.  With it: row 0, the nominal against predict(), var / cov against the sums of dX formed in
    NumPy in the same order, symmetry, and the same bits on a second call."""
    x0, V0, ref_x, ref_dx = l96_tlm_reference(D, T, substeps, every)
    p = np.full((T, 1), K_TRUE)
    with _handle(D) as pb:
        r = pb.predict_tangent(x0, p, V0, STEPS, substeps=substeps, every=every, want=("dx", "var", "cov"))
        again = pb.predict_tangent(x0, p, V0, STEPS, substeps=substeps, every=every, want=("dx", "var", "cov"))
        plain = pb.predict(x0, p, STEPS, substeps=substeps, every=every)
        only_var = pb.predict_tangent(x0, p, V0, STEPS, substeps=substeps, every=every, want=("var",))
    n_out = 14 if every == 3 else STEPS + 1
    assert r["out"].shape == (T, n_out, D) and r["dx"].shape == ref_dx.shape == (T, D + 1, n_out, D)
    assert np.array_equal(r["out"][:, 0], x0) and np.array_equal(r["dx"][:, :, 0], V0[:, :, :D])
    ex, ed, epl = np.abs(r["out"] - ref_x).max(), row_error(r["dx"], ref_dx), np.abs(r["out"] - plain).max()
    print("D=%d substeps=%d every=%d  nominal |device - NumPy| = %.3e, |device - predict()| = %.3e, tangents relative per row = %.3e"
          % (D, substeps, every, ex, epl, ed))
    assert ex <= TOL_X and epl <= TOL_X
    assert ed <= TOL
    var, cov = ordered_sums(r["dx"])
    assert np.array_equal(r["var"], var) and np.array_equal(r["cov"], cov)
    assert np.array_equal(r["cov"], r["cov"].transpose(0, 1, 3, 2))
    assert _same(r, again)
    assert sorted(only_var) == ["out", "var"] and np.array_equal(only_var["var"], r["var"]) and np.array_equal(only_var["out"], r["out"])


def test_own_forcings_and_a_part_filled_chunk():
    """D = 20, five mixed directions (chunks of 2, 2 and 1) and a forcing of its own per trajectory"""
    ks = [8.17, 7.5, 9.0, 8.0, 6.5, 10.0, 8.6]
    V = np.random.RandomState(9).randn(5, 21)
    x0, V0, ref_x, ref_dx = l96_tlm_reference(20, T, ks=ks, V=V)
    with _handle(20) as pb:
        r = pb.predict_tangent(x0, np.array(ks)[:, None], V0, STEPS)
    assert sorted(r) == ["dx", "out", "var"]
    for j in range(T):
        assert np.abs(r["out"][j] - ref_x[j]).max() <= TOL_X and row_error(r["dx"][j], ref_dx[j]) <= TOL, j
    assert row_error(ref_dx[1], ref_dx[0]) > 1e-2
    # every trajectory its own directions as well: trajectory j takes direction (c + j) mod 5 as its c-th
    V0r = np.array([np.roll(V, -j, axis=0) for j in range(T)])
    with _handle(20) as pb:
        rr = pb.predict_tangent(x0, np.array(ks)[:, None], V0r, STEPS, want=("dx",))
    for j in range(T):
        assert np.array_equal(rr["dx"][j], np.roll(r["dx"][j], -j, axis=0)), j


def _nakl_row(t, x, p, st):
    return nakl(t, x[None, :], (p, st[0]))[0]


PIDX_NAKL = [6, 0, 3, 17]            # Vtm, gNa, ENa, t2n: not in order, so the scatter through Pidx shows


def _nakl_case():
    """the trajectories, parameters and stimulus of test_gpu_predict.py::test_generated_module_with_stimulus, and six
    directions [V, m, h, n | Vtm, gNa, ENa, t2n]: the membrane voltage, a gate, three parameters one by one, and a mixed one"""
    c = load_npz_cases("nakl.npz")["g5_nakl_trapezoid_rf1e+00"]
    D, N, NP = 4, int(c["N_model"]), 18
    dt = float(c["dt_model"])
    x0 = c["XP"][:N * D].reshape(N, D)[::40][:T].copy()
    P = np.tile(c["XP"][N * D:], (T, 1))
    P[:, :3] *= (1.0 + 0.01 * np.arange(T))[:, None]
    tt = dt * np.arange(STEPS + 1)
    stim = (10.0 + 25.0 * np.sin(4.0 * tt) ** 2 + 8.0 * tt ** 2)[:, None]
    V = np.zeros((6, D + len(PIDX_NAKL)))
    V[0, 0] = V[1, 2] = V[2, 4] = V[3, 5] = V[4, 6] = 1.0
    V[5] = np.random.RandomState(4).randn(8)
    return dict(D=D, NP=NP, dt=dt, t0=3.0, x0=x0, P=P, stim=stim, V=V)


def _nakl_reference(k, substeps, every, dtype=np.float64):
    ref = np.empty((T, len(k["V"]), STEPS // every + 1, k["D"]), dtype=dtype)
    for j in range(T):
        for c, v in enumerate(k["V"]):
            vp = np.zeros(k["NP"])
            vp[PIDX_NAKL] = v[k["D"]:]
            ref[j, c] = complex_step(_nakl_row, k["x0"][j], k["P"][j], v[:k["D"]], vp, STEPS, k["dt"], t0=k["t0"], substeps=substeps,
                                     every=every, stim=k["stim"], dtype=dtype)
    return ref


NAKL_TOL = 1.9e-11


def derive_nakl_tol():
    """NAKL_TOL as _tlm_ref.TOL is derived, for this model and these inputs: the reference in float64 against the same
    complex-step derivative carried in longdouble, relative to the largest entry of each row (V, m, h, n of one
    trajectory, direction and time; the voltage's tangent sets the scale), times the same 250-fold margin.  Measured
    7.5e-14 at (substeps, every) = (1, 1) and 2.0e-14 at (2, 3): 250 x 7.5e-14 = 1.9e-11."""
    k = _nakl_case()
    worst = 0.0
    for substeps, every in ((1, 1), (2, 3)):
        e = row_error(np.asarray(_nakl_reference(k, substeps, every), dtype=np.longdouble), _nakl_reference(k, substeps, every, np.longdouble))
        print("NaKL substeps=%d every=%d: float64 vs longdouble complex step, relative per row %.2e" % (substeps, every, e))
        worst = max(worst, e)
    return worst


def test_generated_module_with_stimulus_and_parameter_directions():
    """NaKL, D = 4, 18 parameters of which four are estimated, a stimulus that moves between its samples: the nominal and
    the six directions of a trajectory take 28 lanes, two trajectories to a wave.  Reference: the complex-step derivative
    of _predict_ref.rk4 through the NumPy model (exact to rounding); bound: NAKL_TOL relative per row (derive_nakl_tol)."""
    k = _nakl_case()
    D, NP, dt = k["D"], k["NP"], k["dt"]
    m = codegen.module_for(nakl, D, NP, nstim=1, stim_ndim=1)
    Nh = 5
    V0 = np.ascontiguousarray(np.broadcast_to(k["V"], (T,) + k["V"].shape))
    with _capi.Problem(1, D, Nh, np.zeros((Nh, 1)), [0], dt, 1.0, 1.0, k["P"][:1], PIDX_NAKL, rhs=_capi.load_rhs_module(m["so"]),
                       t_model=dt * np.arange(Nh), stim=np.zeros(Nh)) as pb:
        for substeps, every in ((1, 1), (2, 3)):
            r = pb.predict_tangent(k["x0"], k["P"], V0, STEPS, t0=k["t0"], substeps=substeps, every=every, stim=k["stim"])
            plain = pb.predict(k["x0"], k["P"], STEPS, t0=k["t0"], substeps=substeps, every=every, stim=k["stim"])
            ref = _nakl_reference(k, substeps, every)
            assert r["dx"].shape == ref.shape and np.array_equal(r["dx"][:, :, 0], V0[:, :, :D])
            err = row_error(r["dx"], ref)
            scale = np.abs(plain).max()
            print("NaKL substeps=%d every=%d  tangents relative per row = %.3e (largest tangent entry %.3g), |nominal - predict()| = %.3e"
                  % (substeps, every, err, np.abs(ref).max(), np.abs(r["out"] - plain).max()))
            assert err <= NAKL_TOL
            assert np.abs(r["out"] - plain).max() <= TOL_X * scale
            assert np.abs(ref[:, 2:5, -1]).max(axis=-1).min() > 1e-6         # (every parameter direction moves the states)
            assert np.array_equal(r["var"], ordered_sums(r["dx"])[0])
        with pytest.raises(_capi.VaError, match="stimulus"):
            pb.predict_tangent(k["x0"], k["P"], V0, STEPS)


def test_refusals():
    rng = np.random.RandomState(2)
    x0, V0, _, _ = l96_tlm_reference(5, T)
    dp = lambda a: a.ctypes.data_as(_capi.c_dp)
    with _handle(5) as pb:
        with pytest.raises(ValueError, match="nvec"):
            pb.predict_tangent(x0, np.full((T, 1), K_TRUE), np.zeros((T, 0, 6)), STEPS)
        out = np.empty((T, STEPS + 1, 5))
        rc = pb._L.va_predict_tangent(pb._h, dp(x0), dp(np.full((T, 1), K_TRUE)), dp(V0), T, 0, 0.0, STEPS, 1, 1, None, dp(out), None,
                                      None, None)
        assert rc == -1 and b"nvec" in pb._L.va_last_error()
        for bad in (dict(n_steps=0), dict(n_steps=4, substeps=0), dict(n_steps=4, every=0)):
            with pytest.raises(_capi.VaError, match="at least 1"):
                pb.predict_tangent(x0, np.full((T, 1), K_TRUE), V0, **bad)
        with pytest.raises(_capi.VaError, match="no stimulus"):
            pb.predict_tangent(x0, np.full((T, 1), K_TRUE), V0, STEPS, stim=np.zeros((STEPS + 1, 1)))
        with pytest.raises(ValueError, match="want"):
            pb.predict_tangent(x0, np.full((T, 1), K_TRUE), V0, STEPS, want=("dX",))
    # a module whose dense linear part was split off
    N = 7
    lin = codegen.module_for(twin.dense_coupling_model(20, 1)[0], 20, 2)
    assert lin["lin"] is not None
    with _capi.Problem(1, 20, N, rng.randn(N, 2), [0, 2], DT, 1.0, 1.0, np.ones((1, 2)), [0], disc="trapezoid",
                       rhs=_capi.load_rhs_module(lin["so"])) as pb:
        with pytest.raises(NotImplementedError, match="linear"):
            pb.predict_tangent(rng.randn(1, 20), np.ones((1, 2)), rng.randn(1, 1, 21), 4)
    # the network action
    s = twin.nnet_structure(20, 10, 10, 10)
    din, dout, _ = twin.make_nnet_twin(s, 2)
    Xn, Pn, Pidx = twin.nnet_initial_guess(s, 2, 0)
    with _capi.NnetProblem(1, s, din, dout, [np.arange(10), np.arange(10)], 4.0e4, 0.0038, Pn[None, :], Pidx) as nb:
        rc = nb._L.va_predict_tangent(nb._h, dp(Xn), dp(Xn), dp(Xn), 1, 1, 0.0, 4, 1, 1, None, dp(Xn), None, None, None)
        assert rc == -4 and b"network" in nb._L.va_last_error()
        with pytest.raises(NotImplementedError, match="network"):          # the binding's own guard
            nb.predict_tangent(Xn[None, :], Xn[None, :], Xn[None, None, :], 4)


def test_model_past_128_parameters_is_refused():
    D, N = 200, 65
    rng = np.random.RandomState(12)
    Lidx = list(range(0, D, 2))
    P = K_TRUE + 0.1 * rng.randn(1, D)
    m = codegen.module_for(_l96_user, D, D, colparams=True,
                           col_variant=lambda ne, gh, reach=None: _capi.eval_plan(1, D, N, "trapezoid", ne, gh, reach=reach, Lidx=Lidx))
    XP = np.append(3.0 * rng.randn(N * D), P[0])[None, :]
    with _capi.Problem(1, D, N, rng.randn(N, len(Lidx)), Lidx, DT, 4.0, 1e-2, P, list(range(D)),
                       rhs=_capi.load_rhs_module(m["so"])) as pb:
        A0 = pb.action_grad(XP, 2.0)[0]
        with pytest.raises(NotImplementedError, match="flat form"):
            pb.predict_tangent(np.zeros((2, D)), np.tile(P, (2, 1)), np.ones((2, 1, 2 * D)), STEPS)
        A1 = pb.action_grad(XP, 2.0)[0]
    assert np.isfinite(A0[0]) and A1[0] == A0[0]


def test_handle_is_left_alone():
    D, N, B = 20, 41, 3
    t, Y, _, Lidx = twin.make_twin(D, N)
    XP = np.stack([np.append(*twin.initial_guess(N, D, b, Y, Lidx)) for b in range(B)])
    x0, V0, _, _ = l96_tlm_reference(D, T)
    with _capi.Problem(B, D, N, Y, Lidx, DT, 4.0, 4e-6, XP[:, -1:], [0]) as pb:
        before = pb.action_grad(XP, 30.0)
        pb.predict_tangent(x0, np.full((T, 1), K_TRUE), V0, STEPS, want=("dx", "var", "cov"))
        after = pb.action_grad(XP, 30.0)
        resident = pb.read_eval_outputs()
    for u, v, w in zip(before, after, resident):
        assert np.array_equal(u, v) and np.array_equal(v, w)


def test_annealer_predict_spread_end_to_end():
    """the D = 5, N = 9 anneal of test_gpu_selinv.py::test_batch_selection_and_each_rungs_own_rf (two seeds, two rungs),
    Gauss-Newton so that every point is positive definite.  std^2 against diag(M Sigma_0 M^T), M = d forecast / d(x_{N-1}, k)
    from the NumPy tangent-linear RK4 and Sigma_0 from laplace(full=True).  The bound: every tangent row of the device is
    within TOL max|row| of the reference's (M L)_c (tests/_tlm_ref.py), so a variance sum_c d_c,i^2 is within
    2 TOL sum_c max|d_c|^2 =: 2 TOL S, and so is a covariance entry; the host Cholesky factor reproduces Sigma_0 to (n + 1) eps on
    the same scale, and the reference's own triple product rounds at 2 n eps (|M| |Sigma_0| |M|^T)_ij."""
    D, N, B, n_fc, every = 5, 9, 2, STEPS, 4
    rng = np.random.RandomState(6)
    Lidx, RM, RF0, alpha = [0, 2, 3], 4.0, 0.5, 2.0
    Y = 2.0 * rng.randn(N, len(Lidx))
    a = va_ode.Annealer()
    a.set_model(_l96_user, D)
    a.set_data(Y, t=DT * np.arange(N))
    a.anneal(rng.randn(B, N, D), np.array([[8.0], [8.5]]), alpha, [0, 1], RM, RF0, Lidx, [0], disc="trapezoid", verbose=False,
             opt_args={'gtol': 1e-10, 'ftol': 1e-14})
    r = a.predict_spread(n_fc, every=every, gauss_newton=True, full=True)
    lap = a.laplace(gauss_newton=True, full=True)
    mean = a.predict(n_fc, every=every)
    n_out = n_fc // every + 1
    assert r["mean"].shape == r["std"].shape == (B, 2, n_out, D) and r["cov"].shape == (B, 2, n_out, D, D)
    assert np.array_equal(r["status"], lap["status"]) and not r["status"].any()
    assert np.array_equal(r["mean"], mean)
    eps, n = np.finfo(float).eps, D + 1
    mp = a.minpaths
    worst = 0.0
    for b in range(B):
        for k in range(2):
            S0 = np.empty((n, n))
            S0[:D, :D], S0[D:, :D] = lap["state_cov"][b, k, N - 1], lap["state_param_cov"][b, k, :, N - 1]
            S0[:D, D:], S0[D:, D:] = S0[D:, :D].T, lap["param_cov"][b, k]
            _, M = tlm_rk4(l96, l96_jvp, mp[b, k, (N - 1) * D:N * D], mp[b, k, N * D], np.eye(n), n_fc, DT,
                           t0=float(a.t_model[-1]), every=every)                       # M[c, row, i] = d x_row,i / d (x, k)_c
            ref = np.einsum("cri,cd,drj->rij", M, S0, M)
            ML = np.einsum("cri,cd->dri", M, np.linalg.cholesky(S0))
            bound = ((2.0 * TOL + (n + 1) * eps) * (np.abs(ML).max(axis=-1) ** 2).sum(axis=0))[:, None, None] \
                + 2 * n * eps * np.einsum("cri,cd,drj->rij", np.abs(M), np.abs(S0), np.abs(M))
            err = np.abs(r["std"][b, k] ** 2 - np.einsum("rii->ri", ref)) / np.einsum("rii->ri", bound)
            worst = max(worst, err.max())
            assert np.all(err <= 1.0), (b, k)
            assert np.all(np.abs(r["cov"][b, k] - ref) <= bound), (b, k)
            # row 0 is the last fitted time: laplace's own variance there, up to the factor's and the sum's rounding
            v0 = lap["state_var"][b, k, N - 1]
            assert np.all(np.abs(r["std"][b, k, 0] ** 2 - v0) <= (2 * n + 2) * eps * v0)
    print("std^2 against diag(M Sigma_0 M^T): largest error / bound = %.3f" % worst)
    assert np.all(r["std"][:, :, -1].max(axis=-1) > r["std"][:, :, 0].max(axis=-1))     # (the error bar grows along the forecast)
    sel = a.predict_spread(n_fc, beta=[1], seeds=[1], every=every, gauss_newton=True)
    assert sorted(sel) == ["mean", "status", "std"] and np.array_equal(sel["std"][0, 0], r["std"][1, 1])
    a.close()
