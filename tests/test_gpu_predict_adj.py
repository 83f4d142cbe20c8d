"""GPU: the adjoint predictor k_predict_adj (csrc/va_predict_adj.h) through va_predict_adjoint: the built-in Lorenz-96 against
the adjoint RK4 written in NumPy (tests/_adj_ref.py, where the tolerance is derived), the transpose identity against the
tangent kernel k_predict_tlm, misfit mode, a generated module with a stimulus, the refusals and the handle left alone.
T = 7 trajectories, 40 steps."""
import numpy as np
import pytest

import _adj_ref
from _adj_ref import TOL_ADJ, l96_adj_reference, row_error
from _predict_ref import DT, K_TRUE, STEPS
from _predict_ref import TOL as TOL_X
from _predict_ref import l96
from _tlm_ref import TOL, complex_step
from test_gpu_predict_tlm import NAKL_TOL, PIDX_NAKL, _nakl_case, _nakl_reference
from models.nakl import nakl
from varanneal_amd import _capi, codegen, twin

pytestmark = pytest.mark.gpu

T = 7


def _handle(D, N=5, Lidx=None):
    Lidx = list(range(0, D, 2)) if Lidx is None else Lidx
    return _capi.Problem(1, D, N, np.zeros((N, len(Lidx))), Lidx, DT, 4.0, 1e-2, np.array([[K_TRUE]]), [0])


def _same(a, b):
    return sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("D,ncot", [(5, 1), (20, 5), (64, 3), (67, 3)])
@pytest.mark.parametrize("substeps,every", [(1, 1), (2, 3)])
def test_lorenz96_matches_numpy_adjoint(D, ncot, substeps, every):
    """D = 5, one set: a wave of six trajectories side by side, the second group with idle slots; D = 20, five sets: chunks
    of 2, 2 and 1; D = 64 and 67, three sets: workgroups of 256 threads, idle lanes and idle slots.  With it: the nominal
    against predict(), row 0's cotangent alone, and the same bits on a second call."""
    x0, G, ref_x, ref_gx, ref_gp = l96_adj_reference(D, T, ncot, substeps, every)
    p = np.full((T, 1), K_TRUE)
    G0 = np.zeros_like(G)
    G0[:, :, 0] = G[:, :, 0]
    with _handle(D) as pb:
        r = pb.predict_adjoint(x0, p, STEPS, G=G, substeps=substeps, every=every)
        again = pb.predict_adjoint(x0, p, STEPS, G=G, substeps=substeps, every=every)
        plain = pb.predict(x0, p, STEPS, substeps=substeps, every=every)
        r0 = pb.predict_adjoint(x0, p, STEPS, G=G0, substeps=substeps, every=every)
    assert sorted(r) == ["gp", "gx0", "out"]
    assert r["out"].shape == ref_x.shape and r["gx0"].shape == (T, ncot, D) and r["gp"].shape == (T, ncot, 1)
    ex, epl, eg, ep = np.abs(r["out"] - ref_x).max(), np.abs(r["out"] - plain).max(), row_error(r["gx0"], ref_gx), row_error(r["gp"], ref_gp)
    print("D=%d ncot=%d substeps=%d every=%d  nominal |device - NumPy| = %.3e, |device - predict()| = %.3e, gx0 relative per row = %.3e, "
          "gp = %.3e (bound %.1e)" % (D, ncot, substeps, every, ex, epl, eg, ep, TOL_ADJ))
    assert np.array_equal(r["out"][:, 0], x0)
    assert ex <= TOL_X and epl <= TOL_X
    assert eg <= TOL_ADJ and ep <= TOL_ADJ
    assert np.array_equal(r0["gx0"], G[:, :, 0]) and np.array_equal(r0["gp"], np.zeros((T, ncot, 1)))
    assert _same(r, again)


@pytest.mark.parametrize("D", [5, 20])
def test_transpose_of_the_tangent_kernel(D):
    """dX from predict_tangent along the D + 1 identity directions, random G: <G, dX_c> = gx0[c] (c < D) or gp (c = D),
    within (TOL + TOL_ADJ) |G| |dX_c|"""
    substeps, every = 2, 3
    x0, G, _, _, _ = l96_adj_reference(D, T, 1, substeps, every)
    p = np.full((T, 1), K_TRUE)
    V0 = np.ascontiguousarray(np.broadcast_to(np.eye(D + 1), (T, D + 1, D + 1)))
    with _handle(D) as pb:
        dX = pb.predict_tangent(x0, p, V0, STEPS, substeps=substeps, every=every, want=("dx",))["dx"]
        r = pb.predict_adjoint(x0, p, STEPS, G=G, substeps=substeps, every=every)
    worst = 0.0
    for j in range(T):
        got = np.append(r["gx0"][j, 0], r["gp"][j, 0])
        for c in range(D + 1):
            lhs = (G[j, 0] * dX[j, c]).sum()
            worst = max(worst, abs(lhs - got[c]) / (np.linalg.norm(G[j, 0]) * np.linalg.norm(dX[j, c])))
    print("D=%d: <G, dX_c> against gx0 / gp, largest defect relative to |G| |dX_c| = %.3e (bound %.1e)" % (D, worst, TOL + TOL_ADJ))
    assert worst <= TOL + TOL_ADJ


@pytest.mark.parametrize("shared", [False, True])
def test_misfit_mode(shared):
    """cost and gradients against cotangent mode fed 2 w (out - Y), three gradient components against the complex step of
    the NumPy cost; observed columns in an order that is not ascending (the device keeps them sorted)"""
    D, substeps, every = 20, 2, 3
    x0, _, ref_x, _, _ = l96_adj_reference(D, T, 1, substeps, every)
    Lidx = [3, 0, 6, 9, 18, 12, 15]
    rng = np.random.RandomState(4)
    w = 0.5 + rng.rand(len(Lidx))
    Y = ref_x[:, :, Lidx] + 0.3 * rng.randn(T, ref_x.shape[1], len(Lidx))
    if shared:
        Y = np.ascontiguousarray(Y[2])
    p = np.full((T, 1), K_TRUE)
    with _handle(D, Lidx=Lidx) as pb:
        r = pb.predict_adjoint(x0, p, STEPS, Y=Y, weights=w, substeps=substeps, every=every)
        again = pb.predict_adjoint(x0, p, STEPS, Y=Y, weights=w, substeps=substeps, every=every)
        G = np.zeros((T, 1) + ref_x.shape[1:])
        G[:, 0][:, :, Lidx] = 2.0 * w * (r["out"][:, :, Lidx] - Y)
        rc = pb.predict_adjoint(x0, p, STEPS, G=G, substeps=substeps, every=every)
    assert sorted(r) == ["cost", "gp", "gx0", "out"] and r["cost"].shape == (T,) and _same(r, again)
    cost = (w * (r["out"][:, :, Lidx] - Y) ** 2).sum(axis=(1, 2))
    ec = np.abs(r["cost"] - cost).max() / cost.max()
    eg, ep = row_error(r["gx0"], rc["gx0"]), row_error(r["gp"], rc["gp"])
    print("misfit mode against cotangent mode (shared Y: %s): cost %.3e, gx0 %.3e, gp %.3e relative" % (shared, ec, eg, ep))
    assert ec <= TOL_ADJ and eg <= TOL_ADJ and ep <= TOL_ADJ
    assert np.array_equal(r["out"], rc["out"])
    # d cost / d x0_i and d cost / d k by the complex step of the NumPy cost (exact to rounding)
    j = 4
    Yj = Y if shared else Y[j]
    for comp in (0, 7, D):
        vx, vp = np.eye(D + 1)[comp, :D], float(comp == D)
        d_out = complex_step(l96, x0[j], K_TRUE, vx, vp, STEPS, DT, substeps=substeps, every=every)
        ref = (2.0 * w * (ref_x[j][:, Lidx] - Yj) * d_out[:, Lidx]).sum()
        got = r["gp"][j, 0, 0] if comp == D else r["gx0"][j, 0, comp]
        scale = np.abs(r["gx0"][j, 0]).max() if comp < D else abs(ref)
        assert abs(got - ref) <= (TOL + TOL_ADJ) * max(scale, abs(ref)), comp


NAKL_ADJ_TOL = TOL_ADJ


def test_generated_module_with_stimulus_transposes_the_numpy_tangents():
    """NaKL, D = 4, 18 parameters of which four are estimated through PIDX_NAKL (not in order: the gather shows), a stimulus
    that moves between its samples; two cotangent sets per trajectory, so the nominal and its sets take 12 lanes and five
    trajectories share a wave.  <G, dX_c> = <gx0, v_x> + <gp, v_p> with dX_c the complex-step tangents of
    test_gpu_predict_tlm.py.  The bound is what the two references promise, row by row: the tangents are within NAKL_TOL
    max|row| (derived there), so the left side within NAKL_TOL sum_rows |G_row|_1 max|dX_row|; the device's gx0 and gp are
    taken to be within NAKL_ADJ_TOL max|row| as TOL_ADJ is derived for Lorenz-96 in _adj_ref.derive() (there is no NumPy
    adjoint of this model to derive it from: the adjoint applies the transposes of the Jacobians the tangent applies, at the
    same points), so the right side within NAKL_ADJ_TOL (max|gx0| |v_x|_1 + max|gp| |v_p|_1)."""
    k = _nakl_case()
    D, NP, dt = k["D"], k["NP"], k["dt"]
    m = codegen.module_for(nakl, D, NP, nstim=1, stim_ndim=1)
    Nh, ncot = 5, 2
    with _capi.Problem(1, D, Nh, np.zeros((Nh, 1)), [0], dt, 1.0, 1.0, k["P"][:1], PIDX_NAKL, rhs=_capi.load_rhs_module(m["so"]),
                       t_model=dt * np.arange(Nh), stim=np.zeros(Nh)) as pb:
        for substeps, every in ((1, 1), (2, 3)):
            ref = _nakl_reference(k, substeps, every)                      # (T, 6, n_out, D)
            G = np.random.RandomState(21).randn(T, ncot, ref.shape[2], D)
            r = pb.predict_adjoint(k["x0"], k["P"], STEPS, G=G, t0=k["t0"], substeps=substeps, every=every, stim=k["stim"])
            plain = pb.predict(k["x0"], k["P"], STEPS, t0=k["t0"], substeps=substeps, every=every, stim=k["stim"])
            assert np.abs(r["out"] - plain).max() <= TOL_X * np.abs(plain).max()
            assert r["gp"].shape == (T, ncot, len(PIDX_NAKL))
            worst = 0.0
            for j in range(T):
                for g in range(ncot):
                    for c, v in enumerate(k["V"]):
                        lhs = (G[j, g] * ref[j, c]).sum()
                        rhs = np.dot(r["gx0"][j, g], v[:D]) + np.dot(r["gp"][j, g], v[D:])
                        bound = NAKL_TOL * (np.abs(G[j, g]).sum(axis=-1) * np.abs(ref[j, c]).max(axis=-1)).sum() \
                            + NAKL_ADJ_TOL * (np.abs(r["gx0"][j, g]).max() * np.abs(v[:D]).sum() + np.abs(r["gp"][j, g]).max() * np.abs(v[D:]).sum())
                        worst = max(worst, abs(lhs - rhs) / bound)
            print("NaKL substeps=%d every=%d: transpose identity, largest defect / bound = %.3f" % (substeps, every, worst))
            assert worst <= 1.0
            assert np.abs(r["gp"]).max(axis=(0, 1)).min() > 1e-6             # (every estimated parameter takes a gradient)
        with pytest.raises(_capi.VaError, match="stimulus"):
            pb.predict_adjoint(k["x0"], k["P"], STEPS, G=np.zeros((T, 1, STEPS + 1, D)))


def test_refusals():
    rng = np.random.RandomState(2)
    x0, G, _, _, _ = l96_adj_reference(5, T, 1)
    p = np.full((T, 1), K_TRUE)
    dp = lambda a: a.ctypes.data_as(_capi.c_dp)
    with _handle(5) as pb:
        Y, w = np.zeros((STEPS + 1, 3)), np.ones(3)
        with pytest.raises(ValueError, match="exactly one"):
            pb.predict_adjoint(x0, p, STEPS)
        with pytest.raises(ValueError, match="exactly one"):
            pb.predict_adjoint(x0, p, STEPS, G=G, Y=Y, weights=w)
        with pytest.raises(ValueError, match="G must have shape"):
            pb.predict_adjoint(x0, p, STEPS, G=G[:, :, :-1])
        with pytest.raises(ValueError, match="Y must have shape"):
            pb.predict_adjoint(x0, p, STEPS, Y=Y[:, :2], weights=w)
        with pytest.raises(ValueError, match="weights"):
            pb.predict_adjoint(x0, p, STEPS, Y=Y)
        with pytest.raises(ValueError, match="weights must have shape"):
            pb.predict_adjoint(x0, p, STEPS, Y=Y, weights=np.ones(2))
        out, gx0, gp = np.empty((T, STEPS + 1, 5)), np.empty((T, 1, 5)), np.empty((T, 1, 1))
        rc = pb._L.va_predict_adjoint(pb._h, dp(x0), dp(p), None, None, None, 0, T, 1, 0.0, STEPS, 1, 1, None, dp(out), dp(gx0), dp(gp), None)
        assert rc == -1 and b"exactly one" in pb._L.va_last_error()
        rc = pb._L.va_predict_adjoint(pb._h, dp(x0), dp(p), dp(G), None, None, 0, T, 0, 0.0, STEPS, 1, 1, None, dp(out), dp(gx0), dp(gp), None)
        assert rc == -1 and b"ncot" in pb._L.va_last_error()
        for bad in (dict(n_steps=0), dict(n_steps=4, substeps=0)):
            with pytest.raises(_capi.VaError, match="at least 1"):
                pb.predict_adjoint(x0, p, G=np.zeros((T, 1, 1 if bad["n_steps"] == 0 else 5, 5)), **bad)
        with pytest.raises(_capi.VaError, match="no stimulus"):
            pb.predict_adjoint(x0, p, STEPS, G=G, stim=np.zeros((STEPS + 1, 1)))
    N = 7
    lin = codegen.module_for(twin.dense_coupling_model(20, 1)[0], 20, 2)
    assert lin["lin"] is not None
    with _capi.Problem(1, 20, N, rng.randn(N, 2), [0, 2], DT, 1.0, 1.0, np.ones((1, 2)), [0], disc="trapezoid",
                       rhs=_capi.load_rhs_module(lin["so"])) as pb:
        with pytest.raises(NotImplementedError, match="linear"):
            pb.predict_adjoint(rng.randn(1, 20), np.ones((1, 2)), 4, G=rng.randn(1, 1, 5, 20))
    s = twin.nnet_structure(20, 10, 10, 10)
    din, dout, _ = twin.make_nnet_twin(s, 2)
    Xn, Pn, Pidx = twin.nnet_initial_guess(s, 2, 0)
    with _capi.NnetProblem(1, s, din, dout, [np.arange(10), np.arange(10)], 4.0e4, 0.0038, Pn[None, :], Pidx) as nb:
        rc = nb._L.va_predict_adjoint(nb._h, dp(Xn), dp(Xn), dp(Xn), None, None, 0, 1, 1, 0.0, 4, 1, 1, None, dp(Xn), dp(Xn), dp(Xn), None)
        assert rc == -4 and b"network" in nb._L.va_last_error()
        with pytest.raises(NotImplementedError, match="network"):
            nb.predict_adjoint(Xn[None, :], Xn[None, :], 4, G=Xn[None, None, None, :])


def test_handle_is_left_alone():
    D, N, B = 20, 41, 3
    t, Y, _, Lidx = twin.make_twin(D, N)
    XP = np.stack([np.append(*twin.initial_guess(N, D, b, Y, Lidx)) for b in range(B)])
    x0, G, _, _, _ = l96_adj_reference(D, T, 5)
    with _capi.Problem(B, D, N, Y, Lidx, DT, 4.0, 4e-6, XP[:, -1:], [0]) as pb:
        before = pb.action_grad(XP, 30.0)
        pb.predict_adjoint(x0, np.full((T, 1), K_TRUE), STEPS, G=G)
        pb.predict_adjoint(x0[:1], np.full((1, 1), K_TRUE), N - 1, Y=Y, weights=np.ones(len(Lidx)))
        after = pb.action_grad(XP, 30.0)
        resident = pb.read_eval_outputs()
    for u, v, w in zip(before, after, resident):
        assert np.array_equal(u, v) and np.array_equal(v, w)
