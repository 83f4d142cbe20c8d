"""GPU: the forecast kernel k_predict (csrc/va_predict.h) through va_predict -- the built-in Lorenz-96 and generated
modules against the RK4 written in NumPy (tests/_predict_ref.py, where the tolerance is derived), the refusals, the
handle left alone, and va_ode.Annealer.predict / prediction_error end to end."""
import numpy as np
import pytest

from _predict_ref import DT, K_TRUE, STEPS, TOL, l96, l96_reference, rk4
from _util import load_npz_cases
from models.nakl import nakl
from varanneal_amd import _capi, codegen, twin, va_ode

pytestmark = pytest.mark.gpu


def _l96_user(t, x, k):
    return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - x + k


def _handle(D, rhs="lorenz96", P=None, N=5, **kw):
    """a small problem of the model: the forecast takes the model, D, NP, dt_model, device and stream from it"""
    Lidx = list(range(0, D, 2))
    P = np.array([[K_TRUE]]) if P is None else P
    return _capi.Problem(1, D, N, np.zeros((N, len(Lidx))), Lidx, kw.pop("dt", DT), 4.0, 1e-2, P, [0], rhs=rhs, **kw)


@pytest.mark.parametrize("D", [5, 20, 64, 67, 200])
@pytest.mark.parametrize("substeps,every", [(1, 1), (2, 3)])
def test_lorenz96_matches_numpy_rk4(D, substeps, every):
    """T = 7: not a multiple of RW (12 at D = 5, 3 at D = 20), a part-filled last wave, an odd count; D = 64 fills the
    wave, D = 67 and 200 run a workgroup per trajectory with idle lanes"""
    T = 7
    x0, ref = l96_reference(D, T, substeps, every)
    with _handle(D) as pb:
        got = pb.predict(x0, np.full((T, 1), K_TRUE), STEPS, substeps=substeps, every=every)
    assert got.shape == ref.shape == (T, 14 if every == 3 else STEPS + 1, D)
    assert np.array_equal(got[:, 0], x0)
    err = np.abs(got - ref).max()
    print("D=%d substeps=%d every=%d  max |device - NumPy| = %.3e" % (D, substeps, every, err))
    assert err <= TOL


def test_every_trajectory_has_its_own_parameters():
    ks = [8.17, 7.5, 9.0, 8.0, 6.5, 10.0, 8.6]
    x0, ref = l96_reference(20, 7, ks=ks)
    with _handle(20) as pb:
        got = pb.predict(x0, np.array(ks)[:, None], STEPS)
    for j in range(7):
        assert np.abs(got[j] - ref[j]).max() <= TOL, j
    assert np.abs(ref[1] - ref[0]).max() > 1e-2


def _nakl_row(t, x, p, st):
    return nakl(t, x[None, :], (p, st[0]))[0]


def test_generated_module_with_stimulus():
    """NaKL (D = 4: 16 trajectories to a wave), 18 explicit parameters per trajectory, a stimulus that is a smooth
    non-linear function of time: the stage times fall between its samples"""
    c = load_npz_cases("nakl.npz")["g5_nakl_trapezoid_rf1e+00"]
    D, N, NP, T = 4, int(c["N_model"]), 18, 7
    dt = float(c["dt_model"])
    path = c["XP"][:N * D].reshape(N, D)
    x0 = path[::40][:T].copy()
    P = np.tile(c["XP"][N * D:], (T, 1))
    P[:, :3] *= (1.0 + 0.01 * np.arange(T))[:, None]                 # conductances differ from trajectory to trajectory
    t0 = 3.0
    tt = dt * np.arange(STEPS + 1)
    stim = (10.0 + 25.0 * np.sin(4.0 * tt) ** 2 + 8.0 * tt ** 2)[:, None]
    m = codegen.module_for(nakl, D, NP, nstim=1, stim_ndim=1)
    Nh = 5
    with _capi.Problem(1, D, Nh, np.zeros((Nh, 1)), [0], dt, 1.0, 1.0, P[:1], list(range(NP)), rhs=_capi.load_rhs_module(m["so"]),
                       t_model=dt * np.arange(Nh), stim=np.zeros(Nh)) as pb:
        for substeps, every in ((1, 1), (2, 3)):
            got = pb.predict(x0, P, STEPS, t0=t0, substeps=substeps, every=every, stim=stim)
            ref = np.array([rk4(_nakl_row, x0[j], P[j], STEPS, dt, t0=t0, substeps=substeps, every=every, stim=stim)
                            for j in range(T)])
            assert got.shape == ref.shape and np.array_equal(got[:, 0], x0)
            scale = np.abs(ref).max()
            err = np.abs(got - ref).max()
            print("NaKL substeps=%d every=%d  max |device - NumPy| = %.3e  (largest state %.3g)" % (substeps, every, err, scale))
            assert 10.0 < scale < 200.0 and np.abs(ref[:, -1] - ref[:, 0]).max() > 1e-2
            assert err <= TOL * scale
        with pytest.raises(_capi.VaError, match="stimulus"):
            pb.predict(x0, P, STEPS)
        for bad in (dict(n_steps=0), dict(n_steps=4, substeps=0), dict(n_steps=4, every=0)):
            with pytest.raises(_capi.VaError, match="at least 1"):
                pb.predict(x0, P, stim=stim[:bad["n_steps"] + 1], **bad)
    with _handle(20) as pb:
        with pytest.raises(_capi.VaError, match="no stimulus"):
            pb.predict(np.zeros((1, 20)), np.full((1, 1), K_TRUE), STEPS, stim=stim)


def test_generated_lorenz96_with_a_forcing_per_site():
    """D = 20, NP = 20: the module is built in column-parameter form and still has its flat struct"""
    D, T, N = 20, 7, 61
    rng = np.random.RandomState(11)
    x0, _ = l96_reference(D, T)
    P = K_TRUE + 0.5 * rng.randn(T, D)
    Lidx = list(range(0, D, 2))
    m = codegen.module_for(_l96_user, D, D, colparams=True,
                           col_variant=lambda ne, gh, reach=None: _capi.eval_plan(1, D, N, "trapezoid", ne, gh, reach=reach, Lidx=Lidx))
    assert m["colp"] is not None
    with _capi.Problem(1, D, N, np.zeros((N, len(Lidx))), Lidx, DT, 4.0, 1e-2, P[:1], list(range(D)),
                       rhs=_capi.load_rhs_module(m["so"])) as pb:
        got = pb.predict(x0, P, STEPS)
    ref = np.array([rk4(l96, x0[j], P[j], STEPS, DT) for j in range(T)])
    assert np.abs(got - ref).max() <= TOL


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
            pb.predict(np.zeros((2, D)), np.tile(P, (2, 1)), STEPS)
        A1 = pb.action_grad(XP, 2.0)[0]
    assert np.isfinite(A0[0]) and A1[0] == A0[0]


def test_handle_is_left_alone():
    D, N, B = 20, 41, 3
    t, Y, _, Lidx = twin.make_twin(D, N)
    XP = np.stack([np.append(*twin.initial_guess(N, D, b, Y, Lidx)) for b in range(B)])
    x0, _ = l96_reference(D, 7)
    with _capi.Problem(B, D, N, Y, Lidx, DT, 4.0, 4e-6, XP[:, -1:], [0]) as pb:
        before = pb.action_grad(XP, 30.0)
        pb.predict(x0, np.full((7, 1), K_TRUE), STEPS)
        after = pb.action_grad(XP, 30.0)
        resident = pb.read_eval_outputs()
    for u, v, w in zip(before, after, resident):
        assert np.array_equal(u, v) and np.array_equal(v, w)


def test_annealer_predict_end_to_end():
    D, N, B, nb, n_fc = 20, 41, 2, 3, 20
    t, Y, _, Lidx = twin.make_twin(D, N + n_fc)
    X0 = np.stack([twin.initial_guess(N, D, b)[0] for b in range(B)])
    P0 = np.stack([twin.initial_guess(N, D, b)[1] for b in range(B)])
    a = va_ode.Annealer()
    a.set_model(twin.l96, D)
    a.set_data(Y[:N], t=t[:N])
    a.anneal(X0, P0, 2.0, list(range(nb)), 4.0, 1e-2, Lidx, [0], disc="trapezoid", verbose=False,
             opt_args={'gtol': 1e-8, 'ftol': 1e-8, 'maxfun': 2000, 'maxiter': 2000})
    out = a.predict(n_fc, every=4)
    mp = a.minpaths
    assert out.shape == (B, nb, 6, D)
    by_hand = a._pb.predict(mp[:, :, (N - 1) * D:N * D].reshape(-1, D), mp[:, :, N * D:].reshape(-1, 1), n_fc,
                            t0=t[N - 1], every=4).reshape(B, nb, 6, D)
    assert np.array_equal(out, by_hand)
    assert np.array_equal(out[:, :, 0], mp[:, :, (N - 1) * D:N * D])
    sel = a.predict(n_fc, beta=[2], seeds=[1], every=4)
    assert sel.shape == (1, 1, 6, D) and np.array_equal(sel[0, 0], out[1, 2])
    Yf = Y[N - 1::4][:6]
    err = a.prediction_error(Yf, every=4)
    assert err.shape == (B, nb) and np.all(np.isfinite(err))
    assert np.array_equal(err, np.sqrt(np.mean((out[..., 1:, Lidx] - Yf[1:]) ** 2, axis=(-2, -1))))
    assert a.prediction_error(Yf, every=4, beta=[0, 2]).shape == (B, 2)
