"""GPU: Lyapunov spectra -- the kernel k_lyap (csrc/va_lyap.h) through va_lyapunov: the built-in Lorenz-96 against Benettin's
method written in NumPy (tests/_lyap_ref.py, where the tolerance is derived), the log-determinant identity, continuation, a
generated module with an exact answer, the generated NaKL module with its stimulus against the reference driven by a
complex-step Jacobian, the refusals, the handle left alone, a rank-deficient start, and va_ode.Annealer.lyapunov /
sync_exponents end to end.  T = 7 trajectories, 40 steps."""
import numpy as np
import pytest

from _lyap_ref import FORCINGS, TOL, complex_jvp, gain_every_second, l96_lyap_reference, lyap_ref
from _predict_ref import DT, K_TRUE, STEPS, attractor_starts, l96
from _predict_ref import TOL as TOL_X
from _tlm_ref import l96_jvp, tlm_rk4
from _util import load_npz_cases
from models.nakl import nakl
from varanneal_amd import _capi, codegen, twin, va_ode

pytestmark = pytest.mark.gpu

T = 7
KEYS = ("logsum", "x_end", "Q_end", "trace", "status")


def _l96_user(t, x, k):
    return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - x + k


def _handle(D, N=5):
    Lidx = list(range(0, D, 2))
    return _capi.Problem(1, D, N, np.zeros((N, len(Lidx))), Lidx, DT, 4.0, 1e-2, np.array([[K_TRUE]]), [0])


def _same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in KEYS)


@pytest.mark.parametrize("D,K", [(5, 3), (5, 5), (20, 3), (20, 20), (33, 3), (33, 33), (64, 31)])
@pytest.mark.parametrize("substeps,qr_every", [(1, 1), (2, 4)])
@pytest.mark.parametrize("gain", [False, True])
def test_lorenz96_matches_numpy(D, K, substeps, qr_every, gain):
    """a forcing of its own per trajectory.  D = 5: one wave, K = 3 three trajectories to it (seven: the last workgroup holds
    one), K = 5 two; D = 20: K = 3 two waves, K = 20 256 threads x 2 elements; D = 33: K = 33 256 x 5, idle lanes;
    D = 64, K = 31: 256 x 8, the even width whose slots are padded to 65.  And the same bits on a second call."""
    x0, ks, g, ref = l96_lyap_reference(D, T, K, substeps, qr_every, 0, gain)
    with _handle(D) as pb:
        r = pb.lyapunov(x0, ks[:, None], K, STEPS, substeps=substeps, qr_every=qr_every, coupling=g, trace=True)
        again = pb.lyapunov(x0, ks[:, None], K, STEPS, substeps=substeps, qr_every=qr_every, coupling=g, trace=True)
    el, eq = np.abs(r["logsum"] - ref["logsum"]).max(), np.abs(r["Q_end"] - ref["Q_end"]).max()
    ex, et = np.abs(r["x_end"] - ref["x_end"]).max(), np.abs(r["trace"] - ref["trace"]).max()
    eo = np.abs(np.einsum("tki,tli->tkl", r["Q_end"], r["Q_end"]) - np.eye(K)).max()
    print("D=%d K=%d substeps=%d qr_every=%d gain=%s: |device - NumPy| logsum %.3e  Q_end %.3e  x_end %.3e  trace %.3e; |Q Q^T - I| %.3e"
          % (D, K, substeps, qr_every, gain, el, eq, ex, et, eo))
    assert not r["status"].any()
    assert el <= TOL and eq <= TOL and et <= TOL and ex <= TOL_X and eo <= TOL
    assert np.abs(r["trace"].sum(axis=1) - r["logsum"]).max() <= TOL
    assert np.array_equal(r["exponents"], r["logsum"] / (STEPS * DT))
    assert _same(r, again)


def test_skipped_transient():
    x0, ks, _, ref = l96_lyap_reference(20, T, 20, 2, 4, 2, False)
    with _handle(20) as pb:
        r = pb.lyapunov(x0, ks[:, None], 20, STEPS, substeps=2, qr_every=4, n_skip=2, trace=True)
    assert np.abs(r["logsum"] - ref["logsum"]).max() <= TOL and np.abs(r["trace"] - ref["trace"]).max() <= TOL
    assert np.abs(r["trace"][:, 2:].sum(axis=1) - r["logsum"]).max() <= TOL
    assert np.array_equal(r["exponents"], r["logsum"] / (8 * 4 * DT))


@pytest.mark.parametrize("D", [5, 20])
def test_sum_of_the_spectrum_is_the_log_determinant(D):
    """K = D, no gain: sum_j logsum_j = log |det M| of the propagator the tangent-linear reference gives, whatever the QR interval"""
    x0, ks = attractor_starts(D, T), np.array(FORCINGS[:T])
    V = np.hstack([np.eye(D), np.zeros((D, 1))])
    want = np.array([np.linalg.slogdet(tlm_rk4(l96, l96_jvp, x0[i], ks[i], V, STEPS, DT)[1][:, -1, :])[1] for i in range(T)])
    with _handle(D) as pb:
        for qr_every in (1, 4, 8, 40):
            r = pb.lyapunov(x0, ks[:, None], D, STEPS, qr_every=qr_every)
            err = np.abs(r["logsum"].sum(axis=1) - want).max()
            print("D=%d qr_every=%d: |sum logsum - log|det M|| = %.3e" % (D, qr_every, err))
            assert not r["status"].any() and err <= TOL * D


def test_continuation_is_bit_equal():
    D, K = 20, 7
    x0, ks = attractor_starts(D, T), np.array(FORCINGS[:T])[:, None]
    g = np.broadcast_to(gain_every_second(D, 2.0), (T, D))
    kw = dict(substeps=2, qr_every=4, coupling=g, trace=True)
    with _handle(D) as pb:
        one = pb.lyapunov(x0, ks, K, 40, **kw)
        a = pb.lyapunov(x0, ks, K, 20, **kw)
        b = pb.lyapunov(a["x_end"], ks, K, 20, t0=20 * DT, Q0=a["Q_end"], **kw)
    assert np.array_equal(b["x_end"], one["x_end"]) and np.array_equal(b["Q_end"], one["Q_end"])
    assert np.array_equal(np.concatenate([a["trace"], b["trace"]], axis=1), one["trace"])


def _diag4(t, x, p):
    return np.stack([p[i] * x[:, i] for i in range(4)], axis=1)


def test_generated_module_with_an_exact_answer():
    """f_i = a_i x_i: with Q0 = I the tangents never mix, and exponent j is substeps log|R(h a_j)| / dt with R the stability
    polynomial of RK4 and h = dt / substeps"""
    a = np.array([0.5, -1.0, -3.0, 0.2])
    m = codegen.module_for(_diag4, 4, 4, linear=False)
    Nh = 5
    x0 = np.random.RandomState(1).randn(T, 4)
    with _capi.Problem(1, 4, Nh, np.zeros((Nh, 1)), [0], DT, 1.0, 1.0, a[None, :], [0], rhs=_capi.load_rhs_module(m["so"])) as pb:
        for substeps, qr_every in ((1, 1), (2, 4)):
            r = pb.lyapunov(x0, a, 4, STEPS, substeps=substeps, qr_every=qr_every)
            z = DT / substeps * a
            want = substeps * np.log(np.abs(1.0 + z + z ** 2 / 2.0 + z ** 3 / 6.0 + z ** 4 / 24.0)) / DT
            err = np.abs(r["exponents"] - want).max()
            print("diagonal model substeps=%d qr_every=%d: |exponents - exact| = %.3e (exact %s)" % (substeps, qr_every, err, want))
            assert not r["status"].any() and err <= TOL / (40 * DT)
            assert np.abs(np.abs(r["Q_end"]) - np.eye(4)).max() <= TOL


# ---------------------------------------------------------------------------------------------------------------
def _nakl_row(t, x, p, st):
    return nakl(t, x[None, :], (p, st[0]))[0]


def _nakl_case():
    """the trajectories, parameters and stimulus of test_gpu_predict_tlm.py's NaKL case; K = 4, gain on the voltage alone"""
    c = load_npz_cases("nakl.npz")["g5_nakl_trapezoid_rf1e+00"]
    D, N, NP = 4, int(c["N_model"]), 18
    dt = float(c["dt_model"])
    x0 = c["XP"][:N * D].reshape(N, D)[::40][:T].copy()
    P = np.tile(c["XP"][N * D:], (T, 1))
    P[:, :3] *= (1.0 + 0.01 * np.arange(T))[:, None]
    tt = dt * np.arange(STEPS + 1)
    stim = (10.0 + 25.0 * np.sin(4.0 * tt) ** 2 + 8.0 * tt ** 2)[:, None]
    return dict(D=D, NP=NP, dt=dt, t0=3.0, x0=x0, P=P, stim=stim, gain=np.array([2.0, 0.0, 0.0, 0.0]))


def _nakl_reference(k, substeps, qr_every, dtype=np.float64):
    res = [lyap_ref(_nakl_row, complex_jvp(_nakl_row), k["x0"][j], k["P"][j], 4, STEPS, k["dt"], t0=k["t0"], substeps=substeps,
                    qr_every=qr_every, gain=k["gain"], stim=k["stim"], dtype=dtype) for j in range(T)]
    return {key: np.array([r[key] for r in res]) for key in res[0]}


NAKL_TOL = 1.9e-10


def derive_nakl_tol():
    """NAKL_TOL as _lyap_ref.TOL is derived, for this model and these inputs: the reference in float64 against the same
    computation carried in longdouble, largest absolute difference of logsum and of Q_end over both (substeps, qr_every)
    pairs, times the same 250-fold margin.  Measured: logsum 2.4e-14 and Q_end 6.0e-14 at (1, 1), logsum 7.7e-14 and Q_end
    7.7e-13 at (2, 4) -- two of this model's exponents lie within 0.2 of each other (-5.29, -5.50), which is what Q_end feels;
    250 x 7.7e-13 = 1.9e-10."""
    k = _nakl_case()
    worst = 0.0
    for substeps, qr_every in ((1, 1), (2, 4)):
        a, b = _nakl_reference(k, substeps, qr_every), _nakl_reference(k, substeps, qr_every, np.longdouble)
        el, eq = float(np.abs(a["logsum"] - b["logsum"]).max()), float(np.abs(a["Q_end"] - b["Q_end"]).max())
        print("NaKL substeps=%d qr_every=%d: float64 vs longdouble, logsum %.2e  Q_end %.2e" % (substeps, qr_every, el, eq))
        worst = max(worst, el, eq)
    return worst


def test_generated_nakl_module_with_stimulus():
    """NaKL, D = 4, 18 parameters, a stimulus that moves between its samples; the whole spectrum, gain 2 on the voltage.
    Reference: lyap_ref driven by the complex-step Jacobian of the NumPy model.  Bound: NAKL_TOL (derive_nakl_tol)."""
    k = _nakl_case()
    D, NP, dt = k["D"], k["NP"], k["dt"]
    m = codegen.module_for(nakl, D, NP, nstim=1, stim_ndim=1)
    Nh = 5
    g = np.broadcast_to(k["gain"], (T, D))
    with _capi.Problem(1, D, Nh, np.zeros((Nh, 1)), [0], dt, 1.0, 1.0, k["P"][:1], [6, 0, 3, 17], rhs=_capi.load_rhs_module(m["so"]),
                       t_model=dt * np.arange(Nh), stim=np.zeros(Nh)) as pb:
        for substeps, qr_every in ((1, 1), (2, 4)):
            r = pb.lyapunov(k["x0"], k["P"], 4, STEPS, t0=k["t0"], substeps=substeps, qr_every=qr_every, coupling=g, stim=k["stim"], trace=True)
            plain = pb.predict(k["x0"], k["P"], STEPS, t0=k["t0"], substeps=substeps, every=STEPS, stim=k["stim"])
            ref = _nakl_reference(k, substeps, qr_every)
            el, eq, et = (np.abs(r[key] - ref[key]).max() for key in ("logsum", "Q_end", "trace"))
            print("NaKL substeps=%d qr_every=%d: |device - NumPy| logsum %.3e  Q_end %.3e  trace %.3e; |x_end - predict()| = %.3e"
                  % (substeps, qr_every, el, eq, et, np.abs(r["x_end"] - plain[:, -1]).max()))
            assert not r["status"].any() and not ref["status"].any()
            assert el <= NAKL_TOL and eq <= NAKL_TOL and et <= NAKL_TOL
            assert np.abs(r["x_end"] - plain[:, -1]).max() <= TOL_X * np.abs(plain).max()
        with pytest.raises(_capi.VaError, match="stimulus"):
            pb.lyapunov(k["x0"], k["P"], 4, STEPS)


def test_refusals():
    rng = np.random.RandomState(2)
    x0 = attractor_starts(5, T)
    p = np.full((T, 1), K_TRUE)
    with _handle(5) as pb:
        for bad, word in ((dict(n_steps=42, qr_every=4), "multiple"), (dict(n_steps=40, qr_every=4, n_skip=10), "n_skip"),
                          (dict(n_steps=40, coupling=-np.ones(5)), "gains"), (dict(n_steps=40, coupling=np.full(5, np.nan)), "gains"),
                          (dict(n_steps=0), "at least 1"), (dict(n_steps=40, stim=np.zeros((41, 1))), "no stimulus")):
            with pytest.raises(_capi.VaError, match=word):
                pb.lyapunov(x0, p, 3, **bad)
        with pytest.raises(ValueError, match="K=6"):
            pb.lyapunov(x0, p, 6, 40)
    # a module whose dense linear part was split off
    N = 7
    lin = codegen.module_for(twin.dense_coupling_model(20, 1)[0], 20, 2)
    assert lin["lin"] is not None
    with _capi.Problem(1, 20, N, rng.randn(N, 2), [0, 2], DT, 1.0, 1.0, np.ones((1, 2)), [0], disc="trapezoid",
                       rhs=_capi.load_rhs_module(lin["so"])) as pb:
        with pytest.raises(NotImplementedError, match="linear"):
            pb.lyapunov(rng.randn(1, 20), np.ones((1, 2)), 3, 4)
    # the network action
    s = twin.nnet_structure(20, 10, 10, 10)
    din, dout, _ = twin.make_nnet_twin(s, 2)
    Xn, Pn, Pidx = twin.nnet_initial_guess(s, 2, 0)
    dp = lambda a: a.ctypes.data_as(_capi.c_dp)
    with _capi.NnetProblem(1, s, din, dout, [np.arange(10), np.arange(10)], 4.0e4, 0.0038, Pn[None, :], Pidx) as nb:
        st = np.zeros(1, dtype=np.int32)
        rc = nb._L.va_lyapunov(nb._h, dp(Xn), dp(Xn), None, None, 1, 1, 0.0, 4, 1, 1, 0, None, dp(Xn), dp(Xn), dp(Xn), None,
                               st.ctypes.data_as(_capi.c_ip))
        assert rc == -4 and b"network" in nb._L.va_last_error()
        with pytest.raises(NotImplementedError, match="network"):          # the binding's own guard
            nb.lyapunov(Xn[None, :], Xn[None, :], 1, 4)


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
            pb.lyapunov(np.zeros((2, D)), np.tile(P, (2, 1)), 2, STEPS)
        A1 = pb.action_grad(XP, 2.0)[0]
    assert np.isfinite(A0[0]) and A1[0] == A0[0]


def test_handle_is_left_alone():
    D, N, B = 20, 41, 3
    t, Y, _, Lidx = twin.make_twin(D, N)
    XP = np.stack([np.append(*twin.initial_guess(N, D, b, Y, Lidx)) for b in range(B)])
    x0 = attractor_starts(D, T)
    with _capi.Problem(B, D, N, Y, Lidx, DT, 4.0, 4e-6, XP[:, -1:], [0]) as pb:
        before = pb.action_grad(XP, 30.0)
        pb.lyapunov(x0, np.full((T, 1), K_TRUE), D, STEPS, qr_every=4, coupling=gain_every_second(D), trace=True)
        after = pb.action_grad(XP, 30.0)
        resident = pb.read_eval_outputs()
    for u, v, w in zip(before, after, resident):
        assert np.array_equal(u, v) and np.array_equal(v, w)


def test_rank_deficient_start():
    """two equal tangents in trajectory 1: status 2 and NaN there, the neighbours as in a run without it"""
    D, K = 20, 4
    x0, ks = attractor_starts(D, T), np.array(FORCINGS[:T])[:, None]
    Q0 = np.array(np.broadcast_to(np.linalg.qr(np.random.RandomState(2).randn(D, K))[0].T, (T, K, D)))
    with _handle(D) as pb:
        good = pb.lyapunov(x0, ks, K, STEPS, qr_every=4, Q0=Q0, trace=True)
        Q0[1, 1] = Q0[1, 0]
        got = pb.lyapunov(x0, ks, K, STEPS, qr_every=4, Q0=Q0, trace=True)
    assert list(got["status"]) == [0, 2, 0, 0, 0, 0, 0] and not good["status"].any()
    assert np.all(np.isnan(got["logsum"][1])) and np.all(np.isnan(got["exponents"][1])) and np.all(np.isfinite(got["x_end"]))
    keep = [0, 2, 3, 4, 5, 6]
    for k in ("logsum", "x_end", "Q_end", "trace"):
        assert np.array_equal(got[k][keep], good[k][keep]) and np.all(np.isfinite(good[k])), k
    assert np.array_equal(got["x_end"][1], good["x_end"][1])


def test_annealer_end_to_end():
    """the D = 5, N = 9 anneal of test_gpu_predict_tlm.py's end-to-end case (two seeds, two rungs)"""
    D, N, B = 5, 9, 2
    rng = np.random.RandomState(6)
    Lidx, RM, RF0, alpha = [0, 2, 3], 4.0, 0.5, 2.0
    Y = 2.0 * rng.randn(N, len(Lidx))
    a = va_ode.Annealer()
    a.set_model(_l96_user, D)
    a.set_data(Y, t=DT * np.arange(N))
    a.anneal(rng.randn(B, N, D), np.array([[8.0], [8.5]]), alpha, [0, 1], RM, RF0, Lidx, [0], disc="trapezoid", verbose=False,
             opt_args={'gtol': 1e-10, 'ftol': 1e-14})
    r = a.lyapunov(40)
    s = a.sync_exponents(40, [0, 5])
    mp = a.minpaths
    x0, p = mp[:, -1, (N - 1) * D:N * D], mp[:, -1, N * D:]
    t0 = float(a.t_model[-1])
    raw = a._pb.lyapunov(x0, p, D, 40, t0=t0, qr_every=4)
    assert r["exponents"].shape == r["logsum"].shape == (B, 1, D) and r["Q_end"].shape == (B, 1, D, D) and r["x_end"].shape == (B, 1, D)
    assert r["horizon"].shape == r["kaplan_yorke"].shape == r["status"].shape == (B, 1)
    for k in ("exponents", "logsum", "x_end", "Q_end", "status"):
        assert np.array_equal(r[k][:, 0], raw[k]), k
    assert np.all(np.isfinite(r["exponents"])) and np.all(np.isfinite(r["kaplan_yorke"]))
    g = np.zeros((2, D))
    g[1, Lidx] = 5.0
    raw = a._pb.lyapunov(np.repeat(x0, 2, axis=0), np.repeat(p, 2, axis=0), 1, 40, t0=t0, qr_every=4, coupling=np.tile(g, (B, 1)))
    assert s["exponents"].shape == (B, 1, 2, 1) and s["critical_gain"].shape == (B, 1) and s["status"].shape == (B, 1, 2)
    assert np.array_equal(s["exponents"].reshape(2 * B, 1), raw["exponents"])
    # gain 0 with one tangent: the leading exponent of the whole spectrum (the first column of the QR does not see the others)
    assert np.abs(s["exponents"][:, 0, 0, 0] - r["exponents"][:, 0, 0]).max() <= TOL / (40 * DT)
    assert np.all(s["exponents"][:, :, 1] < s["exponents"][:, :, 0])             # (the gain does contract)
    a.close()
