"""GPU: the ensemble Kalman filter -- the kernel k_enkf (csrc/va_enkf.h) through va_enkf: the built-in Lorenz-96 against the filter
written in NumPy (tests/_enkf_ref.py, where the tolerance is derived) at every geometry the plan makes, the same bits on a second
call and for a point run alone, a generated Lorenz-96 module, the generated NaKL module with its stimulus and two estimated
parameters, a NaN member, the handle left alone, the refusals, the twin experiment in which the filter has to filter, and
va_ode.Annealer.track end to end."""
import numpy as np
import pytest

import _enkf_ref
from _enkf_ref import KEYS, MISSING_CASE, OBS_EVERY, OBS_VAR, SHAPES, TOL, TWIN, enkf_ref, l96_case, l96_enkf_reference
from _predict_ref import DT, K_TRUE, STEPS
from _util import load_npz_cases
from models.nakl import nakl
from varanneal_amd import _capi, codegen, twin, va_ode

pytestmark = pytest.mark.gpu

ALL = KEYS + ("status",)


def _l96_user(t, x, k):
    return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - x + k


def _handle(D, N=5, rhs=None):
    Lidx = list(range(0, D, 2))
    kw = {} if rhs is None else dict(rhs=rhs)
    return _capi.Problem(1, D, N, np.zeros((N, len(Lidx))), Lidx, DT, 4.0, 1e-2, np.array([[K_TRUE]]), [0], **kw)


def _same(a, b, keys=ALL):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in keys)


def _errors(r, ref):
    return {k: float(np.abs(r[k] - ref[k]).max()) for k in KEYS}


@pytest.mark.parametrize("D,M", SHAPES)
@pytest.mark.parametrize("NQ,substeps,inflation", [(0, 1, 1.0), (1, 2, 1.05)])
def test_lorenz96_matches_numpy(D, M, NQ, substeps, inflation):
    """3 points with a forcing of their own, one workgroup each.  (5, 4), (5, 12): one wave; (5, 13): two waves, idle lanes;
    (20, 8): 192 threads; (20, 30): 256 x 3; (33, 31): 256 x 4, odd width; (64, 32): 256 x 8 full, slots padded to 65; (20, 102):
    256 x 8, idle lanes.  And the same bits on a second call."""
    x0, p, Y, Lidx, ref = l96_enkf_reference(D, M, NQ, substeps, inflation)
    kw = dict(obs_every=OBS_EVERY, est=[0] if NQ else [], inflation=inflation, substeps=substeps)
    with _handle(D) as pb:
        r = pb.enkf(x0, p, Y, OBS_VAR, **kw)
        again = pb.enkf(x0, p, Y, OBS_VAR, **kw)
    e = _errors(r, ref)
    print("D=%d M=%d NQ=%d substeps=%d inflation=%.2f: |device - NumPy| %s" % (D, M, NQ, substeps, inflation,
                                                                                 "  ".join("%s %.3e" % (k, e[k]) for k in KEYS)))
    assert not r["status"].any()
    for k in KEYS:
        assert e[k] <= TOL, k
    assert _same(r, again)


def test_missing_observations_and_a_point_alone():
    """NaN entries scattered over Y and one whole row missing; point 1 of 3 run alone gives the bits it gave in the batch"""
    D, M, NQ, substeps, inflation = MISSING_CASE
    x0, p, Y, Lidx, ref = l96_enkf_reference(D, M, NQ, substeps, inflation, missing=True)
    kw = dict(obs_every=OBS_EVERY, est=[0], inflation=inflation, substeps=substeps)
    with _handle(D) as pb:
        r = pb.enkf(x0, p, Y, OBS_VAR, **kw)
        one = pb.enkf(x0[1:2], p[1:2], Y[1:2], OBS_VAR, **kw)
    e = _errors(r, ref)
    print("missing data: |device - NumPy| %s" % "  ".join("%s %.3e" % (k, e[k]) for k in KEYS))
    assert not r["status"].any() and max(e.values()) <= TOL
    for k in ALL:
        assert np.array_equal(one[k][0], r[k][1]), k


@pytest.mark.parametrize("D,M", [(5, 12), (20, 30)])
def test_generated_lorenz96_module(D, M):
    x0, p, Y, Lidx, ref = l96_enkf_reference(D, M, 1, 2, 1.05)
    m = codegen.module_for(_l96_user, D, 1)
    kw = dict(obs_every=OBS_EVERY, est=[0], inflation=1.05, substeps=2)
    with _handle(D) as pb:
        builtin = pb.enkf(x0, p, Y, OBS_VAR, **kw)
    with _handle(D, rhs=_capi.load_rhs_module(m["so"])) as pb:
        r = pb.enkf(x0, p, Y, OBS_VAR, **kw)
    e = {k: float(np.abs(r[k] - builtin[k]).max()) for k in KEYS}
    print("generated Lorenz-96 D=%d M=%d: |module - built-in| %s" % (D, M, "  ".join("%s %.3e" % (k, e[k]) for k in KEYS)))
    assert not r["status"].any() and max(e.values()) <= TOL and max(_errors(r, ref).values()) <= TOL


# ---------------------------------------------------------------------------------------------------------------
def _nakl_row(t, x, p, st):
    return nakl(t, x[None, :], (p, st[0]))[0]


def _nakl_case():
    """2 points of 10 members around states of the golden NaKL path, the stimulus of test_gpu_lyap.py's case; the voltage observed
    every 4 steps, two conductances estimated"""
    c = load_npz_cases("nakl.npz")["g5_nakl_trapezoid_rf1e+00"]
    D, N, NP, T, M = 4, int(c["N_model"]), 18, 2, 10
    dt = float(c["dt_model"])
    rng = np.random.RandomState(21)
    base = c["XP"][:N * D].reshape(N, D)[::40][:T]
    x0 = base[:, None, :] + rng.randn(T, M, D) * np.array([1.0, 0.01, 0.01, 0.01])
    P = np.tile(c["XP"][N * D:], (T, M, 1))
    est = [0, 3]
    P[:, :, est] *= 1.0 + 0.01 * rng.randn(T, M, 2)
    tt = dt * np.arange(STEPS + 1)
    stim = (10.0 + 25.0 * np.sin(4.0 * tt) ** 2 + 8.0 * tt ** 2)[:, None]
    n_obs = STEPS // OBS_EVERY
    Y = np.array([_enkf_ref.rk4(_nakl_row, base[i], P[i, 0], STEPS, dt, t0=3.0, substeps=2, every=OBS_EVERY, stim=stim)[1:, :1] for i in range(T)])
    Y = Y + rng.randn(T, n_obs, 1)
    Y[0, 4, 0] = np.nan
    return dict(D=D, NP=NP, dt=dt, t0=3.0, x0=x0, P=P, est=est, stim=stim, Y=Y, T=T)


def _nakl_reference(k, dtype=np.float64):
    res = [enkf_ref(_nakl_row, k["x0"][j], k["P"][j], k["est"], k["Y"][j], [0], [1.0], k["dt"], obs_every=OBS_EVERY, substeps=2,
                    inflation=1.05, t0=k["t0"], stim=k["stim"], dtype=dtype) for j in range(k["T"])]
    return {key: np.array([r[key] for r in res]) for key in res[0]}


NAKL_TOL = 2.6e-11


def derive_nakl_tol():
    """NAKL_TOL as _enkf_ref.TOL is derived, for this model and these inputs: the reference in float64 against the same
    computation carried in longdouble, largest absolute difference over all outputs, times the same 250-fold margin.
    Measured: 1.03e-13 (p_end, conductances of size 120 and 20; x_end 4.6e-14, the statistics 4.0e-14); 250 x 1.03e-13 = 2.6e-11."""
    k = _nakl_case()
    a, b = _nakl_reference(k), _nakl_reference(k, np.longdouble)
    e = {key: float(np.abs(np.asarray(a[key], dtype=np.longdouble) - b[key]).max()) for key in KEYS}
    print("NaKL: float64 vs longdouble %s" % "  ".join("%s %.2e" % (key, e[key]) for key in KEYS))
    return max(e.values())


def test_generated_nakl_module_with_stimulus():
    """NaKL, D = 4, M = 10 (one wave), 18 parameters of which two are estimated, a stimulus that moves between its samples,
    substeps = 2, a missing observation.  Reference: enkf_ref driven by models.nakl member by member.  Bound: NAKL_TOL."""
    k = _nakl_case()
    D, NP, dt = k["D"], k["NP"], k["dt"]
    m = codegen.module_for(nakl, D, NP, nstim=1, stim_ndim=1)
    Nh = 5
    ref = _nakl_reference(k)
    with _capi.Problem(1, D, Nh, np.zeros((Nh, 1)), [0], dt, 1.0, 1.0, k["P"][:1, 0], [6, 0, 3, 17], rhs=_capi.load_rhs_module(m["so"]),
                       t_model=dt * np.arange(Nh), stim=np.zeros(Nh)) as pb:
        r = pb.enkf(k["x0"], k["P"], k["Y"], 1.0, obs_every=OBS_EVERY, est=k["est"], inflation=1.05, t0=k["t0"], substeps=2, stim=k["stim"])
        with pytest.raises(_capi.VaError, match="stimulus"):
            pb.enkf(k["x0"], k["P"], k["Y"], 1.0, obs_every=OBS_EVERY, est=k["est"])
    e = _errors(r, ref)
    print("NaKL: |device - NumPy| %s" % "  ".join("%s %.3e" % (key, e[key]) for key in KEYS))
    assert not r["status"].any() and not ref["status"].any()
    assert max(e.values()) <= NAKL_TOL
    assert np.abs(r["p_end"][:, :, k["est"]] - k["P"][:, :, k["est"]]).min() > 0.0          # (both conductances were moved)
    others = [i for i in range(NP) if i not in k["est"]]
    assert np.array_equal(r["p_end"][:, :, others], k["P"][:, :, others])


def test_nan_member_loses_its_point_only():
    """an arithmetic NaN in one member's x0 of point 1: status 1 and NaN statistics there, the other points bit for bit"""
    D, M = 20, 8
    x0, p, Y, Lidx = l96_case(D, M)
    bad0 = np.array(x0)
    bad0[1, 3, 7] = np.nan
    with _handle(D) as pb:
        good = pb.enkf(x0, p, Y, OBS_VAR, obs_every=OBS_EVERY, est=[0], inflation=1.05)
        got = pb.enkf(bad0, p, Y, OBS_VAR, obs_every=OBS_EVERY, est=[0], inflation=1.05)
    assert list(got["status"]) == [0, 1, 0] and not good["status"].any()
    for k in ("mean_f", "sd_f", "mean_a", "sd_a"):
        assert np.all(np.isnan(got[k][1]))
    for k in ALL:
        assert np.array_equal(got[k][[0, 2]], good[k][[0, 2]]), k


def test_the_filter_filters():
    """The twin experiment of tests/test_enkf_cpu.py (_enkf_ref.twin_case): D = 20, every second column observed with noise of
    variance 0.25 every 2 steps, 30 members, inflation 1.05, 60 rows.  RMS error of the analysis mean on the UNOBSERVED columns
    over the second half: below half that of the same ensemble's mean run without observations.  The NumPy reference alone
    gives 0.187 with the data against 3.543 without."""
    c = TWIN
    x0, p, Y, Lidx, un, truth = _enkf_ref.twin_case()
    with _handle(c["D"]) as pb:
        a = pb.enkf(x0, p, Y, c["obs_var"], obs_every=c["obs_every"], inflation=c["inflation"])
        f = pb.enkf(x0, p, np.full_like(Y, np.nan), c["obs_var"], obs_every=c["obs_every"], inflation=c["inflation"])
    ea, ef = _enkf_ref.twin_errors(a["mean_a"][0], f["mean_a"][0])
    print("device: RMS error on the unobserved columns, second half: %.3f with the data, %.3f without" % (ea, ef))
    assert not a["status"].any() and not f["status"].any()
    assert ea < 0.5 * ef


def test_handle_is_left_alone():
    D, N, B = 20, 41, 3
    t, Y, _, Lidx = twin.make_twin(D, N)
    XP = np.stack([np.append(*twin.initial_guess(N, D, b, Y, Lidx)) for b in range(B)])
    x0, p, _, _ = l96_case(D, 8)
    Yf = np.random.RandomState(1).randn(3, 10, len(Lidx)) + 2.0
    with _capi.Problem(B, D, N, Y, Lidx, DT, 4.0, 4e-6, XP[:, -1:], [0]) as pb:
        before = pb.action_grad(XP, 30.0)
        c0 = pb.counters()
        pb.enkf(x0, p, Yf, OBS_VAR, obs_every=OBS_EVERY, est=[0], inflation=1.05)
        c1 = pb.counters()
        resident = pb.read_eval_outputs()
        after = pb.action_grad(XP, 30.0)
    assert c0 == c1
    for u, v, w in zip(before, after, resident):
        assert np.array_equal(u, v) and np.array_equal(u, w)


def test_refusals():
    rng = np.random.RandomState(2)
    x0, p, Y, Lidx = l96_case(20, 8)
    with _handle(20) as pb:
        for kw, word in ((dict(est=[1]), "outside"), (dict(est=[0, 0]), "NQ=2"), (dict(inflation=0.5), "inflation"),
                         (dict(obs_every=0), "at least 1"), (dict(substeps=0), "at least 1"), (dict(stim=np.zeros((41, 1))), "no stimulus")):
            with pytest.raises(_capi.VaError, match=word) as ei:
                pb.enkf(x0, p, Y, OBS_VAR, **dict(dict(obs_every=OBS_EVERY), **kw))
            assert not isinstance(ei.value, NotImplementedError)
        for ov in (0.0, -1.0, np.nan, np.inf):
            with pytest.raises(_capi.VaError, match="variances"):
                pb.enkf(x0, p, Y, ov, obs_every=OBS_EVERY)
        # what the plan refuses comes through as NotImplementedError
        with pytest.raises(NotImplementedError, match="at least 2 members"):
            pb.enkf(x0[:, :1], p[:, :1], Y, OBS_VAR, obs_every=OBS_EVERY)
        big = np.zeros((1, 103, 20))
        with pytest.raises(NotImplementedError, match="2048"):
            pb.enkf(big, K_TRUE * np.ones((1, 103, 1)), Y[:1], OBS_VAR, obs_every=OBS_EVERY)
    # a model without a flat form
    D, N = 200, 65
    Lw = list(range(0, D, 2))
    P = K_TRUE + 0.1 * rng.randn(1, D)
    m = codegen.module_for(_l96_user, D, D, colparams=True,
                           col_variant=lambda ne, gh, reach=None: _capi.eval_plan(1, D, N, "trapezoid", ne, gh, reach=reach, Lidx=Lw))
    with _capi.Problem(1, D, N, rng.randn(N, len(Lw)), Lw, DT, 4.0, 1e-2, P, list(range(D)), rhs=_capi.load_rhs_module(m["so"])) as pb:
        with pytest.raises(NotImplementedError, match="flat form"):
            pb.enkf(np.zeros((1, 4, D)), np.tile(P, (4, 1)), np.zeros((2, len(Lw))), 1.0)
    # the network action
    s = twin.nnet_structure(20, 10, 10, 10)
    din, dout, _ = twin.make_nnet_twin(s, 2)
    Xn, Pn, Pidx = twin.nnet_initial_guess(s, 2, 0)
    with _capi.NnetProblem(1, s, din, dout, [np.arange(10), np.arange(10)], 4.0e4, 0.0038, Pn[None, :], Pidx) as nb:
        with pytest.raises(NotImplementedError, match="network"):
            nb.enkf(np.zeros((1, 2, 4)), np.zeros(1), np.zeros((2, 1)), 1.0)


def test_module_with_a_split_linear_part_is_carried():
    """the members move through the predictor's right-hand side, which adds the dense linear part the generator split off:
    without observations x_end is predict()'s forecast of every member, bit for bit"""
    rng = np.random.RandomState(3)
    N, D, M = 7, 20, 6
    lin = codegen.module_for(twin.dense_coupling_model(D, 1)[0], D, 2)
    assert lin["lin"] is not None
    x0 = 0.5 * rng.randn(2, M, D)
    p = np.ones((2, M, 2)) + 0.01 * rng.randn(2, M, 2)
    with _capi.Problem(1, D, N, rng.randn(N, 2), [0, 2], DT, 1.0, 1.0, np.ones((1, 2)), [0], disc="trapezoid",
                       rhs=_capi.load_rhs_module(lin["so"])) as pb:
        r = pb.enkf(x0, p, np.full((3, 2), np.nan), 1.0, obs_every=2, est=[0])
        plain = pb.predict(x0.reshape(-1, D), p.reshape(-1, 2), 6)
        obs = pb.enkf(x0, p, np.zeros((3, 2)), 1.0, obs_every=2, est=[0])
    assert not r["status"].any() and np.array_equal(r["x_end"].reshape(-1, D), plain[:, -1]) and np.array_equal(r["p_end"], p)
    assert not obs["status"].any() and np.all(np.isfinite(obs["mean_a"])) and not np.array_equal(obs["x_end"], r["x_end"])


def test_annealer_track_end_to_end(golden_ladders):
    """a short anneal() on the first 61 rows of the golden D = 20 data, then the next 10 rows tracked: members from the Laplace
    posterior, and members from sample()"""
    c = golden_ladders["g4_c1_trapezoid_N200"]
    D, N, n_obs, M = int(c["D"]), 61, 10, 8
    Lidx = list(c["Lidx"])
    L = len(Lidx)
    a = va_ode.Annealer()
    a.set_model(twin.l96, D)
    a.set_data(c["Y"][:N], t=c["t"][:N])
    a.anneal(c["X0"][:N].copy(), c["P0"].copy(), float(c["alpha"]), c["beta"][:12], 4.0, 4e-6, Lidx, [0],
             dt_model=float(c["t"][1] - c["t"][0]), init_to_data=True, disc="trapezoid", method='L-BFGS-B',
             opt_args={'gtol': 1e-8, 'ftol': 1e-8, 'maxfun': 1000000, 'maxiter': 1000000}, adolcID=0, verbose=False)
    Yf = c["Y"][N:N + n_obs]
    stats = ("mean", "std", "mean_forecast", "std_forecast", "params", "params_std", "innovation")

    def consistent(r, M):
        """shapes; an ensemble was built; finite up to the first lost row (status k + 1), NaN from there; the innovation"""
        assert r["mean"].shape == r["std"].shape == r["mean_forecast"].shape == r["std_forecast"].shape == (1, n_obs, D)
        assert r["params"].shape == r["params_std"].shape == (1, n_obs, 1) and r["innovation"].shape == (1, n_obs, L)
        assert r["x_end"].shape == (1, M, D) and r["p_end"].shape == (1, M, 1) and r["status"].shape == (1,)
        assert np.all(np.isfinite(r["mean_forecast"][0, 0])), "no initial ensemble: status %s" % r["status"]
        good = n_obs if r["status"][0] == 0 else int(r["status"][0]) - 1
        assert 1 <= good <= n_obs
        for k in stats:
            assert np.all(np.isfinite(r[k][0, :good])) and np.all(np.isnan(r[k][0, good:])), k
        assert np.array_equal(r["innovation"], Yf - r["mean_forecast"][..., Lidx], equal_nan=True)
        # the analysis pulls the observed columns towards the data
        assert np.abs(Yf - r["mean"][..., Lidx])[0, :good].mean() <= np.abs(r["innovation"])[0, :good].mean()
        return good
    # (12 rungs leave the exact Hessian indefinite at this point: the Gauss-Newton part gives the posterior its factor)
    r = a.track(Yf, members=M, inflation=1.05, seed=3, gauss_newton=True)
    good = consistent(r, M)
    print("track, members from the Laplace factor: status %s (%d of %d rows)  k = %s  mean |innovation| %.3f"
          % (r["status"], good, n_obs, r["params"][0, :good, 0], np.abs(r["innovation"][0, :good]).mean()))
    again = a.track(Yf, members=M, inflation=1.05, seed=3, gauss_newton=True)
    assert all(np.array_equal(r[k], again[k], equal_nan=True) for k in r)
    other = a.track(Yf, members=M, inflation=1.05, seed=4, gauss_newton=True)
    assert not np.array_equal(r["mean"][0, 0], other["mean"][0, 0])               # (another seed, other members)
    s = a.sample(6, n_leap=4, seed=1)
    rs = a.track(Yf, samples=s, obs_var=0.25)
    good = consistent(rs, 6)
    print("track, members from sample(): status %s (%d of %d rows)" % (rs["status"], good, n_obs))
    assert list(rs["rungs"]) == list(s["rungs"])
    a.close()
