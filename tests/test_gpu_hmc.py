"""GPU: the Hamiltonian Monte Carlo sampler (va_hmc; csrc/va_hmc.h) against the NumPy chain of tests/_hmc_ref.py, whose gradient
is Problem.action_grad on a SECOND handle of the same problem.  Every chain is fed explicit noise unless the test is about
the generator.  Positions, final states, running means and variances: bit for bit; dH within the summation-order bound
derived in _hmc_ref; every accept decision equal (the reference asserts no decision lies within that bound); a second call
gives the same bits.  n_iter = 6, n_leap = 5 throughout."""
import numpy as np
import pytest

import _hmc_ref as R
from varanneal_amd import _capi, codegen, twin, va_ode

pytestmark = pytest.mark.gpu
N_ITER, N_LEAP = 6, 5


def _noise(B, n, seed=1):
    rs = np.random.RandomState(seed)
    z = rs.randn(N_ITER, B, n + 2)
    z[:, :, n:] = rs.uniform(0.02, 1.0, (N_ITER, B, 2))
    return z


def _compare(make, XP, rf, eps, want_kernel, both=False, minv=None, thin=1, keep=None, jitter=0.25, seed=1):
    """make(): a fresh handle of the problem; want_kernel: the evaluation kernel family it must report (1 flat, 3, 4, 5);
    both: the chains must hold accepted AND rejected iterations (the restore from the saved point runs on the device).
    Returns (device result, reference)."""
    B, n = XP.shape
    noise = _noise(B, n, seed)
    keep = np.arange(n) if keep is None else np.asarray(keep)
    with make() as pg:
        # the evaluator repeats its own bits from call to call (else nothing below can be bit for bit)
        first, again = pg.action_grad(XP, rf), pg.action_grad(XP, rf)
        assert all(np.array_equal(a, b) for a, b in zip(first, again))
        ref = R.chain(XP, lambda X: pg.action_grad(X, rf)[::3], eps, N_ITER, N_LEAP, noise, jitter=jitter, minv=minv, thin=thin, keep_idx=keep)
    assert R.decisions_are_safe(ref)
    with make() as pb:
        assert pb.info()["eval_kernel"] == want_kernel, pb.info()
        assert pb.info()["n_var"] == n
        got = pb.hmc(XP, rf, N_ITER, N_LEAP, eps, jitter=jitter, minv=minv, noise=noise, thin=thin, keep_idx=keep)
        twice = pb.hmc(XP, rf, N_ITER, N_LEAP, eps, jitter=jitter, minv=minv, noise=noise, thin=thin, keep_idx=keep)
    for k in got:
        assert np.array_equal(got[k], twice[k], equal_nan=True), "second call: " + k
    assert np.array_equal(got["accepted"], ref["accepted"])
    if both:
        assert 0 < got["accepted"].sum() < got["accepted"].size
    if thin == 1 and keep.size == n:
        assert np.array_equal(got["kept"], ref["x_trace"].transpose(1, 0, 2))                 # the x traces
    for k in ("kept", "x", "mean", "var", "A"):
        assert np.array_equal(got[k], ref[k]), k
    fin = np.isfinite(ref["dH"])
    assert np.array_equal(np.isfinite(got["dH"]), fin) and np.array_equal(got["n_divergent"], ref["n_divergent"])
    err = np.abs(got["dH"] - ref["dH"])[fin]
    print("accepted %d of %d; |dH dev - dH ref| / bound at most %.3f" % (ref["accepted"].sum(), ref["accepted"].size,
                                                                         (err / ref["dh_bound"][fin]).max() if err.size else 0.0))
    assert np.all(err <= ref["dh_bound"][fin])
    return got, ref


def _l96(D, N, B, disc="trapezoid", seed=0, **kw):
    t, Y, _, Lidx = twin.make_twin(D, N)
    XP = np.empty((B, N * D + 1)); P = np.empty((B, 1))
    for b in range(B):
        X0, P0 = twin.initial_guess(N, D, b + seed, Y, Lidx)
        XP[b, :-1] = X0.ravel(); XP[b, -1] = P0[0]; P[b] = P0
    return (lambda: _capi.Problem(B, D, N, Y, Lidx, twin.DT, 4.0, 4e-6, P, [0], disc=disc, **kw)), XP


# eps: the action is normalised (its gradient is O(1 / N)), so unit-mass steps of order 1 move the path visibly in 5 steps
@pytest.mark.parametrize("disc", ["euler", "trapezoid", "SimpsonHermite", "forwardmap"])
def test_l96_small_every_discretisation(disc):
    """D = 5, N = 9, B = 3: n_var = 46, less than one wave; per-chain step sizes.  The library runs paths this short on k_eval3"""
    make, XP = _l96(5, 9, 3, disc)
    _compare(make, XP, 40.0, np.array([0.6, 1.1, 1.9]), 3, both=True)


def test_l96_flat_kernel():
    """the same small shape on the flat kernel (asked for)"""
    make, XP = _l96(5, 9, 3, eval_kernel=1)
    _compare(make, XP, 40.0, np.array([0.6, 1.1, 1.9]), 1, both=True)


def test_l96_several_workgroups_per_chain():
    """D = 20, N = 60: n_var = 1201, two workgroups per chain, the second one ragged in the energy sum"""
    make, XP = _l96(20, 60, 3)
    _compare(make, XP, 40.0, 1.5, 4, both=True)


def test_l96_workgroup_column_runs():
    """D = 20, N = 60 on k_eval3 (asked for: the library's own choice at this width is k_eval4): rejected iterations restore the
    state across two workgroups per chain"""
    make, XP = _l96(20, 60, 3, eval_kernel=3)
    _compare(make, XP, 40.0, 1.5, 3, both=True)


def test_l96_streaming_kernel():
    """D = 66, N = 8: the streaming column-strip kernel"""
    make, XP = _l96(66, 8, 2)
    _compare(make, XP, 10.0, 1.0, 5, both=True)


def test_handle_with_a_persistent_ladder():
    """B = 1 on a handle whose ladders run as the persistent kernel: sampling uses the evaluation kernel only, and a ladder
    afterwards gives the bits it gives on a fresh handle"""
    make, XP = _l96(20, 200, 1, max_beta=2)
    with make() as pb:
        assert pb.persistent() is not None
    _compare(make, XP, 40.0, 1.5, 4)
    opts = {'gtol': 1e-8, 'ftol': 1e-8, 'maxfun': 200, 'maxiter': 200}
    rf = 1.5 ** np.arange(2)
    with make() as fresh:
        want = fresh.anneal(XP, rf, opts)
    with make() as pb:
        pb.hmc(XP, 40.0, N_ITER, N_LEAP, 1.5, seed=3)
        got = pb.anneal(XP, rf, opts)
    for k in ("x", "A", "pest", "nit", "nfev", "status"):
        assert np.array_equal(got[k], want[k]), k


def test_mass_shapes_thinning_and_scattered_columns():
    """minv shared by the chains and per chain, thin = 2, a scattered keep_idx (with a repeated entry)"""
    make, XP = _l96(5, 9, 3)
    n = XP.shape[1]
    rs = np.random.RandomState(4)
    for minv in (rs.uniform(0.5, 2.0, n), rs.uniform(0.5, 2.0, (3, n))):
        got, _ = _compare(make, XP, 40.0, np.array([0.5, 0.9, 1.4]), 3, both=True, minv=minv, thin=2, keep=[45, 0, 17, 44, 17])
        assert got["kept"].shape == (3, 3, 5)


def test_nakl_with_stimulus_unbounded():
    """generated NaKL, D = 4, N = 11, a stimulus, 4 estimated parameters"""
    from models.nakl import nakl
    D, N, Pidx = 4, 11, [0, 6, 7, 12]
    rng = np.random.RandomState(12)
    stim = np.sin(0.7 * np.arange(N)) + 0.3
    rid = _capi.load_rhs_module(codegen.module_for(nakl, D, 18, nstim=1)["so"])
    P = 0.6 + 0.8 * rng.rand(18)
    Y = rng.randn(N, 2)
    XP = 0.3 * rng.randn(2, N * D + 4)
    XP[:, N * D:] = P[Pidx] + 0.1 * rng.rand(2, 4)
    make = lambda: _capi.Problem(2, D, N, Y, [0, 2], 0.02, 2.0, 0.7, np.tile(P, (2, 1)), Pidx, disc="trapezoid", rhs=rid, stim=stim)
    _compare(make, XP, 2.0, 0.05, 1)


def test_column_parameter_form():
    """Lorenz-96 with a forcing per site in column-parameter form, D = 8, N = 7, P0 = 8"""
    def l96(t, x, k):
        return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - x + k
    D, N, B = 8, 7, 2
    P0 = np.full(8, 8.0)
    Pidx = list(range(D))
    rng = np.random.RandomState(3)
    Lidx = list(range(0, D, 2))
    Y = rng.randn(N, len(Lidx))
    m = codegen.module_for(l96, D, D, colparams=True,
                           col_variant=lambda ne, gh, reach=None: _capi.eval_plan(B, D, N, "trapezoid", ne, gh, reach=reach, Lidx=Lidx))
    rid = _capi.load_rhs_module(m["so"])
    XP = np.stack([np.append(3.0 * rng.randn(N * D), P0 + 0.1 * rng.randn(D)) for b in range(B)])
    make = lambda: _capi.Problem(B, D, N, Y, Lidx, 0.025, 4.0, 0.01, np.tile(P0, (B, 1)), Pidx, disc="trapezoid", rhs=rid)
    _compare(make, XP, 20.0, 0.3, 4)


def test_time_dependent_parameters():
    """built-in Lorenz-96 with a forcing per time row, D = 5, N = 9: the path vector is [X | p_est time-major]"""
    D, N, B = 5, 9, 2
    t, Y, _, Lidx = twin.make_twin(D, N)
    rng = np.random.RandomState(6)
    P = 8.0 + 0.3 * rng.randn(B, N, 1)
    XP = np.concatenate([3.0 * rng.randn(B, N * D), P[:, :, 0]], axis=1)
    make = lambda: _capi.Problem(B, D, N, Y, Lidx, twin.DT, 4.0, 4e-6, P, [0], disc="trapezoid", p_time_dependent=True)
    _compare(make, XP, 40.0, 0.8, 1)


def test_full_rf_matrices():
    """a full model-error precision matrix per time step, (N - 1, D, D) as tests/golden/rffull.npz's cases have it"""
    D, N, B = 5, 9, 2
    t, Y, _, Lidx = twin.make_twin(D, N)
    rng = np.random.RandomState(8)
    M = rng.randn(N - 1, D, D)
    RF0 = 1e-3 * (np.einsum("nij,nkj->nik", M, M) + D * np.eye(D))
    XP = np.concatenate([3.0 * rng.randn(B, N * D), 8.0 + 0.1 * rng.randn(B, 1)], axis=1)
    make = lambda: _capi.Problem(B, D, N, Y, Lidx, twin.DT, 4.0, RF0, np.full((B, 1), 8.0), [0], disc="trapezoid")
    _compare(make, XP, 10.0, 0.8, 1)


# ---------------------------------------------------------------- the generator
def test_noise_words_and_normals():
    seed, chain, it, n = 0xC0FFEE1234567, 5, 77, 1201
    words, normals, uniforms = _capi.hmc_noise(seed, chain, it, n)
    ref = R.words(seed, chain, it, n)
    assert np.array_equal(words, ref)
    assert np.array_equal(uniforms, R.u01(ref[n, :2]))
    err = np.abs(normals - R.box_muller(ref[:n, 0], ref[:n, 1]))
    bound = R.normal_bound(ref[:n, 0])
    print("normals: worst |device - NumPy| / bound = %.3f" % (err / bound).max())
    assert np.all(err <= bound)


def test_internal_generator_equals_its_own_noise_fed_back():
    make, XP = _l96(5, 9, 3)
    B, n = XP.shape
    seed = 987654321987
    noise = np.empty((N_ITER, B, n + 2))
    for it in range(N_ITER):
        for b in range(B):
            _, z, u = _capi.hmc_noise(seed, b, it, n)
            noise[it, b] = np.concatenate([z, u])
    with make() as pb:
        a = pb.hmc(XP, 40.0, N_ITER, N_LEAP, 1.2, jitter=0.25, seed=seed, keep_idx=np.arange(n))
        b_ = pb.hmc(XP, 40.0, N_ITER, N_LEAP, 1.2, jitter=0.25, noise=noise, keep_idx=np.arange(n))
    for k in a:
        assert np.array_equal(a[k], b_[k], equal_nan=True), k
    assert 0 < a["accepted"].sum()


# ---------------------------------------------------------------- the handle afterwards
def test_ladder_bits_and_counters_after_sampling():
    make, XP = _l96(5, 9, 3)
    opts = {'gtol': 1e-8, 'ftol': 1e-8, 'maxfun': 200, 'maxiter': 200}
    rf = 1.5 ** np.arange(3)
    with _l96(5, 9, 3, max_beta=3)[0]() as pb:
        want = pb.anneal(XP, rf, opts)
    with _l96(5, 9, 3, max_beta=3)[0]() as pb:
        c0 = pb.counters()
        pb.hmc(XP, 40.0, N_ITER, N_LEAP, 1.0, seed=1)
        c1 = pb.counters()
        assert c1["seed_evals"] - c0["seed_evals"] == 3 * (N_ITER * N_LEAP + 1)
        assert c1["eval_launches"] - c0["eval_launches"] == N_ITER * N_LEAP + 1
        got = pb.anneal(XP, rf, opts)
    for k in ("x", "A", "pest", "nit", "nfev", "status"):
        assert np.array_equal(got[k], want[k]), k


def test_refusals():
    D, N = 5, 9
    make, XP = _l96(D, N, 1)
    with make() as pb:
        for kw, word in ((dict(n_iter=0), "n_iter"), (dict(n_leap=0), "n_leap"), (dict(thin=0), "thin"), (dict(eps=0.0), "eps"),
                         (dict(eps=np.inf), "eps"), (dict(jitter=1.0), "jitter"), (dict(minv=np.zeros(XP.shape[1])), "minv"),
                         (dict(keep_idx=[XP.shape[1]]), "keep_idx")):
            args = dict(n_iter=2, n_leap=2, eps=0.1)
            args.update(kw)
            with pytest.raises(_capi.VaError, match=word) as e:
                pb.hmc(XP, 1.0, **args)
            assert e.value.code == -1
    t, Y, _, Lidx = twin.make_twin(D, N)
    with _capi.Problem(1, D, N, Y, Lidx, twin.DT, 4.0, 4e-6, [[8.0]], [0], bounds=[(-15.0, 15.0)] * (N * D + 1)) as pb:
        with pytest.raises(_capi.VaUnsupported, match="bounds"):
            pb.hmc(XP, 1.0, 2, 2, 0.1)
    s = twin.nnet_structure(20, 10, 10, 10)
    din, dout, _ = twin.make_nnet_twin(s, 2)
    Xn, Pn, Pidx = twin.nnet_initial_guess(s, 2, 0)
    with _capi.NnetProblem(1, s, din, dout, [np.arange(10), np.arange(10)], 4.0e4, 0.0038, Pn[None, :], Pidx) as nb:
        XPn = np.ascontiguousarray(np.append(Xn, Pn[Pidx])[None, :])
        with pytest.raises(NotImplementedError):
            nb.hmc(XPn, 1.0, 2, 2, 0.1)
        # ... and the library itself, reached past the Python layer's check: VA_EUNSUPPORTED, the path untouched
        before, eps = XPn.copy(), np.array([0.1])
        rc = _capi.lib().va_hmc(nb._h, XPn.ctypes.data, XPn.shape[1], _capi.MEM_HOST, 1.0, 2, 2, eps.ctypes.data_as(_capi.c_dp), 0.0,
                                None, 0, 1, None, 1, None, 0, None, None, None, None, None, None, None)
        assert rc == _capi.VA_EUNSUPPORTED and b"network" in _capi.lib().va_last_error()
        assert np.array_equal(XPn, before)


# ---------------------------------------------------------------- Annealer.sample / predict_ensemble
def test_annealer_sample_and_ensemble_end_to_end():
    D, N, B = 5, 9, 2
    t, Y, _, Lidx = twin.make_twin(D, N)

    def l96(t, x, k):
        return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - x + k
    an = va_ode.Annealer()
    an.set_model(l96, D)
    an.set_data(Y, t=t)
    X0 = np.stack([twin.initial_guess(N, D, b, Y, Lidx)[0] for b in range(B)])
    P0 = np.array([twin.initial_guess(N, D, b, Y, Lidx)[1] for b in range(B)])
    an.anneal(X0, P0, 1.5, np.arange(4), 4.0, 4e-6, Lidx, [0], disc="trapezoid", verbose=False,
              opt_args={'gtol': 1e-8, 'ftol': 1e-8, 'maxfun': 500, 'maxiter': 500})
    calls = []
    hmc = an._pb.hmc
    an._pb.hmc = lambda *a, **k: calls.append((a, k, hmc(*a, **k))) or calls[-1][2]
    r = an.sample(8, beta=[2, 3], n_leap=4, warmup=6, warmup_block=3, thin=2, seed=5, mass='laplace')
    n_var = N * D + 1
    assert r["mean"].shape == (B, 2, n_var) and r["x_last"].shape == (B, 2, 8, D) and r["params"].shape == (B, 2, 8, 1)
    assert r["A"].shape == (B, 2, 16) and np.all(np.isfinite(r["mean"])) and np.all(r["std"] >= 0)
    # two warm-up blocks and one sampling call per rung; the statistics are the sampling call's alone
    assert [c[0][2] for c in calls] == [3, 3, 16, 3, 3, 16]
    assert np.array_equal(r["mean"][:, 0], calls[2][2]["mean"]) and np.array_equal(r["mean"][:, 1], calls[5][2]["mean"])
    assert np.array_equal(calls[1][0][0], calls[0][2]["x"]) and np.array_equal(calls[3][0][0], calls[2][2]["x"])     # each continues the last
    assert np.array_equal(calls[1][0][4], va_ode.hmc_rescale_step(calls[0][0][4], calls[0][2]["accepted"].mean(axis=1)))
    assert len({c[1]["seed"] for c in calls}) == 6
    ens = an.predict_ensemble(10, r, every=5)
    assert ens["members"].shape == (B, 2, 8, 3, D) and ens["quantiles"].shape == (3, B, 2, 3, D)
    P = np.repeat(an._mp[:, [2, 3]][:, :, None, N * D:], 8, axis=2)
    P[..., 0] = r["params"][..., 0]
    want = an._pb.predict(r["x_last"].reshape(-1, D), P.reshape(-1, 1), 10, t0=float(t[-1]), every=5)
    assert np.array_equal(ens["members"].reshape(want.shape), want)
    assert np.array_equal(ens["members"][..., 0, :], r["x_last"])
    an.close()
