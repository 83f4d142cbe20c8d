"""GPU: the box sampler (va_hmc_box; csrc/va_hmc_box.h) against the NumPy chain of tests/_hmc_box_ref.py, whose gradient is
Problem.action_grad on a SECOND handle of the same problem.  Explicit noise everywhere; n_iter = 6, n_leap = 5.  The first test
runs the map alone on the device: positions can only be asked bit for bit if it passes.  Then positions, z, running
statistics, kept columns and decisions as the reference, dH within the bound derived in _hmc_box_ref, a second call the
same bits, the handle's resident paths as they were."""
import numpy as np
import pytest

import _hmc_box_ref as BR
from varanneal_amd import _capi, codegen, twin, va_ode

pytestmark = pytest.mark.gpu
N_ITER, N_LEAP = 6, 5


def test_map_on_the_device_equals_numpy():
    """hmc_box_map in one launch over the table of the CPU test: x, dx, dlj bit for bit (the device's double sqrt and division
    are correctly rounded in this build), lj within the 2 ulp of two logarithms"""
    lo, hi, z = BR.map_table()
    x, dx, dlj, lj = BR.box_map(BR.box_kinds(lo, hi), lo, hi, z)
    gx, gdx, gdlj, glj = _capi.hmc_box_map(lo, hi, z)
    for name, a, b in (("x", gx, x), ("dx", gdx, dx), ("dlj", gdlj, dlj)):
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, "%s differs at %d entries, first z = %r box (%r, %r): %r vs %r" % (name, bad.size, z[bad[0]], lo[bad[0]], hi[bad[0]], a[bad[0]], b[bad[0]])
    print("lj: at most %.2f ulp" % (np.abs(glj - lj) / np.spacing(np.abs(lj)).clip(5e-324)).max())
    assert np.all(np.abs(glj - lj) <= 2 * np.spacing(np.abs(lj)))


def _noise(B, n, seed=1):
    """accept uniforms: iterations 0 and 3 accept whatever is finite, 1 and 4 reject, 2 and 5 decide by their draw"""
    rs = np.random.RandomState(seed)
    z = rs.randn(N_ITER, B, n + 2)
    z[:, :, n:] = rs.uniform(0.02, 1.0, (N_ITER, B, 2))
    z[0::3, :, n] = 1e-300
    z[1::3, :, n] = 1e30
    return z


def _compare(make_ref, make_dev, XP, rf, eps, bounds, pass_bounds, want_kernel, minv=None, thin=1, keep=None, jitter=0.25, seed=1):
    """make_ref(): a handle for the reference's gradient; make_dev(): the handle sampled on, with `bounds` passed to hmc_box
    (pass_bounds) or left to the handle.  Returns (device result, reference)."""
    B, n = XP.shape
    noise = _noise(B, n, seed)
    keep = np.arange(n) if keep is None else np.asarray(keep)
    lo, hi = BR.bounds_arrays(bounds)
    z0 = BR.box_inverse(BR.box_kinds(lo, hi), lo, hi, XP)
    with make_ref() as pg:
        first, again = pg.action_grad(XP, rf), pg.action_grad(XP, rf)
        assert all(np.array_equal(a, b) for a, b in zip(first, again))
        ref = BR.chain_box(z0, lambda X: pg.action_grad(X, rf)[::3], lo, hi, eps, N_ITER, N_LEAP, noise, jitter=jitter, minv=minv, thin=thin, keep_idx=keep)
    assert BR.decisions_are_safe(ref)
    assert 0 < ref["accepted"].sum() < ref["accepted"].size
    other = XP[::-1] * 0.5 + 0.25                                                 # resident paths to find again afterwards
    with make_dev() as pb:
        assert want_kernel is None or pb.info()["eval_kernel"] == want_kernel, pb.info()
        assert pb.info()["n_var"] == n
        before = pb.action_grad(other, rf)
        kw = dict(bounds=bounds if pass_bounds else None, jitter=jitter, minv=minv, noise=noise, thin=thin, keep_idx=keep)
        got = pb.hmc_box(XP, rf, N_ITER, N_LEAP, eps, **kw)
        pb.eval_timed(rf, 1)
        after = pb.read_eval_outputs()
        twice = pb.hmc_box(XP, rf, N_ITER, N_LEAP, eps, **kw)
        cont = pb.hmc_box(XP, rf, N_ITER, N_LEAP, eps, z0=z0, **kw)              # the same start given in z: XP is only written
    for a, b in zip(before, after):
        assert np.array_equal(a, b), "resident paths"
    for k in got:
        assert np.array_equal(got[k], twice[k], equal_nan=True), "second call: " + k
        assert np.array_equal(got[k], cont[k], equal_nan=True), "start in z: " + k
    assert np.array_equal(got["accepted"], ref["accepted"])
    if thin == 1 and keep.size == n:
        assert np.array_equal(got["kept"], ref["x_trace"].transpose(1, 0, 2))
    for k in ("kept", "x", "z", "mean", "var", "A"):
        assert np.array_equal(got[k], ref[k]), k
    assert np.all(got["kept"] >= lo[keep]) and np.all(got["kept"] <= hi[keep])
    fin = np.isfinite(ref["dH"])
    assert np.array_equal(np.isfinite(got["dH"]), fin) and np.array_equal(got["n_divergent"], ref["n_divergent"])
    err = np.abs(got["dH"] - ref["dH"])[fin]
    print("accepted %d of %d; |dH dev - dH ref| / bound at most %.3f" % (ref["accepted"].sum(), ref["accepted"].size,
                                                                         (err / ref["dh_bound"][fin]).max() if err.size else 0.0))
    assert np.all(err <= ref["dh_bound"][fin])
    return got, ref


def _l96(D, N, B, col_bounds, par_bounds, bounded):
    """(make, XP, bounds): the built-in Lorenz-96 with one estimated parameter; bounds per column repeated along time; the
    start is twin.initial_guess's, moved inside its box where it lies outside"""
    t, Y, _, Lidx = twin.make_twin(D, N)
    XP = np.empty((B, N * D + 1)); P = np.empty((B, 1))
    for b in range(B):
        X0, P0 = twin.initial_guess(N, D, b, Y, Lidx)
        XP[b, :-1] = X0.ravel(); XP[b, -1] = P0[0]; P[b] = P0
    bounds = [col_bounds[i % D] for i in range(N * D)] + [par_bounds]
    lo, hi = BR.bounds_arrays(bounds)
    XP = np.clip(XP, lo + 0.5, hi - 0.5)                                          # (the guesses stray past +-9: half a unit inside)
    kw = dict(bounds=bounds) if bounded else {}
    return (lambda: _capi.Problem(B, D, N, Y, Lidx, twin.DT, 4.0, 4e-6, P, [0], disc="trapezoid", **kw)), XP, bounds


COLS5 = [(-15.0, 15.0), (-12.0, None), (None, 14.0), (None, None), (-9.0, 9.0)]
EPS3 = np.array([0.04, 0.08, 0.15])


def _inside(XP, bounds):
    lo, hi = BR.bounds_arrays(bounds)
    return bool(np.all(XP > lo) and np.all(XP < hi))


def test_l96_bounds_passed_on_an_unbounded_handle():
    """D = 5, N = 9, B = 3: every kind in the path vector, per-chain step sizes, bounds as arguments of the call"""
    make, XP, bounds = _l96(5, 9, 3, COLS5, (0.5, None), bounded=False)
    assert _inside(XP, bounds)
    _compare(make, make, XP, 40.0, EPS3, bounds, True, 3)


def test_l96_bounds_of_a_bounded_handle():
    """the same chains with lower = upper = NULL on a handle created with the bounds (it evaluates with another kernel than
    the unbounded handle, so the reference takes its gradient from a second BOUNDED handle: other kernel, other rounding)"""
    _, XP, bounds = _l96(5, 9, 3, COLS5, (0.5, None), bounded=False)
    make_b = _l96(5, 9, 3, COLS5, (0.5, None), bounded=True)[0]
    _compare(make_b, make_b, XP, 40.0, EPS3, bounds, False, None)


def test_l96_mass_shapes_thinning_and_scattered_columns():
    make, XP, bounds = _l96(5, 9, 3, COLS5, (0.5, None), bounded=False)
    n = XP.shape[1]
    minv = np.random.RandomState(4).uniform(0.5, 2.0, (3, n))
    got, _ = _compare(make, make, XP, 40.0, EPS3, bounds, True, 3, minv=minv, thin=2, keep=[45, 0, 17, 44, 17])
    assert got["kept"].shape == (3, 3, 5)


def test_l96_two_workgroups_per_chain():
    """D = 20, N = 52, one parameter: n_var = 1041, two workgroups per chain, the second ragged; kind 3 everywhere"""
    make, XP, bounds = _l96(20, 52, 2, [(-15.0, 15.0)] * 20, (0.5, 15.5), bounded=False)
    assert XP.shape[1] == 1041 and _inside(XP, bounds)
    _compare(make, make, XP, 40.0, 0.1, bounds, True, None)


def _nakl():
    from models.nakl import PB, STATE_BOUNDS, nakl
    D, N, Pidx = 4, 11, [0, 6, 7, 12]
    rng = np.random.RandomState(12)
    stim = np.sin(0.7 * np.arange(N)) + 0.3
    rid = _capi.load_rhs_module(codegen.module_for(nakl, D, 18, nstim=1)["so"])
    pb = np.array(PB)
    P = pb[:, 0] + (pb[:, 1] - pb[:, 0]) * (0.3 + 0.4 * rng.rand(18))
    Y = -65.0 + 10.0 * rng.randn(N, 2)
    Y[:, 1] = 0.5 + 0.1 * rng.randn(N)
    X = np.empty((2, N, D))
    X[..., 0] = -65.0 + 10.0 * rng.randn(2, N)
    X[..., 1:] = 0.1 + 0.8 * rng.rand(2, N, 3)
    XP = np.concatenate([X.reshape(2, -1), P[Pidx] * (1.0 + 0.02 * rng.rand(2, 4))], axis=1)
    bounds = [tuple(STATE_BOUNDS[i % D]) for i in range(N * D)] + [tuple(PB[i]) for i in Pidx]
    make = lambda: _capi.Problem(2, D, N, Y, [0, 2], 0.02, 2.0, 0.7, np.tile(P, (2, 1)), Pidx, disc="trapezoid", rhs=rid, stim=stim)
    return make, XP, bounds


def test_nakl_start_on_a_bound_is_refused_by_name():
    """generated NaKL, D = 4, N = 11, a stimulus, 4 estimated parameters, the tutorial's two-sided bounds on everything; state
    m at the second time point of chain 1 exactly on its lower bound"""
    make, XP, bounds = _nakl()
    XP[1, 5] = 0.0
    with make() as pb:
        with pytest.raises(_capi.VaError, match=r"XP\[1\]\[5\] = 0 is not strictly inside") as e:
            pb.hmc_box(XP, 2.0, 2, 2, 0.01, bounds=bounds)
        assert e.value.code == -1


def test_nakl_pulled_in_start_agrees_with_the_reference():
    make, XP, bounds = _nakl()
    XP[1, 5] = 0.0
    lo, hi = BR.bounds_arrays(bounds)
    XP, n_pulled = va_ode.hmc_box_pull_in(XP, lo, hi)
    assert list(n_pulled) == [0, 1] and XP[1, 5] == 1e-6 and _inside(XP, bounds)
    _compare(make, make, XP, 2.0, 0.01, bounds, True, 1)


def test_annealer_sample_on_a_bounded_anneal():
    """two seeds, two rungs, D = 5, N = 9, bounds on every state and on the parameter: the documented keys, every kept value
    inside its box, predict_ensemble takes the result.  (Without the box sampler this raised NotImplementedError.)"""
    D, N, B = 5, 9, 2
    t, Y, _, Lidx = twin.make_twin(D, N)

    def l96(t, x, k):
        return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - x + k
    an = va_ode.Annealer()
    an.set_model(l96, D)
    an.set_data(Y, t=t)
    X0 = np.stack([twin.initial_guess(N, D, b, Y, Lidx)[0] for b in range(B)])
    P0 = np.array([twin.initial_guess(N, D, b, Y, Lidx)[1] for b in range(B)])
    sb, pbnd = (-15.0, 15.0), (0.5, 15.0)
    an.anneal(X0, P0, 1.5, np.arange(4), 4.0, 4e-6, Lidx, [0], disc="trapezoid", verbose=False, bounds=[sb] * D + [pbnd],
              opt_args={'gtol': 1e-8, 'ftol': 1e-8, 'maxfun': 500, 'maxiter': 500})
    r = an.sample(8, beta=[2, 3], n_leap=4, warmup=6, warmup_block=3, thin=2, seed=5, mass='laplace')
    n_var = N * D + 1
    for k in ("mean", "std", "accept_rate", "n_divergent", "step_size", "A", "dH", "x", "x_last", "params", "seeds", "rungs", "mass_note", "n_pulled_in"):
        assert k in r, k
    assert r["mean"].shape == (B, 2, n_var) and r["x_last"].shape == (B, 2, 8, D) and r["params"].shape == (B, 2, 8, 1)
    assert r["n_pulled_in"].shape == (B, 2) and np.all(r["n_pulled_in"][:, 1] == 0)
    assert np.all(np.isfinite(r["mean"])) and np.all(r["std"] >= 0)
    assert np.all(r["x_last"] > sb[0]) and np.all(r["x_last"] < sb[1])
    assert np.all(r["params"] > pbnd[0]) and np.all(r["params"] < pbnd[1])
    assert np.all(r["x"][..., :-1] > sb[0]) and np.all(r["x"][..., :-1] < sb[1])
    ens = an.predict_ensemble(10, r, every=5)
    assert ens["members"].shape == (B, 2, 8, 3, D) and np.array_equal(ens["members"][..., 0, :], r["x_last"])
    an.close()


def test_refusals():
    D, N = 5, 9
    make, XP, bounds = _l96(D, N, 1, COLS5, (0.5, None), bounded=False)
    with make() as pb:
        with pytest.raises(_capi.VaUnsupported, match="no bounds"):
            pb.hmc_box(XP, 1.0, 2, 2, 0.1)
        with pytest.raises(_capi.VaUnsupported, match="no bounds"):
            pb.hmc_box(XP, 1.0, 2, 2, 0.1, bounds=[(None, None)] * XP.shape[1])
        bad = list(bounds)
        bad[7] = (3.0, 3.0)
        with pytest.raises(_capi.VaError, match=r"lower\[7\] = 3 >= upper\[7\] = 3") as e:
            pb.hmc_box(XP, 1.0, 2, 2, 0.1, bounds=bad)
        assert e.value.code == -1
        with pytest.raises(_capi.VaError, match="n_leap"):
            pb.hmc_box(XP, 1.0, 2, 0, 0.1, bounds=bounds)
    s = twin.nnet_structure(20, 10, 10, 10)
    din, dout, _ = twin.make_nnet_twin(s, 2)
    Xn, Pn, Pidx = twin.nnet_initial_guess(s, 2, 0)
    with _capi.NnetProblem(1, s, din, dout, [np.arange(10), np.arange(10)], 4.0e4, 0.0038, Pn[None, :], Pidx) as nb:
        XPn = np.ascontiguousarray(np.append(Xn, Pn[Pidx])[None, :])
        with pytest.raises(NotImplementedError):
            nb.hmc_box(XPn, 1.0, 2, 2, 0.1, bounds=[(-9.0, 9.0)] * XPn.shape[1])
        # ... and the library itself, reached past the Python layer's check: VA_EUNSUPPORTED, the path untouched
        before, eps = XPn.copy(), np.array([0.1])
        rc = _capi.lib().va_hmc_box(nb._h, XPn.ctypes.data, XPn.shape[1], _capi.MEM_HOST, 1.0, 2, 2, eps.ctypes.data_as(_capi.c_dp), 0.0,
                                    None, 0, 1, None, 1, None, 0, None, None, None, None, None, None, None, None, None, None, None)
        assert rc == _capi.VA_EUNSUPPORTED and b"network" in _capi.lib().va_last_error()
        assert np.array_equal(XPn, before)
