"""GPU: va_hess_vec (csrc/va_hvp.h k_hvp) against the SymPy Hessians of tests/_hess_ref.py, against central differences of
the library's own gradient at the shipped example's shape, and end to end through va_ode.Annealer."""
import numpy as np
import pytest

import _hess_ref as hr
from varanneal_amd import _capi, codegen, twin, va_ode

pytestmark = pytest.mark.gpu

L96_CASES = ([(d, "plain") for d in ("euler", "forwardmap", "trapezoid", "SimpsonHermite")]
             + [("trapezoid", "nskip"), ("SimpsonHermite", "rfarr")])


def _problem(c, rhs="lorenz96", **kw):
    npts = c["X"].shape[0]
    P = np.broadcast_to(np.asarray(c["P"], float), (npts, len(c["P"]))).copy()
    return _capi.Problem(npts, c["D"], c["N"], c["Y"], c["Lidx"], c["dt"], c["RM"], c["RF0"], P, c["Pidx"], disc=c["disc"],
                         rhs=rhs, merr_nskip=c["nskip"], **kw)


@pytest.mark.parametrize("disc,variant", L96_CASES)
def test_l96_matches_the_sympy_hessian(disc, variant):
    """D = 5, N = 7 / 6, 3 distinct points x 4 directions, tile rows 0 / 2 / 3, full and Gauss-Newton; the parameter rows
    are the same bits when the call is repeated; action_grad on the handle returns the bits it returned before."""
    c = hr.l96_case(disc, variant)
    with _problem(c) as pb:
        before = pb.action_grad(c["X"], c["rf_scale"])
        for gn, H in ((False, c["H"]), (True, c["Hgn"])):
            want = np.einsum("pij,pvj->pvi", H, c["V"])
            for tr in (0, 2, 3):
                got = pb.hess_vec(c["X"], c["V"], c["rf_scale"], gauss_newton=gn, tile_rows=tr)
                err = hr.rel_err(got, want)
                print("%s %s gn=%d tile_rows=%d  max |Hv - H_ref v| / max |H_ref v| = %.2e" % (disc, variant, gn, tr, err))
                assert err <= hr.REL
                again = pb.hess_vec(c["X"], c["V"], c["rf_scale"], gauss_newton=gn, tile_rows=tr)
                assert np.array_equal(again[:, :, c["N"] * c["D"]:], got[:, :, c["N"] * c["D"]:])
        _same_bits(before, pb.action_grad(c["X"], c["rf_scale"]))
        with pytest.raises(_capi.VaError):
            pb.hess_vec(c["X"], c["V"], c["rf_scale"], tile_rows=1000)          # more rows than the path has


def _same_bits(before, after):
    for a, b in zip(before, after):
        assert np.array_equal(a, b)


def _generated(f, D, N, NP, Pidx, disc, seed, stim=None, sym_f=None, scale=1.0):
    rng = np.random.RandomState(seed)
    Lidx = [0, 2]
    n = N * D + len(Pidx)
    P = 0.6 + 0.8 * rng.rand(NP)
    X = scale * rng.randn(2, n)
    X[:, N * D:] = P[Pidx] + 0.1 * rng.rand(2, len(Pidx))
    c = dict(D=D, N=N, disc=disc, nskip=1, Lidx=Lidx, Pidx=Pidx, Y=rng.randn(N, 2), RM=2.0, RF0=0.7, P=P, X=X,
             V=rng.randn(2, 3, n), rf_scale=2.0, dt=hr.DT, stim=stim)
    sa = hr.SymbolicAction(sym_f or f, D, N, c["Y"], Lidx, c["dt"], c["RM"], c["RF0"] * c["rf_scale"], P, Pidx, disc, stim=stim,
                           gauss_newton=False)
    c["want"] = np.einsum("pij,pvj->pvi", np.array([sa.hessian(x) for x in X]), c["V"])
    return c


def test_generated_stencil_with_parameter_cross_terms():
    """D = 8, N = 7: two parameters that multiply states, both estimated (a non-empty pgrad2, d2f/dxdp)"""
    D, N = 8, 7
    m = codegen.module_for(hr.two_param_stencil, D, 2)
    c = _generated(hr.two_param_stencil, D, N, 2, [0, 1], "SimpsonHermite", 9)
    with _problem(c, rhs=_capi.load_rhs_module(m["so"])) as pb:
        before = pb.action_grad(c["X"], c["rf_scale"])
        for tr in (0, 3):
            err = hr.rel_err(pb.hess_vec(c["X"], c["V"], c["rf_scale"], P=c["P"], tile_rows=tr), c["want"])
            print("stencil tile_rows=%d: %.2e" % (tr, err))
            assert err <= hr.REL
        _same_bits(before, pb.action_grad(c["X"], c["rf_scale"]))


def test_nakl_with_its_stimulus():
    """D = 4, N = 9, 18 parameters of which three are estimated, transcendental functions, a stimulus"""
    from models.nakl import nakl
    D, N = 4, 9
    stim = np.sin(0.7 * np.arange(N)) + 0.3
    m = codegen.module_for(nakl, D, 18, nstim=1)
    c = _generated(nakl, D, N, 18, [0, 6, 7], "trapezoid", 12, stim=stim, sym_f=hr.nakl_sym, scale=0.3)
    with _problem(c, rhs=_capi.load_rhs_module(m["so"]), stim=stim) as pb:
        before = pb.action_grad(c["X"], c["rf_scale"])
        err = hr.rel_err(pb.hess_vec(c["X"], c["V"], c["rf_scale"], P=c["P"], tile_rows=4), c["want"])
        print("NaKL: %.2e" % err)
        assert err <= hr.REL
        _same_bits(before, pb.action_grad(c["X"], c["rf_scale"]))


def test_library_geometry_against_central_differences():
    """D = 20, N = 161, trapezoid, the library's own tiles (4 of 52 rows): (grad(x + d v) - grad(x - d v)) / 2 d of the
    existing action_grad, d = 1e-4 |x|_inf / |v|_inf.  Truncation ~1e-8 relative; a seam or index error is O(1)."""
    D, N = 20, 161
    t, Y, _, Lidx = twin.make_twin(D, N)
    X0, P0 = twin.initial_guess(N, D, 0, Y, Lidx)
    xp = np.append(X0.ravel(), P0[0])
    rng = np.random.RandomState(2)
    V = rng.randn(2, xp.size)
    rf = 50.0
    with _capi.Problem(1, D, N, Y, Lidx, twin.DT, 4.0, 4e-6, np.array([P0]), [0], disc="trapezoid") as pb:
        got = pb.hess_vec(xp[None, :], V, rf)
        for k in range(2):
            d = 1e-4 * np.abs(xp).max() / np.abs(V[k]).max()
            gp = pb.action_grad((xp + d * V[k])[None, :], rf)[3][0]
            gm = pb.action_grad((xp - d * V[k])[None, :], rf)[3][0]
            want = (gp - gm) / (2.0 * d)
            err = np.abs(got[k] - want).max() / np.abs(want).max()
            print("central difference, direction %d: %.2e" % (k, err))
            assert err <= 1e-6


@pytest.mark.parametrize("rm_array", [False, True])
def test_wide_state_on_a_streaming_kernel_handle(rm_array):
    """D = 200, N = 21: the handle runs the streaming column-strip kernel, whose observation weights live in padded rows
    (scalar weights spread out into that image as well) -- hess_vec reads them at the handle's pitch.  Reference: central
    differences of the handle's own action_grad, as above."""
    D, N = 200, 21
    t, Y, _, Lidx = twin.make_twin(D, N)
    X0, P0 = twin.initial_guess(N, D, 0, Y, Lidx)
    xp = np.append(X0.ravel(), P0[0])
    rng = np.random.RandomState(4)
    V = rng.randn(2, xp.size)
    RM = 4.0 * (0.25 + rng.rand(N, len(Lidx))) if rm_array else 4.0
    rf = 5.0e4                                      # (both terms of the action matter at this rung)
    with _capi.Problem(1, D, N, Y, Lidx, twin.DT, RM, 4e-6, np.array([P0]), [0], disc="trapezoid") as pb:
        assert pb.info()["eval_kernel"] == 5
        before = pb.action_grad(xp[None, :], rf)
        got = pb.hess_vec(xp[None, :], V, rf)
        # the measurement term alone: H v on the observed entries is 2 cme w v when the model term is switched off
        meas = pb.hess_vec(xp[None, :], V, 0.0)
        w = np.zeros((N, D))
        w[:, Lidx] = RM
        want_meas = np.concatenate([(2.0 / (len(Lidx) * N) * w).ravel(), [0.0]]) * V
        assert np.abs(meas - want_meas).max() <= 1e-14 * np.abs(want_meas).max()      # (three products in another order: a few ulp)
        for k in range(2):
            d = 1e-4 * np.abs(xp).max() / np.abs(V[k]).max()
            gp = pb.action_grad((xp + d * V[k])[None, :], rf)[3][0]
            gm = pb.action_grad((xp - d * V[k])[None, :], rf)[3][0]
            want = (gp - gm) / (2.0 * d)
            err = np.abs(got[k] - want).max() / np.abs(want).max()
            print("wide state (rm_array=%s), direction %d: %.2e" % (rm_array, k, err))
            assert err <= 1e-6
        _same_bits(before, pb.action_grad(xp[None, :], rf))


def _l96(t, x, k):
    return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - x + k


def test_annealer_covariance_end_to_end():
    """D = 5, N = 9, two rungs of anneal(): action_hessian and param_covariance against the SymPy Hessian at the returned
    minimiser"""
    D, N = 5, 9
    rng = np.random.RandomState(6)
    Lidx, RM, RF0, alpha = [0, 2, 3], 4.0, 0.5, 2.0
    Y = 2.0 * rng.randn(N, len(Lidx))
    a = va_ode.Annealer()
    a.set_model(_l96, D)
    a.set_data(Y, t=hr.DT * np.arange(N))
    a.anneal(rng.randn(N, D), np.array([8.0]), alpha, [0, 1], RM, RF0, Lidx, [0], disc="trapezoid", verbose=False,
             opt_args={'gtol': 1e-10, 'ftol': 1e-14})
    mp = a.minpaths[-1]
    before = a._pb.action_grad(mp[None, :], alpha)
    sa = hr.SymbolicAction(hr.l96, D, N, Y, Lidx, hr.DT, RM, RF0 * alpha ** 1, np.array([8.0]), [0], "trapezoid", gauss_newton=False)
    H_ref = sa.hessian(mp)
    H = a.action_hessian(form='dense')
    err = np.abs(H - H_ref).max() / np.abs(H_ref).max()
    cond = np.linalg.cond(H_ref)
    print("dense Hessian: %.2e   cond_2 = %.2e" % (err, cond))
    assert err <= hr.REL
    assert np.linalg.eigvalsh(H_ref[:N * D, :N * D]).min() > 0          # (a minimiser with three of five columns observed)
    cov = a.param_covariance()
    want = np.linalg.inv(H_ref)[N * D:, N * D:]
    cerr = np.abs(cov - want).max() / np.abs(want).max()
    print("covariance %s vs %s: %.2e" % (cov, want, cerr))
    assert cerr <= 1e-10 * cond
    _same_bits(before, a._pb.action_grad(mp[None, :], alpha))
    a.close()


def test_refusals_name_their_reason():
    D, N = 5, 7
    rng = np.random.RandomState(1)
    Y, Lidx = rng.randn(N, 2), [0, 2]
    xp, V = rng.randn(1, N * D + 1), rng.randn(1, 1, N * D + 1)
    # full RF matrices
    with _capi.Problem(1, D, N, Y, Lidx, hr.DT, 1.0, np.resize(np.eye(D), (N - 1, D, D)), np.array([[8.0]]), [0], disc="trapezoid") as pb:
        with pytest.raises(NotImplementedError, match="RF"):
            pb.hess_vec(xp, V, 1.0)
    # time-dependent parameters
    from models.nakl import l96_damped_tdp
    m = codegen.module_for(l96_damped_tdp, D, 2, p_rows=True)
    with _capi.Problem(1, D, N, Y, Lidx, hr.DT, 1.0, 1.0, np.ones((1, N, 2)), [0], disc="trapezoid", rhs=_capi.load_rhs_module(m["so"]),
                       p_time_dependent=True, t_model=hr.DT * np.arange(N)) as pb:
        with pytest.raises(NotImplementedError, match="time-dependent"):
            _capi.check(pb._L.va_hess_vec(pb._h, xp.ctypes.data_as(_capi.c_dp), None, V.ctypes.data_as(_capi.c_dp), 1, 1,
                                          10 ** 6, 1.0, 0, 0, V.ctypes.data_as(_capi.c_dp)))
    # a module whose dense linear part was split off
    lin = codegen.module_for(twin.dense_coupling_model(20, 1)[0], 20, 2)
    assert lin["lin"] is not None
    with _capi.Problem(1, 20, N, Y, Lidx, hr.DT, 1.0, 1.0, np.ones((1, 2)), [0], disc="trapezoid",
                       rhs=_capi.load_rhs_module(lin["so"])) as pb:
        with pytest.raises(NotImplementedError, match="linear"):
            pb.hess_vec(rng.randn(1, N * 20 + 1), rng.randn(1, 1, N * 20 + 1), 1.0)
    # the network action
    s = twin.nnet_structure(20, 10, 10, 10)
    din, dout, _ = twin.make_nnet_twin(s, 2)
    Xn, Pn, Pidx = twin.nnet_initial_guess(s, 2, 0)
    with _capi.NnetProblem(1, s, din, dout, [np.arange(10), np.arange(10)], 4.0e4, 0.0038, Pn[None, :], Pidx) as nb:
        rc = nb._L.va_hess_vec(nb._h, Xn.ctypes.data_as(_capi.c_dp), None, Xn.ctypes.data_as(_capi.c_dp), 1, 1, 10 ** 6, 1.0, 0, 0,
                               Xn.ctypes.data_as(_capi.c_dp))
        assert rc == -4 and b"network" in nb._L.va_last_error()
        with pytest.raises(NotImplementedError, match="network"):          # the binding's own guard
            nb.hess_vec(Xn[None, :], Xn[None, None, :], 1.0)
