"""GPU: the block-tridiagonal selected inverse k_selinv and the block builder k_hblocks (csrc/va_selinv.h) through
va_blocktri_selinv and va_laplace, against numpy's dense inverse of reference matrices (tests/_selinv_ref.py: max |Sigma -
Sigma_ref| <= kappa_2(H_ref) 2.2e-16 max |Sigma_ref|, logdet within n kappa 2.2e-16), and end to end through va_ode.Annealer."""
import numpy as np
import pytest

import _hess_ref as hr
import _hess_torch_ref as tr
import _selinv_ref as sr
from varanneal_amd import _capi, codegen, twin, va_ode

pytestmark = pytest.mark.gpu

L96_CASES = ([(d, "plain") for d in ("euler", "forwardmap", "trapezoid", "SimpsonHermite")]
             + [("trapezoid", "nskip"), ("SimpsonHermite", "rfarr")])


def _problem(c, rhs="lorenz96", **kw):
    npts = c["X"].shape[0]
    P = np.broadcast_to(np.asarray(c["P"], float), (npts, len(c["P"]))).copy()
    return _capi.Problem(npts, c["D"], c["N"], c["Y"], c["Lidx"], c["dt"], c["RM"], c["RF0"], P, c["Pidx"], disc=c["disc"],
                         rhs=rhs, merr_nskip=c["nskip"], **kw)


@pytest.fixture(scope="module")
def any_handle():
    """va_blocktri_selinv runs on a handle's device and stream; the blocks are the caller's"""
    c = hr.l96_case("trapezoid")
    with _problem(c) as pb:
        yield pb


def _same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in a)


@pytest.mark.parametrize("W,K,NPe", sr.SHAPES)
def test_raw_solver_matches_the_dense_inverse(any_handle, W, K, NPe):
    """three random positive definite arrow matrices per shape: every block, logdet, status; the same bits on a second
    call; NULL outputs.  (64, 2, 32) keeps Sigma_{k+1,k} in global memory, the others in LDS.
    Measured on an MI355X: ratios err / bound at most 0.60 (W = 17, kappa = 5)."""
    Dk, Bk, Pk, Hpp, H = sr.arrow_batch(W, K, NPe)
    r = any_handle.blocktri_selinv(Dk, Bk, Pk, Hpp)
    assert list(r["status"]) == [0, 0, 0]
    for p in range(3):
        sr.check_blocks("W=%d K=%d NPe=%d pt %d" % (W, K, NPe, p), H[p], W, K, NPe, r["Skk"][p], r["Snk"][p], r["Spk"][p], r["Spp"][p],
                        r["logdet"][p])
    assert _same(r, any_handle.blocktri_selinv(Dk, Bk, Pk, Hpp))
    part = any_handle.blocktri_selinv(Dk, Bk, Pk, Hpp, want=("Skk",))
    assert sorted(part) == ["Skk", "logdet", "status"] and _same(part, {k: r[k] for k in part})
    none = any_handle.blocktri_selinv(Dk, Bk, Pk, Hpp, want=())
    assert np.array_equal(none["logdet"], r["logdet"]) and list(none["status"]) == [0, 0, 0]


def test_raw_solver_not_positive_definite(any_handle):
    W, K, NPe = 5, 4, 1
    Dk, Bk, Pk, Hpp, H = (np.array(a) for a in sr.arrow_batch(W, K, NPe))
    good = any_handle.blocktri_selinv(Dk[[0, 2]], Bk[[0, 2]], Pk[[0, 2]], Hpp[[0, 2]])
    Dk[1, 1] = -Dk[1, 1]
    r = any_handle.blocktri_selinv(Dk, Bk, Pk, Hpp)
    assert list(r["status"]) == [0, 2, 0]
    for name in ("Skk", "Snk", "Spk", "Spp"):
        assert np.all(np.isnan(r[name][1])), name
        assert np.array_equal(r[name][[0, 2]], good[name]), name              # bit for bit
    assert np.isnan(r["logdet"][1]) and np.array_equal(r["logdet"][[0, 2]], good["logdet"])
    Dk, Bk, Pk, Hpp, H = (np.array(a) for a in sr.arrow_batch(W, K, NPe))
    Hpp[2] = -Hpp[2]
    r = any_handle.blocktri_selinv(Dk, Bk, Pk, Hpp)
    assert list(r["status"]) == [0, 0, -1] and np.all(np.isnan(r["Skk"][2])) and np.all(np.isfinite(r["Skk"][:2]))


def _check_laplace(label, r, p, H, N, D, NPe, logdet=True):
    sr.check_time_rows(label, H, N, D, NPe, r["var_x"][p], r.get("cov_xx", [None] * (p + 1))[p], r.get("cov_px", [None] * (p + 1))[p],
                       r["cov_pp"][p], r["logdet"][p] if logdet else None)


@pytest.mark.parametrize("disc,variant", L96_CASES)
def test_laplace_on_the_l96_cases(disc, variant):
    """D = 5, N = 6 / 7, three points: Gauss-Newton against inv(Hgn); chunks of 0 (all), 1 and 2 points give the same bits;
    action_grad on the handle returns the bits it returned before; the full Hessian at these random points is indefinite
    (min eig(H_xx) < 0 in the reference): status > 0 and NaN, no exception."""
    c = hr.l96_case(disc, variant)
    N, D = c["N"], c["D"]
    with _problem(c) as pb:
        before = pb.action_grad(c["X"], c["rf_scale"])
        r = pb.laplace(c["X"], c["rf_scale"], gauss_newton=True, full=True)
        assert list(r["status"]) == [0, 0, 0]
        for p in range(3):
            _check_laplace("%s %s pt %d" % (disc, variant, p), r, p, c["Hgn"][p], N, D, 1)
        for chunk in (1, 2):
            assert _same(r, pb.laplace(c["X"], c["rf_scale"], gauss_newton=True, full=True, chunk_pts=chunk))
        small = pb.laplace(c["X"], c["rf_scale"], gauss_newton=True)
        assert sorted(small) == ["cov_pp", "logdet", "status", "var_x"] and _same(small, {k: r[k] for k in small})
        for p in range(3):
            assert np.linalg.eigvalsh(c["H"][p][:N * D, :N * D]).min() < 0
        bad = pb.laplace(c["X"], c["rf_scale"], full=True)
        assert np.all(bad["status"] > 0)
        for k in ("var_x", "cov_xx", "cov_px", "cov_pp", "logdet"):
            assert np.all(np.isnan(bad[k])), k
        for a, b in zip(before, pb.action_grad(c["X"], c["rf_scale"])):
            assert np.array_equal(a, b)


def test_generated_model_with_two_parameters():
    """hr.two_param_stencil, D = 8, N = 7, Simpson-Hermite: W = 16, K = 4 with a padded last block, NPe = 2; Gauss-Newton
    against the SymPy Gauss-Newton Hessian"""
    D, N, NP, Pidx = 8, 7, 2, [0, 1]
    rng = np.random.RandomState(9)
    n = N * D + 2
    P = 0.6 + 0.8 * rng.rand(NP)
    X = rng.randn(2, n)
    X[:, N * D:] = P[Pidx] + 0.1 * rng.rand(2, 2)
    c = dict(D=D, N=N, disc="SimpsonHermite", nskip=1, Lidx=[0, 2], Pidx=Pidx, Y=rng.randn(N, 2), RM=2.0, RF0=0.7, P=P, X=X, dt=hr.DT)
    rf_scale = 2.0
    sa = hr.SymbolicAction(hr.two_param_stencil, D, N, c["Y"], c["Lidx"], hr.DT, c["RM"], c["RF0"] * rf_scale, P, Pidx, "SimpsonHermite")
    m = codegen.module_for(hr.two_param_stencil, D, 2)
    with _problem(c, rhs=_capi.load_rhs_module(m["so"])) as pb:
        r = pb.laplace(X, rf_scale, P=P, gauss_newton=True, full=True)
        assert list(r["status"]) == [0, 0]
        for p in range(2):
            _check_laplace("stencil pt %d" % p, r, p, sa.gauss_newton(X[p]), N, D, 2)


def _l96(t, x, k):
    return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - x + k


@pytest.mark.parametrize("disc", ["trapezoid", "SimpsonHermite"])
def test_library_geometry_through_the_annealer(disc):
    """D = 20, N = 41, one seed, two rungs: W = 20, K = 41, and W = 40, K = 21 with a padded last block.  The dense Hessian
    action_hessian assembles at each rung's minimiser against dense() of tests/_hess_torch_ref.py, entrywise within
    REL max |H_ref| (measured on an MI355X: 1.1e-16 .. 2.1e-16 of max |H_ref|); then laplace(full=True)
    against numpy.linalg.inv of that assembled matrix (kappa from that matrix);
    param_cov against param_covariance(): both carry a first-order error of kappa 2.2e-16 max |Sigma|, so they agree
    within twice that."""
    D, N = 20, 41
    t, Y, _, Lidx = twin.make_twin(D, N)
    X0, P0 = twin.initial_guess(N, D, 0, Y, Lidx)
    a = va_ode.Annealer()
    a.set_model(_l96, D)
    a.set_data(Y, t=twin.DT * np.arange(N))
    a.anneal(X0, np.array([P0[0]]), 2.0, [0, 1], 4.0, 0.5, Lidx, [0], disc=disc, verbose=False,
             opt_args={'gtol': 1e-10, 'ftol': 1e-14})
    r = a.laplace(full=True)
    assert r["state_var"].shape == (2, N, D) and r["state_cov"].shape == (2, N, D, D) and r["state_param_cov"].shape == (2, 1, N, D)
    assert r["param_cov"].shape == (2, 1, 1) and r["logdet"].shape == (2,) and list(r["status"]) == [0, 0]
    for k in range(2):
        H = a.action_hessian(beta=k, form='dense')
        # that matrix is assembled from hess_vec: hold it, entry by entry, to a Hessian the kernel has no part in
        xp, Pk, rf = a._minimiser(k, 0)
        assert rf == 2.0 ** k
        H_ref = tr.TorchAction(tr.l96, D, N, Y, Lidx, twin.DT, 4.0, 0.5 * 2.0 ** k, Pk, [0], disc).dense(xp)
        herr = np.abs(H - H_ref).max() / np.abs(H_ref).max()
        print("%s rung %d: dense Hessian vs the torch reference %.2e" % (disc, k, herr))
        assert H.shape == H_ref.shape and herr <= hr.REL
        sr.check_time_rows("%s rung %d" % (disc, k), H, N, D, 1, r["state_var"][k], r["state_cov"][k], r["state_param_cov"][k],
                           r["param_cov"][k], r["logdet"][k])
        Sig, kappa, _ = sr.reference(H)
        cov = a.param_covariance(beta=k)
        dc, bound = np.abs(r["param_cov"][k] - cov).max(), 2.0 * kappa * sr.EPS * np.abs(Sig).max()
        print("param_cov vs param_covariance: %.2e  bound %.2e  ratio %.3f" % (dc, bound, dc / bound))
        assert dc <= bound
    se = a.state_stderr()
    assert se.shape == (1, N, D) and np.array_equal(se[0], np.sqrt(r["state_var"][-1]))
    a.close()


def test_batch_selection_and_each_rungs_own_rf():
    """the D = 5, N = 9 setup of test_gpu_hvp.py::test_annealer_covariance_end_to_end with two seeds and two rungs"""
    D, N, B = 5, 9, 2
    rng = np.random.RandomState(6)
    Lidx, RM, RF0, alpha = [0, 2, 3], 4.0, 0.5, 2.0
    Y = 2.0 * rng.randn(N, len(Lidx))
    a = va_ode.Annealer()
    a.set_model(_l96, D)
    a.set_data(Y, t=hr.DT * np.arange(N))
    a.anneal(rng.randn(B, N, D), np.array([[8.0], [8.5]]), alpha, [0, 1], RM, RF0, Lidx, [0], disc="trapezoid", verbose=False,
             opt_args={'gtol': 1e-10, 'ftol': 1e-14})
    r = a.laplace(gauss_newton=True, full=True)
    assert r["state_var"].shape == (B, 2, N, D) and r["param_cov"].shape == (B, 2, 1, 1) and r["logdet"].shape == (B, 2)
    assert r["status"].shape == (B, 2) and r["state_cov"].shape == (B, 2, N, D, D) and r["state_param_cov"].shape == (B, 2, 1, N, D)
    assert not r["status"].any()
    # every (seed, rung) is the single-point call at that minimiser with THAT rung's rf_scale (the same bits), and no other's
    mp = a.minpaths.reshape(B, 2, -1)
    for b in range(B):
        for k in range(2):
            row = mp[b, k]
            one = a._pb.laplace(row[None, :], alpha ** k, P=row[N * D:][None, :], gauss_newton=True)
            assert np.array_equal(one["var_x"][0], r["state_var"][b, k]) and one["logdet"][0] == r["logdet"][b, k]
            other = a._pb.laplace(row[None, :], alpha ** (1 - k), P=row[N * D:][None, :], gauss_newton=True)
            assert not np.array_equal(other["var_x"][0], r["state_var"][b, k])
    sel = a.laplace(beta=1, seeds=[1], gauss_newton=True)
    assert sel["state_var"].shape == (1, 1, N, D) and np.array_equal(sel["state_var"][0, 0], r["state_var"][1, 1])
    assert sorted(sel) == ["logdet", "param_cov", "state_var", "status"]
    assert a.state_stderr(seeds=0, gauss_newton=True).shape == (1, 1, N, D)
    assert a.laplace(beta=[1, 0], gauss_newton=True)["logdet"].shape == (B, 2)
    a.close()


def test_refusals_name_their_reason():
    D, N = 5, 7
    rng = np.random.RandomState(1)
    Y, Lidx = rng.randn(N, 2), [0, 2]
    xp = rng.randn(1, N * D + 1)
    out = np.empty(N * D * 70)
    st = np.empty(1, np.int32)

    def raw(pb, n_var):
        return pb._L.va_laplace(pb._h, xp.ctypes.data_as(_capi.c_dp), None, 1, n_var, np.ones(1).ctypes.data_as(_capi.c_dp), 1, 0,
                                out.ctypes.data_as(_capi.c_dp), None, None, None, out.ctypes.data_as(_capi.c_dp),
                                st.ctypes.data_as(_capi.c_ip))
    # full RF matrices
    with _capi.Problem(1, D, N, Y, Lidx, hr.DT, 1.0, np.resize(np.eye(D), (N - 1, D, D)), np.array([[8.0]]), [0], disc="trapezoid") as pb:
        with pytest.raises(NotImplementedError, match="RF"):
            pb.laplace(xp, 1.0)
    # time-dependent parameters
    from models.nakl import l96_damped_tdp
    m = codegen.module_for(l96_damped_tdp, D, 2, p_rows=True)
    with _capi.Problem(1, D, N, Y, Lidx, hr.DT, 1.0, 1.0, np.ones((1, N, 2)), [0], disc="trapezoid", rhs=_capi.load_rhs_module(m["so"]),
                       p_time_dependent=True, t_model=hr.DT * np.arange(N)) as pb:
        with pytest.raises(NotImplementedError, match="time-dependent"):
            _capi.check(raw(pb, 10 ** 6))
    # the network action
    s = twin.nnet_structure(20, 10, 10, 10)
    din, dout, _ = twin.make_nnet_twin(s, 2)
    Xn, Pn, Pidx = twin.nnet_initial_guess(s, 2, 0)
    with _capi.NnetProblem(1, s, din, dout, [np.arange(10), np.arange(10)], 4.0e4, 0.0038, Pn[None, :], Pidx) as nb:
        assert raw(nb, 10 ** 6) == -4 and b"network" in nb._L.va_last_error()
        with pytest.raises(NotImplementedError, match="network"):          # the binding's own guard
            nb.laplace(Xn[None, :], 1.0)
    # states wider than a block: D = 65, and D = 33 with Simpson-Hermite (W = 66)
    for Dw, disc in ((65, "trapezoid"), (33, "SimpsonHermite")):
        with _capi.Problem(1, Dw, N, Y, Lidx, hr.DT, 1.0, 1.0, np.array([[8.0]]), [0], disc=disc) as pb:
            with pytest.raises(NotImplementedError, match="64"):
                pb.laplace(rng.randn(1, N * Dw + 1), 1.0)
            pb.hess_vec(rng.randn(1, N * Dw + 1), rng.randn(1, 1, N * Dw + 1), 1.0)       # (the products themselves are carried)
    # a forced chunk that does not fit the workspace; a raw solver wider than its limits
    c = hr.l96_case("trapezoid")
    with _problem(c) as pb:
        with pytest.raises(_capi.VaError, match="workspace"):
            pb.laplace(c["X"], 1.0, gauss_newton=True, chunk_pts=10 ** 6)
        with pytest.raises(NotImplementedError, match="64"):
            pb.blocktri_selinv(np.ones((1, 1, 65, 65)), np.ones((1, 0, 65, 65)), np.ones((1, 1, 0, 65)), np.ones((1, 0, 0)))
        with pytest.raises(NotImplementedError, match="32"):
            pb.blocktri_selinv(np.ones((1, 1, 2, 2)), np.ones((1, 0, 2, 2)), np.ones((1, 1, 33, 2)), np.ones((1, 33, 33)))
