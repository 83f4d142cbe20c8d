"""GPU: models in column-parameter form (codegen.colparam_form: shared scalars + per-column parameter vectors, e.g. a
Lorenz-96 forcing per site) on the column-run kernels k_eval4 / k_eval5 -- against the NumPy restatement of the
reference's action with complex-step derivatives, against the flat kernel, seed by seed, and end to end past the flat
kernel's 128 parameters."""
import os

import numpy as np
import pytest

import va_oracle
from varanneal_amd import _capi, codegen, va_ode

pytestmark = pytest.mark.gpu


def l96(t, x, k):
    """examples/Lorenz96_D20/Lorenz96_anneal.py:15-16"""
    return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - x + k


def mixed(t, x, p):
    """two shared scalars (coupling, damping) and two interleaved vectors (forcing p[2 + 2i], gain p[3 + 2i])"""
    D = x.shape[1]
    return p[0] * np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - p[1] * x * p[3:3 + 2 * D:2] + p[2:2 + 2 * D:2]


GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DISCS = ["trapezoid", "SimpsonHermite", "euler"]


def colparams_inputs(D, N, data, seed):
    """tools/gen_golden_colparams.py's inputs of a case, from its seed: (t, Y, Lidx, X0, P0, Pidx, 3 directions)"""
    rng = np.random.RandomState(seed)
    if data == 0:
        rec = np.load(os.path.join(GOLD, "l96_D20_dt0p025_N161_sm0p5_sec1_mem1.npy"))
        t, Y, Lidx = rec[:N, 0], rec[:N, 1:][:, [0, 2, 4, 6, 8, 10, 14, 16]], [0, 2, 4, 6, 8, 10, 14, 16]
    else:
        Lidx = list(range(0, D, 2))
        t = 0.025 * np.arange(N)
        Y = 3.0 * rng.randn(N, len(Lidx))
    X0 = 20.0 * rng.rand(N, D) - 10.0
    P0 = 8.0 + rng.rand(D)
    Pidx = [i for i in range(D) if i % 7 != 3]
    U = rng.randn(3, N * D + len(Pidx))
    return t, Y, Lidx, X0, P0, Pidx, U


@pytest.mark.parametrize("case", range(5))
def test_reference_golden(case):
    """the reference's own A and complex-step directional derivatives (tests/golden/colparams.npz) for l96 with a forcing
    per site: D = 20 on the shipped recording (k_eval4, forced), D = 200 on synthetic data (k_eval5)"""
    z = np.load(os.path.join(GOLD, "colparams.npz"))
    D, N, data, di, seed = (int(v) for v in z["cases"][case])
    disc, rf = DISCS[di], float(z["rf_scale"][case])
    t, Y, Lidx, X0, P0, Pidx, U = colparams_inputs(D, N, data, seed)
    ek = 4 if D == 20 else 0
    m = codegen.module_for(l96, D, D, colparams=True,
                           col_variant=lambda ne, gh, reach=None: _capi.eval_plan(1, D, N, disc, ne, gh, eval_kernel=ek,
                                                                                reach=reach, Lidx=Lidx))
    XP = np.append(X0.ravel(), P0[Pidx])[None, :]
    with _capi.Problem(1, D, N, Y, Lidx, t[1] - t[0], 4.0, 4e-6, P0[None, :], Pidx, disc=disc, eval_kernel=ek,
                       rhs=_capi.load_rhs_module(m["so"])) as pr:
        assert pr.info()["eval_kernel"] == (4 if D == 20 else 5)
        A, me, fe, g = pr.action_grad(XP, rf)
    assert abs(A[0] - z["A"][case]) <= 1e-12 * abs(z["A"][case])
    assert abs(me[0] - z["me"][case]) <= 1e-12 * abs(z["A"][case]) and abs(fe[0] - z["fe"][case]) <= 1e-12 * abs(z["A"][case])
    for k in range(3):
        gu = np.dot(g[0], U[k])
        assert abs(gu - z["dA"][case][k]) <= 1e-10 * np.dot(np.abs(g[0]), np.abs(U[k])), (k, gu, z["dA"][case][k])


def _problem(f, D, N, NP, B, disc, P, Pidx, seed=3, rf_array=False, nskip=1, eval_kernel=0, tile_rows=0):
    rng = np.random.RandomState(seed)
    Lidx = list(range(0, D, 2))
    N_data = (N - 1) // nskip + 1
    Y = rng.randn(N_data, len(Lidx))
    RF0 = 0.01 * (0.5 + rng.rand(N - 1, D)) if rf_array else 0.01
    m = codegen.module_for(f, D, NP, colparams=True,
                           col_variant=lambda ne, gh, reach=None: _capi.eval_plan(
                               B, D, N, disc, ne, gh, rf_array=rf_array, merr_nskip=nskip, eval_kernel=eval_kernel,
                               tile_rows=tile_rows, reach=reach, Lidx=Lidx))
    assert m["colp"] is not None and m["col_variant"] is not None
    rid = _capi.load_rhs_module(m["so"])
    XP = np.stack([np.append(3.0 * rng.randn(N * D), P[b][Pidx] + 0.1 * rng.randn(len(Pidx))) for b in range(B)])
    kw = dict(disc=disc, rhs=rid, merr_nskip=nskip, eval_kernel=eval_kernel, tile_rows=tile_rows)
    return Lidx, Y, RF0, XP, kw


def _check_grad(f, D, N, NP, disc, P, Pidx, want_kernel, **opts):
    Lidx, Y, RF0, XP, kw = _problem(f, D, N, NP, 1, disc, P[None, :], Pidx, **opts)
    rf = 20.0
    with _capi.Problem(1, D, N, Y, Lidx, 0.025, 4.0, RF0, P[None, :], Pidx, **kw) as pr:
        assert pr.info()["eval_kernel"] == want_kernel
        A, me, fe, g = pr.action_grad(XP, rf)
    fun = lambda z: va_oracle.numpy_action_generic(f, z, D, N, Y, Lidx, 0.025, 4.0, RF0 * rf, NP, Pidx, P, disc,
                                                   nskip=opts.get("nskip", 1))
    A0 = fun(XP[0])[0]
    assert abs(A[0] - A0) <= 1e-12 * abs(A0)
    g0 = va_oracle.complex_step_grad(fun, XP[0])
    assert np.abs(g[0] - g0).max() <= 1e-10 * np.abs(g0).max()
    ND = N * D
    assert np.abs(g[0, ND:] - g0[ND:]).max() <= 1e-10 * np.abs(g0[ND:]).max()      # (the parameter block on its own scale)


@pytest.mark.parametrize("disc", ["trapezoid", "SimpsonHermite", "euler"])
def test_mixed_form_k_eval4(disc):
    """shared scalars, estimated and fixed vector entries, on k_eval4 (D = 20, chosen by itself: NP = 42 runs nowhere else
    with colparams=True)"""
    D, N = 20, 61
    NP = 2 + 2 * D
    rng = np.random.RandomState(5)
    P = np.concatenate([[1.0, 1.0], np.ravel(np.stack([8.0 + rng.rand(D), 0.8 + 0.4 * rng.rand(D)], 1))])
    Pidx = [0] + [2 + 2 * i for i in range(0, D, 3)] + [3 + 2 * i for i in (1, 4, 19)]      # (p[1] and the rest fixed)
    _check_grad(mixed, D, N, NP, disc, P, Pidx, 4)


def test_rf_array_and_nskip_k_eval4():
    D, N = 20, 61
    P = 8.0 + np.random.RandomState(6).rand(D)
    _check_grad(l96, D, N, D, "trapezoid", P, list(range(0, D, 2)), 4, rf_array=True)
    _check_grad(l96, D, N, D, "trapezoid", P, list(range(D)), 4, nskip=2)


@pytest.mark.parametrize("disc", ["trapezoid", "SimpsonHermite"])
def test_per_site_forcing_k_eval5(disc):
    """D = 200: the streaming kernel, 200 parameters (past the flat kernel's 128), all but a few estimated"""
    D, N = 200, 65
    P = 8.0 + np.random.RandomState(7).rand(D)
    Pidx = [i for i in range(D) if i % 17 != 3]
    _check_grad(l96, D, N, D, disc, P, Pidx, 5)


def test_rf_array_k_eval5():
    D, N = 200, 65
    P = 8.0 + np.random.RandomState(8).rand(D)
    _check_grad(l96, D, N, D, "trapezoid", P, list(range(D)), 5, rf_array=True)


@pytest.mark.parametrize("D,N,want", [(20, 61, 4), (200, 65, 5)])
def test_seeds_are_independent(D, N, want):
    """B = 3: every seed's (A, grad A) equals a B = 1 run of that seed, bit for bit (the same rows per workgroup)"""
    B = 3
    tr = 84 if D == 20 else 32
    rng = np.random.RandomState(11)
    P = 8.0 + rng.rand(B, D)
    Pidx = list(range(D))
    Lidx, Y, RF0, XP, kw = _problem(l96, D, N, D, B, "trapezoid", P, Pidx, tile_rows=tr)
    with _capi.Problem(B, D, N, Y, Lidx, 0.025, 4.0, RF0, P, Pidx, **kw) as pr:
        assert pr.info()["eval_kernel"] == want
        A, me, fe, g = pr.action_grad(XP, 30.0)
        A2, _, _, g2 = pr.action_grad(XP, 30.0)
    assert np.array_equal(A, A2) and np.array_equal(g, g2)                           # run to run
    for b in range(B):
        kw1 = _problem(l96, D, N, D, 1, "trapezoid", P[b:b + 1], Pidx, tile_rows=tr)[4]
        with _capi.Problem(1, D, N, Y, Lidx, 0.025, 4.0, RF0, P[b:b + 1], Pidx, **kw1) as pr:
            A1, _, _, g1 = pr.action_grad(XP[b:b + 1], 30.0)
        assert A1[0] == A[b] and np.array_equal(g1[0], g[b])


def test_agrees_with_the_flat_kernel():
    """NP = 40 <= 128: the same problem on the flat kernel (eval_kernel = 1) and on k_eval4 (forced) agrees within 1e-12,
    and a 20-iteration L-BFGS takes the same path on both"""
    D, N, B = 20, 201, 2
    NP = 2 * D
    rng = np.random.RandomState(9)
    P = np.tile(np.append(8.0 + rng.rand(D), 0.8 + 0.4 * rng.rand(D)), (B, 1))
    Pidx = [0, 5, 19, 20, 23, 24, 25, 31, 39]

    def fd(t, x, p):
        D = x.shape[1]
        return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - p[D:2 * D] * x + p[:D]
    Lidx, Y, RF0, XP, kw4 = _problem(fd, D, N, NP, B, "trapezoid", P, Pidx, eval_kernel=4)
    res = {}
    for ek in (1, 4):
        kw = dict(kw4, eval_kernel=ek)
        if ek == 1:
            kw["rhs"] = _capi.load_rhs_module(codegen.module_for(fd, D, NP)["so"])
        with _capi.Problem(B, D, N, Y, Lidx, 0.025, 4.0, RF0, P, Pidx, **kw) as pr:
            assert pr.info()["eval_kernel"] == ek
            ag = pr.action_grad(XP, 25.0)
            mn = pr.minimize_lbfgs(XP, 25.0, {'gtol': 1e-8, 'ftol': 1e-12, 'maxfun': 1000, 'maxiter': 20})
        res[ek] = (ag, mn)
    (A1, _, _, g1), m1 = res[1]
    (A4, _, _, g4), m4 = res[4]
    assert np.all(np.abs(A4 - A1) <= 1e-12 * np.abs(A1))
    assert np.abs(g4 - g1).max() <= 1e-12 * np.abs(g1).max()
    for k in ("nit", "nfev", "status"):
        assert list(m1[k]) == list(m4[k]), k
    assert np.all(np.abs(m4["A"] - m1["A"]) <= 1e-10 * np.abs(m1["A"]))


def test_anneal_past_the_old_cap():
    """the reference's own l96 with P0 of length D = 200 (a forcing per site, all estimated): a 5-rung anneal on
    k_eval5; every rung's A equals a fresh evaluation at the minimiser it returns, and lies below the action of the point
    the rung started from (the previous rung's minimiser) at this rung's RF"""
    D, N = 200, 400
    dt = 0.025
    rng = np.random.RandomState(12)
    Lidx = list(range(0, D, 2))
    x = np.empty((N, D))
    x[0] = 8.0 + rng.randn(D)
    forcing = 8.0 + 0.5 * rng.randn(D)
    for n in range(N - 1):                              # RK4 truth with the per-site forcing
        k1 = l96(0, x[n:n + 1], forcing)[0]
        k2 = l96(0, x[n:n + 1] + 0.5 * dt * k1, forcing)[0]
        k3 = l96(0, x[n:n + 1] + 0.5 * dt * k2, forcing)[0]
        k4 = l96(0, x[n:n + 1] + dt * k3, forcing)[0]
        x[n + 1] = x[n] + dt * (k1 + 2 * k2 + 2 * k3 + k4) / 6.0
    Y = x[:, Lidx] + 0.1 * rng.randn(N, len(Lidx))
    t = dt * np.arange(N)
    X0 = 10.0 * rng.rand(N, D) - 5.0
    P0 = np.full(D, 8.0)
    a = va_ode.Annealer()
    a.set_model(l96, D)
    a.set_data(Y, t=t)
    beta = np.arange(5)
    a.anneal(X0.copy(), P0.copy(), 2.0, beta, 4.0, 1e-2, Lidx, list(range(D)), disc="trapezoid",
             opt_args={'gtol': 1e-8, 'ftol': 1e-8, 'maxfun': 100000, 'maxiter': 200}, verbose=False)
    assert a._pb.info()["eval_kernel"] == 5
    ND = N * D
    for k in range(len(beta)):
        mp = a.minpaths[k]
        XP = np.append(mp[:ND], mp[ND:])[None, :]
        A, me, fe, g = a._pb.action_grad(XP, 2.0 ** beta[k])
        assert abs(A[0] - a.A_array[k]) <= 1e-12 * abs(A[0]), (k, A[0], a.A_array[k])
        if k > 0:
            A_start = a._pb.action_grad(a.minpaths[k - 1][None, :], 2.0 ** beta[k], want_grad=False)[0][0]
            assert a.A_array[k] < A_start, (k, a.A_array[k], A_start)
    assert np.any(a.minpaths[-1][ND:] != P0)                  # the forcing per site was estimated


def test_mixed_form_k_eval5():
    """D = 200, 402 parameters: two shared scalars (one estimated) and two interleaved vectors (some entries fixed) on the
    streaming kernel -- its shared-scalar path and a tail over more than one vector"""
    D, N = 200, 65
    NP = 2 + 2 * D
    rng = np.random.RandomState(14)
    P = np.concatenate([[1.0, 1.0], np.ravel(np.stack([8.0 + rng.rand(D), 0.8 + 0.4 * rng.rand(D)], 1))])
    Pidx = [0] + [2 + 2 * i for i in range(D) if i % 9 != 4] + [3 + 2 * i for i in range(0, D, 3)]
    _check_grad(mixed, D, N, NP, "trapezoid", P, Pidx, 5)


def test_refused_past_the_cap_with_the_reason():
    """200 parameters on a problem the column-parameter form cannot run (full RF matrices, box bounds): refused before
    anything is launched, as NotImplementedError naming the reason"""
    D, N = 200, 65
    P = 8.0 + np.random.RandomState(15).rand(D)
    Pidx = list(range(D))
    Lidx, Y, RF0, XP, kw = _problem(l96, D, N, D, 1, "trapezoid", P[None, :], Pidx)
    RFfull = np.tile(0.01 * np.eye(D), (N - 1, 1, 1))
    with pytest.raises(NotImplementedError, match="full RM / RF matrices"):
        _capi.Problem(1, D, N, Y, Lidx, 0.025, 4.0, RFfull, P[None, :], Pidx, **kw)
    bounds = [(-50.0, 50.0)] * (N * D + len(Pidx))
    with pytest.raises(NotImplementedError, match="box bounds"):
        _capi.Problem(1, D, N, Y, Lidx, 0.025, 4.0, RF0, P[None, :], Pidx, bounds=bounds, **kw)


@pytest.mark.parametrize("D,N", [(20, 61), (200, 65)])
def test_separate_tail_kernels(D, N):
    """with the tail NOT folded into the evaluation kernel (large grids: k_finalize_eval / k_ls run it) the evaluation and a
    short minimisation give what the folded tail gives (the row sums are added in another order: within 1e-12)"""
    B = 2
    P = 8.0 + np.random.RandomState(13).rand(B, D)
    Pidx = [i for i in range(D) if i % 5 != 1]
    Lidx, Y, RF0, XP, kw = _problem(l96, D, N, D, B, "trapezoid", P, Pidx)
    out = []
    for fold in (1, 0):
        with _capi.Problem(B, D, N, Y, Lidx, 0.025, 4.0, RF0, P, Pidx, **kw) as pr:
            pr.tune(fold=fold)
            A, me, fe, g = pr.action_grad(XP, 30.0)
            mn = pr.minimize_lbfgs(XP, 30.0, {'gtol': 1e-8, 'ftol': 1e-12, 'maxfun': 1000, 'maxiter': 10})
        out.append((A, g, mn))
    assert np.all(np.abs(out[0][0] - out[1][0]) <= 1e-12 * np.abs(out[0][0]))
    assert np.abs(out[0][1] - out[1][1]).max() <= 1e-12 * np.abs(out[0][1]).max()
    for k in ("nit", "nfev", "status"):
        assert np.array_equal(out[0][2][k], out[1][2][k]), k
    assert np.all(np.abs(out[0][2]["A"] - out[1][2]["A"]) <= 1e-10 * np.abs(out[0][2]["A"]))
