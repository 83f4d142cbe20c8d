"""CPU: Hessian-vector products of the action (csrc/va_hvp.h) without a GPU -- the kernel's phases run thread by thread on the
host by a g++ build of tests/cpu_emul/hvp_check.cpp (the same header the kernel includes) against a SymPy Hessian of the
oracle's action (tests/_hess_ref.py); the generated second-order model functions against SymPy derivatives; the launch
geometry of csrc/va_hvp_geo.h; and what va_ode.Annealer makes of the products (colouring, banded assembly, covariance)."""
import subprocess

import numpy as np
import pytest

import _hess_ref as hr
import _zoo_ref as zr
from _hvp_run import build_exe, fn_values, host_hv, sympy_second_order
from varanneal_amd import _capi, codegen, va_ode

L96_CASES = ([(d, "plain") for d in ("euler", "forwardmap", "trapezoid", "SimpsonHermite")]
             + [("trapezoid", "nskip"), ("SimpsonHermite", "rfarr")])


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return build_exe(str(tmp_path_factory.mktemp("hvp") / "hvp_check"))


@pytest.mark.parametrize("disc,variant", L96_CASES)
def test_host_phases_match_the_sympy_hessian(check_exe, tmp_path, disc, variant):
    """Lorenz-96, D = 5, N = 7 / 6, observed columns [0, 2], an estimated forcing; tile rows 2 and 3 (several tiles, a
    partial last tile, Simpson-Hermite halos -- 3: the odd tiles that stage extra rows) and one tile; full and
    Gauss-Newton.  Measured: 3e-16 .. 4e-15 (the SymPy Hessian itself is rounded)."""
    c = hr.l96_case(disc, variant)
    for gn, H in ((0, c["H"]), (1, c["Hgn"])):
        want = np.einsum("pij,pvj->pvi", H, c["V"])
        for tr in (0, 2, 3):
            got, (T, ntiles) = host_hv(check_exe, tmp_path, c, tile_rows=tr, gn=gn)
            assert (T, ntiles) == ((c["N"], 1) if tr == 0 else (tr, -(-c["N"] // tr)))
            err = hr.rel_err(got, want)
            print("%s %s gn=%d tile_rows=%d  max |Hv - H_ref v| / max |H_ref v| = %.2e" % (disc, variant, gn, tr, err))
            assert err <= hr.REL


def test_hessian_is_symmetric_and_gauss_newton_differs(check_exe, tmp_path):
    c = hr.l96_case("trapezoid", "plain")
    got, _ = host_hv(check_exe, tmp_path, c, tile_rows=3)
    V = c["V"]
    for p in range(V.shape[0]):
        uHv = np.dot(V[p], got[p].T)                        # [u, v] = u^T H v
        assert np.abs(uHv - uHv.T).max() <= 1e-12 * np.abs(uHv).max()
    # the model's second derivatives matter at these points: the two Hessians are different matrices
    assert np.abs(c["H"] - c["Hgn"]).max() > 1e-3 * np.abs(c["H"]).max()


def _generated_case(f, D, N, NP, Pidx, disc, seed, nstim=0):
    rng = np.random.RandomState(seed)
    Lidx = [0, 2]
    n = N * D + len(Pidx)
    P = 0.6 + 0.8 * rng.rand(NP)
    X = rng.randn(2, n)
    X[:, N * D:] = P[Pidx] + 0.1 * rng.rand(2, len(Pidx))
    c = dict(D=D, N=N, disc=disc, nskip=1, Lidx=Lidx, Pidx=Pidx, Y=rng.randn(N, 2), RM=2.0, RF0=0.7, P=P, X=X,
             V=rng.randn(2, 3, n), rf_scale=2.0, dt=hr.DT)
    return c


def test_gauss_newton_is_the_hessian_of_a_linear_model(tmp_path):
    D, N = 5, 6
    m = codegen.module_for(hr.linear_model, D, 1, compile=False, linear=False)
    exe = build_exe(str(tmp_path / "hvp_lin"), m["header"])
    c = _generated_case(hr.linear_model, D, N, 1, [0], "trapezoid", 4)
    sa = hr.SymbolicAction(hr.linear_model, D, N, c["Y"], c["Lidx"], c["dt"], c["RM"], c["RF0"] * c["rf_scale"], c["P"], c["Pidx"],
                           "trapezoid", gauss_newton=False)
    want = np.einsum("pij,pvj->pvi", np.array([sa.hessian(x) for x in c["X"]]), c["V"])
    full, _ = host_hv(exe, tmp_path, c, tile_rows=2, gn=0)
    gn, _ = host_hv(exe, tmp_path, c, tile_rows=2, gn=1)
    assert hr.rel_err(full, want) <= hr.REL and hr.rel_err(gn, want) <= hr.REL


def _nakl():
    from models.nakl import nakl
    return nakl


@pytest.mark.parametrize("name,D,NP,nstim,uniform", [("l96", 8, 1, 0, True), ("stencil", 8, 2, 0, True), ("nakl", 4, 18, 1, False),
                                                     ("l96_switch", 5, 1, 0, False)])
def test_generated_second_order_functions(tmp_path, name, D, NP, nstim, uniform):
    """the emitted jvp, vjp2 and pgrad2, compiled on the host, against SymPy Jacobians and Hessians of the traced model"""
    f = {"l96": hr.l96, "l96_switch": hr.l96, "stencil": hr.two_param_stencil, "nakl": _nakl()}[name.replace("()", "")]
    m = codegen.module_for(f, D, NP, nstim=nstim, compile=False, linear=False)
    assert ("switch (i)" not in m["text"]) == uniform
    for fn in ("jvp(", "vjp2(", "pgrad2("):
        assert fn in m["text"]
    exe = build_exe(str(tmp_path / "hvp_fn"), m["header"])
    rng = np.random.RandomState(5)
    nonzero = np.zeros(3)
    for _ in range(2):
        x, v, s = rng.rand(D) * 0.8 + 0.1, rng.randn(D), rng.randn(D)
        q, p = rng.randn(NP), rng.rand(NP) * 0.8 + 0.6
        t, st = 0.3, rng.randn(max(nstim, 1))
        got = fn_values(exe, tmp_path, D, NP, nstim, x, v, s, q, p, t, st)
        want = sympy_second_order(m["exprs"], D, NP, nstim, x, v, s, q, p, t, st)
        for k, (g, w) in enumerate(zip(got, want)):
            scale = np.abs(w).max()
            nonzero[k] = max(nonzero[k], scale)
            assert np.abs(g - w).max() <= 1e-10 * max(scale, 1e-300), (name, k)
    assert nonzero[0] > 0.1 and nonzero[1] > 0.1
    if name in ("stencil", "nakl"):
        assert nonzero[2] > 0.1                             # parameters that multiply states: pgrad2 is not empty


def _zoo_functions_error(tmp_path, name, npoints, tag="zoo"):
    """the emitted jvp / vjp2 / pgrad2 of a zoo model, compiled on the host, against torch autograd at points kept away from
    the thresholds: (module, worst error / (1e-10 max|want|) per function, largest |want| per function, switching arguments)"""
    m = zr.model(name)
    D, NP, nstim = m.D, m.NP, m.nstim
    mod = codegen.module_for(m.numpy, D, NP, nstim=nstim, compile=False, linear=False)
    exe = build_exe(str(tmp_path / ("hvp_" + tag)), mod["header"])
    t, x, p, st, sw = zr.safe_points(name, npoints, 41)
    assert t != 0.0 and (sw is None or np.abs(sw).min() >= zr.MARGIN_POINT)          # (a condition on the inputs)
    rng = np.random.RandomState(42)
    worst, nonzero = np.zeros(3), np.zeros(3)
    for r in range(npoints):
        v, s, q = rng.randn(D), rng.randn(D), rng.randn(NP)
        sr = st[r:r + 1] if nstim else np.zeros(1)
        got = fn_values(exe, tmp_path, D, NP, nstim, x[r], v, s, q, p, t, sr)
        want = m.torch_second_order(t, x[r], v, s, q, p, sr)
        for k, (g, w) in enumerate(zip(got, want)):
            scale = np.abs(w).max()
            nonzero[k] = max(nonzero[k], scale)
            worst[k] = max(worst[k], np.abs(g - w).max() / (1e-10 * max(scale, 1e-300)))
    return mod, worst, nonzero, sw


@pytest.mark.parametrize("name,uniform,npoints", [("kinked_small", False, 48), ("kinked_stencil", True, 48), ("timed_mix9", False, 4)])
def test_generated_second_order_functions_against_autograd(tmp_path, name, uniform, npoints):
    """the emitted jvp, vjp2 and pgrad2 of the zoo's kinked models (selects inside all three, which
    codegen.check_second_order leaves unchecked) and of a random model with a stimulus and explicit time, t = 2.3: `want`
    from torch autograd of the torch binding -- jvp, then the gradient of s . jvp in x and in p -- so that a printer or
    Piecewise slip shared with sympy_second_order cannot cancel.  Every switching argument is at least 1e-3 from its
    threshold, and every branch of every select of every component is taken by some point."""
    mod, worst, nonzero, sw = _zoo_functions_error(tmp_path, name, npoints)
    assert ("switch (i)" not in mod["text"]) == uniform
    for fn in ("jvp(", "vjp2(", "pgrad2("):
        assert fn in mod["text"]
    if sw is not None:
        assert "?" in mod["text"]                                                 # (the selects are printed as conditionals)
        assert np.all((sw > 0).any(axis=0)) and np.all((sw < 0).any(axis=0))
    print("%s: error / (1e-10 max|want|) jvp %.2e vjp2 %.2e pgrad2 %.2e" % ((name,) + tuple(worst)))
    assert np.all(worst <= 1.0), worst
    assert np.all(nonzero > 0.1)                                                  # (pgrad2 among them: parameters multiply states)


def test_a_generator_slip_on_the_kinked_stencil_does_not_pass(tmp_path):
    """the slip of test_module_time_check_covers_both_forms (the last uniform piece doubled) applied to kinked_stencil, which
    check_second_order does not look at: the autograd-referenced comparison above catches it"""
    real = codegen._uniform_second_order

    def slipped(exprs, syms, D, NP):
        fd0, dx, dp = real(exprs, syms, D, NP)
        return fd0, [(o, d) for o, d in dx[:-1]] + [(dx[-1][0], 2 * dx[-1][1])], dp
    codegen._uniform_second_order = slipped
    try:
        _, worst, _, _ = _zoo_functions_error(tmp_path, "kinked_stencil", 4, tag="slipped")
    finally:
        codegen._uniform_second_order = real
    assert worst[0] <= 1.0 and worst[1] > 1e6 and worst[2] <= 1.0


@pytest.mark.parametrize("disc", ["trapezoid", "SimpsonHermite"])
def test_kinked_model_through_the_phases(tmp_path, disc):
    """kinked_small (D = 6, the switch form, selects in jvp / vjp2 / pgrad2, sin(0.3 t)) through the kernel's phases on the
    host: N = 7, t_model = 1.7 + dt arange(N), two points with parameters of their own, both parameters estimated, one tile
    and tiles of 3 rows, full and Gauss-Newton, against tests/_hess_torch_ref.TorchAction of the torch binding"""
    m, c = zr.model("kinked_small"), zr.hvp_case("kinked_small", disc)
    mod = codegen.module_for(m.numpy, m.D, m.NP, compile=False, linear=False)
    exe = build_exe(str(tmp_path / "hvp_kinked"), mod["header"])
    assert c["margin"] >= zr.MARGIN_POINT and c["t_model"][0] == zr.T_HVP
    for gn, want in ((0, c["want"]), (1, c["want_gn"])):
        for tr in (0, 3):
            got, (T, ntiles) = host_hv(exe, tmp_path, c, tile_rows=tr, gn=gn)
            assert (T, ntiles) == ((7, 1) if tr == 0 else (3, 3))
            err = hr.rel_err(got, want)
            print("kinked_small %s gn=%d tile_rows=%d: %.2e" % (disc, gn, tr, err))
            assert err <= hr.REL


def test_generated_stencil_through_the_phases(tmp_path):
    """the two-parameter stencil (cross terms d2f/dxdp, a non-empty pgrad2), both parameters estimated, D = 8, N = 7"""
    D, N = 8, 7
    m = codegen.module_for(hr.two_param_stencil, D, 2, compile=False, linear=False)
    exe = build_exe(str(tmp_path / "hvp_st"), m["header"])
    c = _generated_case(hr.two_param_stencil, D, N, 2, [0, 1], "SimpsonHermite", 9)
    sa = hr.SymbolicAction(hr.two_param_stencil, D, N, c["Y"], c["Lidx"], c["dt"], c["RM"], c["RF0"] * c["rf_scale"], c["P"],
                           c["Pidx"], "SimpsonHermite", gauss_newton=False)
    want = np.einsum("pij,pvj->pvi", np.array([sa.hessian(x) for x in c["X"]]), c["V"])
    got, _ = host_hv(exe, tmp_path, c, tile_rows=3)
    err = hr.rel_err(got, want)
    print("stencil: %.2e" % err)
    assert err <= hr.REL


def test_geometry(check_exe):
    widths = [1, 5, 20, 64, 200, 512, 600, 683, 1138]
    for disc, halo in ((1, 2), (2, 3)):
        out = subprocess.run([check_exe, "geo", str(disc), "1"] + [str(d) for d in widths], capture_output=True, text=True)
        assert out.returncode == 0
        lines = out.stdout.strip().splitlines()
        assert len(lines) == len(widths)
        for D, ln in zip(widths, lines):
            w = ln.split()
            assert int(w[1]) == D
            # the smallest tile: one owned row and its halo; Simpson-Hermite: two rows (an odd tile stages three rows more),
            # of six images, and four partial rows, in 160 KiB
            maxD = (160 * 1024 // 8 - 4) // (6 * ((2 if disc == 2 else 1) + halo))
            assert maxD == (682 if disc == 2 else 1137)
            if D > maxD:
                assert w[0] == "NO" and int(w[2]) == maxD and "too wide" in ln
                continue
            assert w[0] == "OK", ln
            T, ntiles, Tmax, lds, grid = (int(v) for v in w[2:7])
            extra = 3 if (disc == 2 and T % 2) else 0
            assert lds == 8 * (6 * (T + halo + extra) * D + 4) and lds <= 160 * 1024
            assert ntiles == -(-161 // T) and grid == 61 * ntiles and 1 <= T <= Tmax <= 161
            assert T == min(Tmax, max(16, -(-1024 // D))) or (disc == 2 and T == min(Tmax, max(16, -(-1024 // D))) - 1)
            nxt = 3 if (disc == 2 and (Tmax + 1) % 2) else 0
            assert 8 * (6 * (Tmax + 1 + halo + nxt) * D + 4) > 160 * 1024 or Tmax == 161    # (Tmax is the most that fits)
            if D == 600:
                assert (T, Tmax) == ((2, 2) if disc == 2 else (3, 3))
        assert lines[2].split()[2:4] == ["52", "4"]                                        # the shipped example: 4 tiles of 52 rows


# ---------------------------------------------------------------------------------------------------------------
class _MatrixDevice(object):
    """device stand-in: anneal() answers with recognisable minimisers, hess_vec() multiplies by a known matrix"""
    made = []
    H = None

    def __init__(self, batch, D, N_model, Y, Lidx, dt_model, RM, RF0, P, Pidx, **kw):
        self.B, self.D, self.N, self.NPest, self.P = batch, D, N_model, len(Pidx), np.array(P)
        self.calls = []
        _MatrixDevice.made.append(self)

    def close(self):
        pass

    def anneal(self, XP, rf_scale, opt_args=None, want_paths=False, **kw):
        B, nb = self.B, len(rf_scale)
        z = np.zeros((B, nb))
        mp = np.random.RandomState(7).randn(B, nb, self.N * self.D + self.P.shape[-1])
        return dict(x=None, A=z, me=z, fe=z, status=np.zeros((B, nb), np.int32), nit=np.zeros((B, nb), np.int32),
                    nfev=np.zeros((B, nb), np.int64), minpaths=mp, pest=np.zeros((B, nb, self.NPest)))

    def hess_vec(self, XP, V, rf_scale, P=None, gauss_newton=False, tile_rows=0):
        self.calls.append(dict(XP=np.array(XP), V=np.array(V), rf=rf_scale, P=np.array(P), gn=gauss_newton))
        return np.einsum("ij,pvj->pvi", _MatrixDevice.H, V)


def _banded_spd(N, D, NPe, hb, rng, shift):
    """a random symmetric matrix whose path block couples time rows at most hb apart, with a dense parameter border"""
    ND = N * D
    n = ND + NPe
    H = np.zeros((n, n))
    for a in range(N):
        for b in range(a, min(N, a + hb + 1)):
            H[a * D:(a + 1) * D, b * D:(b + 1) * D] = rng.randn(D, D)
    H[:ND, ND:] = rng.randn(ND, NPe)
    H = np.triu(H) + np.triu(H, 1).T
    return H + shift * np.eye(n)


def _annealed(monkeypatch, disc, B=None, D=4, N=9, NPe=2):
    monkeypatch.setattr(_capi, "Problem", _MatrixDevice)
    monkeypatch.setattr(codegen, "module_for", lambda *ar, **kw: dict(so="/nonexistent/libva_rhs_test.so"))
    monkeypatch.setattr(_capi, "load_rhs_module", lambda path: 1000)
    _MatrixDevice.made = []
    rng = np.random.RandomState(3)
    a = va_ode.Annealer()
    a.set_model(lambda t, x, p: -p[0] * x + p[1] + p[2], D)
    a.set_data(rng.randn(N, 2), t=hr.DT * np.arange(N))
    X0 = rng.randn(N, D) if B is None else rng.randn(B, N, D)
    P0 = np.array([1.0, 2.0, 3.0]) if B is None else 1.0 + rng.rand(B, 3)
    a.anneal(X0, P0, 2.0, [0, 1, 2], 4.0, 1e-2, [0, 2], [0, 2][:NPe], disc=disc, verbose=False)
    return a, _MatrixDevice.made[-1]


@pytest.mark.parametrize("disc,hb", [("trapezoid", 1), ("SimpsonHermite", 2)])
def test_colouring_recovers_a_known_matrix_exactly(monkeypatch, disc, hb):
    D, N, NPe = 4, 9, 2
    rng = np.random.RandomState(hb)
    _MatrixDevice.H = H = _banded_spd(N, D, NPe, hb, rng, 0.0)
    a, dev = _annealed(monkeypatch, disc)
    got = a.action_hessian(beta=1, form='dense')
    (c,) = dev.calls
    assert c["V"].shape == (1, (2 * hb + 1) * D + NPe, N * D + NPe) and c["rf"] == 2.0 ** 1 and not c["gn"]
    mp = a.minpaths[1]
    assert np.array_equal(c["XP"][0], np.concatenate([mp[:N * D], mp[N * D:][[0, 2]]])) and np.array_equal(c["P"][0], mp[N * D:])
    # coloured direction c: ones at the path entries (n, j) with (n mod (2 hb + 1)) D + j == c
    for col in range((2 * hb + 1) * D):
        want = np.zeros(N * D + NPe)
        for n in range(N):
            for j in range(D):
                want[n * D + j] = float((n % (2 * hb + 1)) * D + j == col)
        assert np.array_equal(c["V"][0, col], want)
    assert np.array_equal(got, H)                                            # entries are copied, never summed: exact
    ab, H_xp, H_pp = a.action_hessian(beta=1, form='banded')
    u = (hb + 1) * D - 1
    assert ab.shape == (u + 1, N * D) and np.array_equal(H_xp, H[:N * D, N * D:]) and np.array_equal(H_pp, H[N * D:, N * D:])
    for i in range(N * D):
        for j in range(i, min(N * D, i + u + 1)):
            assert ab[u + i - j, j] == H[i, j]
    a.hess_vec(np.ones(N * D + NPe), gauss_newton=True)
    assert dev.calls[-1]["gn"] and dev.calls[-1]["rf"] == 2.0 ** 2              # default: the last rung


@pytest.mark.parametrize("disc,hb", [("trapezoid", 1), ("SimpsonHermite", 2)])
def test_param_covariance_is_the_inverse_block(monkeypatch, disc, hb):
    D, N, NPe = 4, 9, 2
    rng = np.random.RandomState(10 + hb)
    H = _banded_spd(N, D, NPe, hb, rng, 0.0)
    H += (1.0 - np.linalg.eigvalsh(H).min()) * np.eye(H.shape[0])            # positive definite
    _MatrixDevice.H = H
    a, dev = _annealed(monkeypatch, disc, B=2)
    cov = a.param_covariance()
    want = np.linalg.inv(H)[N * D:, N * D:]
    assert cov.shape == (2, NPe, NPe) and len(dev.calls) == 2
    err = np.abs(cov - want).max() / np.abs(want).max()
    print("covariance: %.2e at cond %.1e" % (err, np.linalg.cond(H)))
    assert err <= 1e-10 * np.linalg.cond(H)
    assert a.param_covariance(seeds=[1]).shape == (1, NPe, NPe)


def test_not_positive_definite_and_size_refusals(monkeypatch):
    D, N, NPe = 4, 9, 2
    H = _banded_spd(N, D, NPe, 1, np.random.RandomState(1), 0.0)            # indefinite
    _MatrixDevice.H = H
    a, dev = _annealed(monkeypatch, "trapezoid")
    with pytest.raises(np.linalg.LinAlgError, match="gauss_newton=True"):
        a.param_covariance()
    with pytest.raises(ValueError):
        a.action_hessian(form='sparse')
    # a positive definite path block under parameters the matrix says nothing about: the Schur complement is singular
    _MatrixDevice.H = np.diag(np.r_[np.ones(N * D), np.zeros(NPe)])
    with pytest.raises(np.linalg.LinAlgError, match="Schur"):
        a.param_covariance()
    ncalls = len(dev.calls)
    a.N_model = 100000                                                       # 400 002 variables: 1.2 TiB dense
    with pytest.raises(ValueError, match="2 GiB"):
        a.action_hessian(form='dense')
    assert len(dev.calls) == ncalls                                          # (refused before any device work)


def test_module_time_check_covers_both_forms():
    """codegen.check_second_order: which form it checked, that a wrong expression is caught, and what goes unchecked"""
    ex, sy = codegen.trace(hr.l96, 200, 1)
    assert codegen.check_second_order(ex, sy, 200, 1, 0) == "uniform"                 # wide states are checked too
    ex, sy = codegen.trace(hr.two_param_stencil, 8, 2)
    assert codegen.check_second_order(ex, sy, 8, 2, 0) == "uniform"
    ex5, sy5 = codegen.trace(hr.l96, 5, 1)
    assert codegen.check_second_order(ex5, sy5, 5, 1, 0) == "switch"
    exk, syk = codegen.trace(lambda t, x, p: -np.abs(x) * x + p[0], 5, 1)
    assert codegen.check_second_order(exk, syk, 5, 1, 0) is None                      # a kink: no complex step, unchecked
    # a generator slip (the uniform pieces' derivative taken in the wrong variable) does not pass
    real = codegen._uniform_second_order

    def slipped(exprs, syms, D, NP):
        fd0, dx, dp = real(exprs, syms, D, NP)
        return fd0, [(o, d) for o, d in dx[:-1]] + [(dx[-1][0], 2 * dx[-1][1])], dp
    codegen._uniform_second_order = slipped
    try:
        with pytest.raises(ValueError, match="vjp2"):
            codegen.check_second_order(ex, sy, 8, 2, 0)
    finally:
        codegen._uniform_second_order = real
