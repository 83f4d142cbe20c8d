"""CPU: the scalable Hessian reference (tests/_hess_torch_ref.py: the oracle's action on torch float64 tensors, differentiated
twice by autograd) against the SymPy Hessians of tests/_hess_ref.py at the sizes SymPy reaches, held to 1 % of the
derivative bound; then the host run of the kernel's phases (csrc/va_hvp.h hvp_host through tests/cpu_emul/hvp_check.cpp)
against that reference at the shapes tests/test_gpu_hvp_geometry.py runs on the device, held to the bound itself."""
import numpy as np
import pytest

import _hess_ref as hr
import _hess_torch_ref as tr
from _hvp_run import build_exe, host_hv
from varanneal_amd import codegen

REF_REL = 1e-12          # 1 % of hr.REL: the reference may not eat the bound it is used at

L96_CASES = ([(d, "plain") for d in ("euler", "forwardmap", "trapezoid", "SimpsonHermite")]
             + [("trapezoid", "nskip"), ("SimpsonHermite", "rfarr")])


@pytest.mark.parametrize("disc,variant", L96_CASES)
def test_reference_matches_sympy_on_the_l96_cases(disc, variant):
    """D = 5, N = 6 / 7, three points x four directions, full and Gauss-Newton.  Measured: 3.4e-16 .. 2.6e-15 (full),
    3.2e-16 .. 1.4e-15 (Gauss-Newton); the dense Hessian is symmetric to 1e-16 of its largest entry."""
    c = hr.l96_case(disc, variant)
    full, gn = tr.from_case(c).products(c["X"], c["V"])
    for name, got, H in (("full", full, c["H"]), ("gauss-newton", gn, c["Hgn"])):
        err = hr.rel_err(got, np.einsum("pij,pvj->pvi", H, c["V"]))
        print("%s %s %s: torch vs SymPy %.2e" % (disc, variant, name, err))
        assert err <= REF_REL
    ta = tr.from_case(c)
    H = ta.dense(c["X"][0])
    assert np.abs(H - H.T).max() <= 1e-14 * np.abs(H).max()
    assert np.abs(H - c["H"][0]).max() <= REF_REL * np.abs(c["H"][0]).max()


def _generated(f_sym, f_torch, D, N, NP, Pidx, disc, seed, stim=None, scale=1.0, gauss_newton=True):
    rng = np.random.RandomState(seed)
    n = N * D + len(Pidx)
    P = 0.6 + 0.8 * rng.rand(NP)
    X = scale * rng.randn(2, n)
    X[:, N * D:] = P[Pidx] + 0.1 * rng.rand(2, len(Pidx))
    c = dict(D=D, N=N, disc=disc, nskip=1, Lidx=[2, 0], Pidx=Pidx, Y=rng.randn(N, 2), RM=2.0, RF0=0.7, P=P, X=X, V=rng.randn(2, 3, n),
             rf_scale=2.0, dt=hr.DT, stim=stim)
    sa = hr.SymbolicAction(f_sym, D, N, c["Y"], c["Lidx"], c["dt"], c["RM"], c["RF0"] * c["rf_scale"], P, Pidx, disc, stim=stim,
                           gauss_newton=gauss_newton)
    full, gn = tr.from_case(c, f_torch).products(X, c["V"])
    err = hr.rel_err(full, np.einsum("pij,pvj->pvi", np.array([sa.hessian(x) for x in X]), c["V"]))
    egn = hr.rel_err(gn, np.einsum("pij,pvj->pvi", np.array([sa.gauss_newton(x) for x in X]), c["V"])) if gauss_newton else None
    return err, egn


def test_reference_matches_sympy_on_the_two_parameter_stencil():
    """D = 8, N = 7, Simpson-Hermite, both parameters estimated, observed columns given as [2, 0].
    Measured: 1.3e-15 (full), 5.7e-16 (Gauss-Newton)."""
    err, egn = _generated(hr.two_param_stencil, tr.two_param_stencil, 8, 7, 2, [0, 1], "SimpsonHermite", 9)
    print("stencil: torch vs SymPy %.2e (full) %.2e (gauss-newton)" % (err, egn))
    assert err <= REF_REL and egn <= REF_REL


def test_reference_matches_sympy_on_nakl():
    """D = 4, N = 9, trapezoid, a stimulus, 18 parameters of which three are estimated.  Measured: 8.3e-16."""
    N = 9
    stim = np.sin(0.7 * np.arange(N)) + 0.3
    err, _ = _generated(hr.nakl_sym, tr.nakl, 4, N, 18, [0, 6, 7], "trapezoid", 12, stim=stim, scale=0.3, gauss_newton=False)
    print("NaKL: torch vs SymPy %.2e" % err)
    assert err <= REF_REL


def test_reference_follows_the_call_s_own_parameters():
    """a point's fixed (not estimated) parameters change its Hessian: the reference takes them per call"""
    c = tr.geometry_case("nakl-n161")
    assert np.abs(c["P"][0] - c["P"][1]).min() > 0
    ta = tr.from_case(c, tr.nakl)
    a = ta.hv(c["X"][1], c["V"][1][:1], c["P"][1])
    other = ta.hv(c["X"][1], c["V"][1][:1], c["P"][0])
    assert np.array_equal(a, c["want"][1][:1]) and hr.rel_err(other, a) > 1e-3


# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return build_exe(str(tmp_path_factory.mktemp("hvp") / "hvp_check"))


def _host_case(exe, tmp_path, c):
    worst = 0.0
    for gn, want in ((0, c["want"]), (1, c["want_gn"])):
        assert np.abs(want).max(axis=-1).min() > 0                       # (no direction whose product is all zero)
        for tile_rows, plan in c["plan"].items():
            got, geo = host_hv(exe, tmp_path, c, tile_rows=tile_rows, gn=gn)
            assert geo == plan, (tile_rows, geo)
            err = hr.rel_err(got, want)
            print("%s gn=%d tile_rows=%d (T, ntiles)=%s  max |Hv - H_ref v| / max |H_ref v| = %.2e" % (c["name"], gn, tile_rows, geo, err))
            assert err <= hr.REL
            worst = max(worst, err)
    return worst


@pytest.mark.parametrize("name", tr.L96_GEOMETRY)
def test_host_phases_at_the_device_shapes(check_exe, tmp_path, name):
    """the built-in Lorenz-96 cases of tests/test_gpu_hvp_geometry.py through hvp_host, every tiling of each, full and
    Gauss-Newton, at REL against the torch reference; (T, ntiles) of plan_hvp as the case records them.
    Measured: 1.2e-16 .. 5.9e-15 over all cases (6e-5 of REL)."""
    _host_case(check_exe, tmp_path, tr.geometry_case(name))


@pytest.mark.parametrize("name,f,NP,nstim", [("stencil-d20", hr.two_param_stencil, 2, 0), ("nakl-n161", "nakl", 18, 1)])
def test_host_phases_of_the_generated_models(tmp_path, name, f, NP, nstim):
    """the generated two-parameter stencil (D = 20, N = 21, Simpson-Hermite, tiles of 21 and 5 rows) and NaKL (D = 4,
    N = 161, 3 of 18 parameters estimated, every point its own fixed parameters, tiles of 161 and 50 rows): pgrad2 and the
    tiles' shares of the parameter rows.  Measured: 3.4e-16 .. 5.8e-16 (stencil), 1.2e-15 .. 6.1e-15 (NaKL)."""
    if f == "nakl":
        from models.nakl import nakl as f
    c = tr.geometry_case(name)
    m = codegen.module_for(f, c["D"], NP, nstim=nstim, compile=False, linear=False)
    exe = build_exe(str(tmp_path / "hvp_gen"), m["header"])
    _host_case(exe, tmp_path, c)
