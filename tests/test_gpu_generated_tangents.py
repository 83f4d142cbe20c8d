"""GPU: generated models' f / jvp / vjp2 / pgrad2 on the device -- every model of the zoo (tests/models/zoo.py: kinked models in
the switch and the one-body form, random mixed models with a stimulus and explicit time, the sin(t)-forced Lorenz-96 at D = 20
and 67, the column-parameter Lorenz-96) through hess_vec (k_hvp), predict (k_predict), predict_tangent (k_predict_tlm) and
lyapunov (k_lyap), with t_model / t0 away from 0.  References, inputs, the conditions on the inputs and the derived tolerances:
tests/_zoo_ref.py (held together on the CPU by tests/test_zoo_cpu.py).  T = 7 trajectories, 40 steps."""
import numpy as np
import pytest

import _hess_ref as hr
import _zoo_ref as zr
from _tlm_ref import row_error
from varanneal_amd import _capi, codegen

pytestmark = pytest.mark.gpu

T = zr.T
WITH_LYAP = [n for n in zr.NAMES if zr.model(n).D <= 64]


@pytest.fixture(scope="module")
def rhs():
    """name -> id of the model's module, generated and compiled once"""
    made = {}

    def get(name):
        if name not in made:
            m = zr.model(name)
            kw = {}
            if m.colparams:           # as tests/test_gpu_predict.py: column-parameter form, which still has its flat struct
                Lidx = list(range(0, m.D, 2))
                kw = dict(colparams=True, col_variant=lambda ne, gh, reach=None: _capi.eval_plan(1, m.D, 61, "trapezoid", ne, gh,
                                                                                                 reach=reach, Lidx=Lidx))
            mod = codegen.module_for(m.numpy, m.D, m.NP, nstim=m.nstim, stim_ndim=1, **kw)
            assert (mod["colp"] is not None) == m.colparams
            if name in ("kinked_small", "kinked_stencil"):
                assert ("switch (i)" not in mod["text"]) == (name == "kinked_stencil") and "?" in mod["text"]
            made[name] = _capi.load_rhs_module(mod["so"])
        return made[name]
    return get


def _traj_handle(name, rid):
    """a small problem of the model: the trajectory calls take the model, D, NP, Pidx, dt_model and the stream from it"""
    m, c = zr.model(name), zr.traj_case(name)
    Nh = 5
    return _capi.Problem(1, m.D, Nh, np.zeros((Nh, 2)), [0, 2], c["dt"], 1.0, 1.0, c["P"][:1].copy(), c["Pidx"], rhs=rid,
                         t_model=c["dt"] * np.arange(Nh), stim=np.zeros(Nh) if m.nstim else None)


def _inputs_are_fit(name, substeps, every):
    """the conditions on a kinked model's inputs, on the reference alone: its margin from every threshold, a branch change in
    every trajectory"""
    _, kinks = zr.predict_reference(name, substeps, every)
    if kinks is not None:
        assert kinks.margin >= zr.MARGIN and all(kinks.crossed())


@pytest.mark.parametrize("name", zr.NAMES)
def test_hess_vec(rhs, name):
    """N = 7 (9 at D = 67), t_model from 1.7, two points with parameters of their own, two random directions and the unit
    vector of every estimated parameter (all 20 forcings of l96_colparams); one tile and tiles of 3 rows, trapezoid and
    Simpson-Hermite, full and Gauss-Newton, against torch autograd of the torch binding; action_grad's bits before and after"""
    m = zr.model(name)
    for disc in ("trapezoid", "SimpsonHermite"):
        c = zr.hvp_case(name, disc)
        assert c["t_model"][0] == zr.T_HVP and (not m.kinked or c["margin"] >= zr.MARGIN_POINT)
        with _capi.Problem(2, c["D"], c["N"], c["Y"], c["Lidx"], c["dt"], c["RM"], c["RF0"], c["P"].copy(), c["Pidx"], disc=disc,
                           rhs=rhs(name), t_model=c["t_model"], stim=c["stim"]) as pb:
            before = pb.action_grad(c["X"], c["rf_scale"])
            for gn, want in ((False, c["want"]), (True, c["want_gn"])):
                for tr in (0, 3):
                    got = pb.hess_vec(c["X"], c["V"], c["rf_scale"], P=c["P"], gauss_newton=gn, tile_rows=tr)
                    err = hr.rel_err(got, want)
                    print("%s hess_vec %s gn=%d tile_rows=%d  max |Hv - H_ref v| / max |H_ref v| = %.2e  (bound %.1e)"
                          % (name, disc, gn, tr, err, hr.REL))
                    assert err <= hr.REL
            after = pb.action_grad(c["X"], c["rf_scale"])
        for a, b in zip(before, after):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("name", zr.NAMES)
def test_predict(rhs, name):
    c, tol = zr.traj_case(name), zr.TOL[name]["x"]
    with _traj_handle(name, rhs(name)) as pb:
        for substeps, every in zr.PAIRS_TLM:
            _inputs_are_fit(name, substeps, every)
            ref, _ = zr.predict_reference(name, substeps, every)
            got = pb.predict(c["x0"], c["P"], c["steps"], t0=c["t0"], substeps=substeps, every=every, stim=c["stim"])
            assert got.shape == ref.shape and np.array_equal(got[:, 0], c["x0"])
            err = np.abs(got - ref).max()
            print("%s predict substeps=%d every=%d  max |device - NumPy| = %.3e  (bound %.1e, largest state %.3g)"
                  % (name, substeps, every, err, tol, np.abs(ref).max()))
            assert err <= tol


@pytest.mark.parametrize("name", zr.NAMES)
def test_predict_tangent(rhs, name):
    """directions I_(D + NPe) (a few at D = 67), every trajectory the same; the nominal against predict()'s reference"""
    c, tol = zr.traj_case(name), zr.TOL[name]
    V0 = np.ascontiguousarray(np.broadcast_to(c["V"], (T,) + c["V"].shape))
    with _traj_handle(name, rhs(name)) as pb:
        for substeps, every in zr.PAIRS_TLM:
            _inputs_are_fit(name, substeps, every)
            out, dX = zr.tangent_reference(name, substeps, every)
            r = pb.predict_tangent(c["x0"], c["P"], V0, c["steps"], t0=c["t0"], substeps=substeps, every=every, stim=c["stim"],
                                   want=("dx",))
            assert r["dx"].shape == dX.shape and np.array_equal(r["dx"][:, :, 0], V0[:, :, :c["D"]])
            ex, ed = np.abs(r["out"] - out).max(), row_error(r["dx"], dX)
            print("%s predict_tangent substeps=%d every=%d  nominal |device - NumPy| = %.3e (bound %.1e), tangents relative per row = %.3e "
                  "(bound %.1e, largest tangent entry %.3g)" % (name, substeps, every, ex, tol["x"], ed, tol["tlm"], np.abs(dX).max()))
            assert ex <= tol["x"] and ed <= tol["tlm"]


@pytest.mark.parametrize("name", WITH_LYAP)
def test_lyapunov(rhs, name):
    """K = D for the small models, K = 3 and 20 at D = 20, both (substeps, qr_every) pairs, the largest K once more with gain
    5 on every second column; x_end against the reference and against predict()'s last row (each within the states' bound
    of the reference, so within twice that of each other)"""
    c, tol = zr.traj_case(name), zr.TOL[name]
    D = c["D"]
    with _traj_handle(name, rhs(name)) as pb:
        for K, substeps, qr_every, gain in zr.lyap_cases(name):
            _inputs_are_fit(name, substeps, qr_every)
            ref = zr.lyap_reference(name, K, substeps, qr_every, gain)
            g = np.ascontiguousarray(np.broadcast_to(zr.gain_every_second(D), (T, D))) if gain else None
            r = pb.lyapunov(c["x0"], c["P"], K, c["steps"], t0=c["t0"], substeps=substeps, qr_every=qr_every, coupling=g, stim=c["stim"],
                            trace=True)
            plain = pb.predict(c["x0"], c["P"], c["steps"], t0=c["t0"], substeps=substeps, every=c["steps"], stim=c["stim"])
            el, eq, et = (np.abs(r[key] - ref[key]).max() for key in ("logsum", "Q_end", "trace"))
            ex, ep = np.abs(r["x_end"] - ref["x_end"]).max(), np.abs(r["x_end"] - plain[:, -1]).max()
            print("%s lyapunov K=%d substeps=%d qr_every=%d gain=%s: |device - NumPy| logsum %.3e  Q_end %.3e  trace %.3e (bound %.1e); "
                  "x_end %.3e, |x_end - predict()| = %.3e (bound %.1e)" % (name, K, substeps, qr_every, gain, el, eq, et, tol["lyap"], ex, ep,
                                                                          tol["x"]))
            assert not r["status"].any() and not ref["status"].any()
            assert el <= tol["lyap"] and eq <= tol["lyap"] and et <= tol["lyap"]
            assert ex <= tol["x"] and ep <= 2.0 * tol["x"]
