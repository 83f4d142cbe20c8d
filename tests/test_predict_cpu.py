"""CPU: the forecast (csrc/va_predict.h) without a GPU -- the integration rule and the kernel's lane / LDS mapping, run
lane by lane on the host by a g++ build of tests/cpu_emul/predict_check.cpp (the same header the kernel includes),
against an RK4 written in NumPy (tests/_predict_ref.py); the launch geometry of csrc/va_predict_geo.h; and what
va_ode.Annealer.predict / prediction_error hand to the device layer and make of its answer."""
import os
import subprocess

import numpy as np
import pytest

from _predict_ref import DT, K_TRUE, STEPS, TOL, l96_reference
from varanneal_amd import _capi, codegen, va_ode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("predict") / "predict_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "varanneal_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpu_emul", "predict_check.cpp")])
    return exe


def _host_run(exe, tmp_path, x0, ks, substeps, every):
    T, D = x0.shape
    f = tmp_path / "in.txt"
    f.write_text("\n".join("%.17g" % v for v in list(x0.ravel()) + list(ks)) + "\n")
    out = subprocess.run([exe, "traj", str(D), str(T), str(STEPS), str(substeps), str(every), repr(DT), str(f)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return np.array([float(v) for v in out.stdout.split()]).reshape(T, STEPS // every + 1, D)


@pytest.mark.parametrize("D", [5, 20, 67])
@pytest.mark.parametrize("substeps,every", [(1, 1), (2, 3)])
def test_host_path_matches_numpy_rk4(check_exe, tmp_path, D, substeps, every):
    """3 trajectories (D = 5, 20: side by side in one wave's image; D = 67: a workgroup each, lanes 67 .. 127 idle)"""
    T = 3
    x0, ref = l96_reference(D, T, substeps, every)
    got = _host_run(check_exe, tmp_path, x0, [K_TRUE] * T, substeps, every)
    assert got.shape == ref.shape and (every != 3 or got.shape[1] == 14)
    assert np.array_equal(got[:, 0], x0)                                   # row 0 is x0, bit for bit
    assert 5.0 < np.abs(ref).max() < 20.0
    err = np.abs(got - ref).max()
    print("D=%d substeps=%d every=%d  max |host C++ - NumPy| = %.3e" % (D, substeps, every, err))
    assert err <= TOL


def test_host_path_own_parameters(check_exe, tmp_path):
    """seven trajectories of D = 20 (three to a wave: the last wave holds one), each with its own forcing"""
    ks = [8.17, 7.5, 9.0, 8.0, 6.5, 10.0, 8.6]
    x0, ref = l96_reference(20, 7, ks=ks)
    got = _host_run(check_exe, tmp_path, x0, ks, 1, 1)
    assert np.abs(got - ref).max() <= TOL
    assert np.abs(ref[1] - ref[0]).max() > 1e-2                            # (the forcings matter)


def test_geometry(check_exe):
    widths = [1, 4, 5, 20, 33, 64, 65, 67, 200, 1024, 1025]
    out = subprocess.run([check_exe, "geo"] + [str(d) for d in widths], capture_output=True, text=True)
    assert out.returncode == 0
    lines = out.stdout.strip().splitlines()
    assert len(lines) == len(widths)
    for D, ln in zip(widths, lines):
        w = ln.split()
        assert int(w[1]) == D
        if D == 1025:
            assert w[0] == "NO" and "1024" in ln
            continue
        assert w[0] == "OK", ln
        RW, threads, E, wave, lds, grid = (int(v) for v in w[2:8])
        assert E * threads >= D and 1 <= E <= 4
        assert grid == (7 + RW - 1) // RW                                   # (the check plans T = 7)
        assert lds == 8 * (RW * (2 * D + 1))                                # two stage inputs and one parameter per trajectory
        if D <= 64:
            assert wave == 1 and threads == 64 and E == 1 and RW == 64 // D and RW * D <= 64
        else:
            assert wave == 0 and RW == 1 and threads == min(256, -(-D // 64) * 64) and threads % 64 == 0
            assert E == -(-D // threads)
    assert lines[3].split()[2:5] == ["3", "64", "1"] and lines[8].split()[2:5] == ["1", "256", "1"]
    assert lines[9].split()[2:5] == ["1", "256", "4"]


# ---------------------------------------------------------------------------------------------------------------
class _Recorder(object):
    """device stand-in: answers anneal() with recognisable minimising paths, records what predict() is handed"""
    made = []

    def __init__(self, batch, D, N_model, Y, Lidx, dt_model, RM, RF0, P, Pidx, **kw):
        self.B, self.D, self.N, self.NPest = batch, D, N_model, len(Pidx)
        self.P, self.kw = np.array(P), kw
        self.calls = []
        _Recorder.made.append(self)

    def close(self):
        pass

    def anneal(self, XP, rf_scale, opt_args=None, want_paths=False, **kw):
        B, nb = self.B, len(rf_scale)
        z = np.zeros((B, nb))
        tdp = self.kw.get("p_time_dependent")
        width = self.N * self.D + (self.N * self.NPest if tdp else self.P.shape[-1])
        mp = np.random.RandomState(7).randn(B, nb, width)
        return dict(x=None, A=z, me=z, fe=z, status=np.zeros((B, nb), np.int32), nit=np.zeros((B, nb), np.int32),
                    nfev=np.zeros((B, nb), np.int64), minpaths=mp, pest=np.zeros((B, nb, self.NPest)))

    def predict(self, x0, p, n_steps, t0=0.0, substeps=1, every=1, stim=None):
        x0 = np.array(x0)
        self.calls.append(dict(x0=x0, p=np.array(p), n_steps=n_steps, t0=t0, substeps=substeps, every=every, stim=stim))
        n_out = n_steps // every + 1
        # trajectory j, output row r, column i -> 100 j + r + i / 100
        return (100.0 * np.arange(x0.shape[0])[:, None, None] + np.arange(n_out)[None, :, None]
                + 0.01 * np.arange(self.D)[None, None, :])


def _l96(t, x, k):
    return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - x + k


def _annealed(monkeypatch, B, tdp=False):
    monkeypatch.setattr(_capi, "Problem", _Recorder)
    _Recorder.made = []
    D, N, nb = 20, 11, 3
    rng = np.random.RandomState(3)
    a = va_ode.Annealer()
    Lidx = list(range(0, D, 2))
    if tdp:
        from models.nakl import l96_damped_tdp
        monkeypatch.setattr(codegen, "module_for", lambda *ar, **kw: dict(so="/nonexistent/libva_rhs_test.so"))
        monkeypatch.setattr(_capi, "load_rhs_module", lambda path: 1000)
        a.set_model(l96_damped_tdp, D)
        P0 = 8.0 + rng.rand(N, 2) if B is None else 8.0 + rng.rand(B, N, 2)
        Pidx = [0]
    else:
        a.set_model(_l96, D)
        P0 = np.array([8.0]) if B is None else 8.0 + rng.rand(B, 1)
        Pidx = [0]
    a.set_data(rng.randn(N, len(Lidx)), t=0.5 + DT * np.arange(N))
    X0 = rng.randn(N, D) if B is None else rng.randn(B, N, D)
    a.anneal(X0, P0, 2.0, list(range(nb)), 4.0, 1e-2, Lidx, Pidx, disc="trapezoid", verbose=False)
    return a, _Recorder.made[-1], D, N, nb


def test_annealer_predict_plain_run(monkeypatch):
    a, dev, D, N, nb = _annealed(monkeypatch, None)
    out = a.predict(12, substeps=2, every=4)
    (c,) = dev.calls
    mp = a.minpaths
    assert mp.shape == (nb, N * D + 1)
    assert np.array_equal(c["x0"], mp[:, (N - 1) * D:N * D]) and np.array_equal(c["p"], mp[:, N * D:])
    assert c["t0"] == a.t_model[-1] == 0.5 + DT * (N - 1) and c["stim"] is None
    assert (c["n_steps"], c["substeps"], c["every"]) == (12, 2, 4)
    assert out.shape == (nb, 4, D) and out[2, 3, 5] == 200.0 + 3 + 0.05
    # a selection of rungs, one call
    out = a.predict(5, beta=[2, 0])
    assert len(dev.calls) == 2 and out.shape == (2, 6, D)
    assert np.array_equal(dev.calls[1]["x0"], mp[[2, 0], (N - 1) * D:N * D])
    assert a.predict(5, beta=1).shape == (1, 6, D)
    with pytest.raises(ValueError):
        a.predict(5, seeds=[0])
    with pytest.raises(IndexError):
        a.predict(5, beta=nb)


def test_annealer_predict_batch_and_selection(monkeypatch):
    B = 4
    a, dev, D, N, nb = _annealed(monkeypatch, B)
    mp = a.minpaths
    assert mp.shape == (B, nb, N * D + 1)
    out = a.predict(6)
    (c,) = dev.calls
    assert c["x0"].shape == (B * nb, D) and c["p"].shape == (B * nb, 1)
    assert np.array_equal(c["x0"].reshape(B, nb, D), mp[:, :, (N - 1) * D:N * D])
    assert np.array_equal(c["p"].reshape(B, nb, 1), mp[:, :, N * D:])
    assert out.shape == (B, nb, 7, D) and out[3, 1, 2, 0] == 100.0 * (3 * nb + 1) + 2     # seed-major, then rung
    out = a.predict(6, beta=[1, 2], seeds=[3, 0, 2])
    c = dev.calls[1]
    assert out.shape == (3, 2, 7, D) and len(dev.calls) == 2
    assert np.array_equal(c["x0"].reshape(3, 2, D), mp[[3, 0, 2]][:, [1, 2], (N - 1) * D:N * D])
    assert np.array_equal(c["p"].reshape(3, 2, 1), mp[[3, 0, 2]][:, [1, 2], N * D:])


@pytest.mark.parametrize("B", [None, 2])
def test_annealer_predict_time_dependent_parameters(monkeypatch, B):
    """the parameters of the LAST row of every rung's estimate"""
    a, dev, D, N, nb = _annealed(monkeypatch, B, tdp=True)
    NP = 2
    a.predict(3)
    (c,) = dev.calls
    mp = a.minpaths.reshape(-1, N * D + N * NP)
    assert np.array_equal(c["x0"], mp[:, (N - 1) * D:N * D])
    assert np.array_equal(c["p"], mp[:, N * D + (N - 1) * NP:])
    assert c["p"].shape == ((B or 1) * nb, NP)
    # column 0 is estimated (the recorder's path), column 1 is the caller's fixed value at the last time
    fixed = np.asarray(a.P).reshape(-1, N, NP)[:, -1, 1]
    assert np.array_equal(c["p"][:, 1].reshape(-1, nb), np.repeat(fixed[:, None], nb, axis=1))


def test_prediction_error_is_the_rms(monkeypatch):
    B = 2
    a, dev, D, N, nb = _annealed(monkeypatch, B)
    every, n_out = 2, 4
    Yf = np.random.RandomState(5).randn(n_out, len(a.Lidx))
    err = a.prediction_error(Yf, every=every, seeds=[1, 0])
    c = dev.calls[-1]
    assert (c["n_steps"], c["every"]) == ((n_out - 1) * every, every) and err.shape == (2, nb)
    pred = dev.predict(np.zeros((2 * nb, D)), None, 6, every=every).reshape(2, nb, n_out, D)      # (what the stand-in answers)
    for s in range(2):
        for k in range(nb):
            tot, cnt = 0.0, 0
            for r in range(1, n_out):
                for l, col in enumerate(a.Lidx):
                    tot += (pred[s, k, r, col] - Yf[r, l]) ** 2
                    cnt += 1
            assert abs(err[s, k] - np.sqrt(tot / cnt)) <= 1e-12 * err[s, k]
    # explicit n_steps, a plain run's shape
    a1, dev1, _, _, _ = _annealed(monkeypatch, None)
    assert a1.prediction_error(Yf, n_steps=6, every=every).shape == (nb,)
    with pytest.raises(ValueError):
        a1.prediction_error(Yf[:, :3])
