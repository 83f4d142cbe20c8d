"""CPU: the forecast spread (csrc/va_predict_tlm.h) without a GPU -- the tangent-linear RK4 rule, the kernel's element /
LDS mapping and the reduction over directions, run lane by lane on the host by a g++ build of
tests/cpu_emul/predict_tlm_check.cpp (the same header the kernels include), against the tangent-linear RK4 written in NumPy
(tests/_tlm_ref.py, where the tolerance is derived); the launch geometry of csrc/va_predict_tlm_geo.h; and what
va_ode.Annealer.predict_spread hands to the device layer and makes of its answer."""
import os
import subprocess

import numpy as np
import pytest

import _tlm_ref
from _predict_ref import DT, K_TRUE, STEPS
from _predict_ref import TOL as TOL_X
from _tlm_ref import TOL, l96_tlm_reference, ordered_sums, row_error
from varanneal_amd import _capi, codegen, va_ode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("predict_tlm") / "predict_tlm_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "varanneal_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpu_emul", "predict_tlm_check.cpp")])
    return exe


def _host_run(exe, tmp_path, x0, ks, V0, substeps, every):
    T, D = x0.shape
    nvec = V0.shape[1]
    f, o = tmp_path / "in.txt", tmp_path / "out.bin"
    f.write_text("\n".join("%.17g" % v for v in list(x0.ravel()) + list(ks) + list(V0.ravel())) + "\n")
    run = subprocess.run([exe, "traj", str(D), str(T), str(nvec), str(STEPS), str(substeps), str(every), repr(DT), str(f), str(o)],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    n_out = STEPS // every + 1
    raw = np.fromfile(str(o))
    sizes = [T * n_out * D, T * nvec * n_out * D, T * n_out * D, T * n_out * D * D]
    assert raw.size == sum(sizes)
    out, dX, var, cov = np.split(raw, np.cumsum(sizes)[:-1])
    return (out.reshape(T, n_out, D), dX.reshape(T, nvec, n_out, D), var.reshape(T, n_out, D), cov.reshape(T, n_out, D, D),
            [int(v) for v in run.stdout.split()])


def test_reference_agrees_with_the_complex_step_of_rk4():
    worst = _tlm_ref.self_check()
    print("tangent-linear NumPy reference against the complex step of _predict_ref.rk4: %.3e relative per row" % worst)
    assert worst <= 1e-13


@pytest.mark.parametrize("D", [5, 20, 67])
@pytest.mark.parametrize("substeps,every", [(1, 1), (2, 3)])
@pytest.mark.parametrize("full", [True, False])
def test_host_path_matches_numpy_tlm(check_exe, tmp_path, D, substeps, every, full):
    """3 trajectories; nvec = D + 1 (an identity on the states plus the forcing: D = 5 the nominal and all 6 directions in
    one wave, D = 20 a wave of 3 slots and 11 chunks, the last one half full, D = 67 five workgroups of 256 lanes x 4
    elements per trajectory, idle lanes and slots), and nvec = 1 (a mixed direction; D = 5: six trajectories to a wave)"""
    T = 3
    V = None if full else np.random.RandomState(D).randn(1, D + 1)
    x0, V0, ref_x, ref_dx = l96_tlm_reference(D, T, substeps, every, V=V)
    out, dX, var, cov, geo = _host_run(check_exe, tmp_path, x0, [K_TRUE] * T, V0, substeps, every)
    n_out = 14 if every == 3 else STEPS + 1
    assert dX.shape == ref_dx.shape == (T, D + 1 if full else 1, n_out, D)
    assert np.array_equal(out[:, 0], x0) and np.array_equal(dX[:, :, 0], V0[:, :, :D])     # row 0, bit for bit
    ex, ed = np.abs(out - ref_x).max(), row_error(dX, ref_dx)
    print("D=%d nvec=%d substeps=%d every=%d geometry %s: nominal |host C++ - NumPy| = %.3e, tangents relative per row = %.3e"
          % (D, dX.shape[1], substeps, every, geo, ex, ed))
    assert ex <= TOL_X
    assert ed <= TOL
    assert np.abs(ref_dx[:, :, -1]).max() > 2.0 * np.abs(ref_dx[:, :, 0]).max()            # (the tangents do grow)
    v, c = ordered_sums(dX)
    assert np.array_equal(var, v) and np.array_equal(cov, c)
    assert np.array_equal(cov, cov.transpose(0, 1, 3, 2))


def test_host_path_own_forcings(check_exe, tmp_path):
    """seven trajectories of D = 20, each with its own forcing; 5 directions: 2 slots beside the nominal, the last chunk
    half full"""
    ks = [8.17, 7.5, 9.0, 8.0, 6.5, 10.0, 8.6]
    V = np.random.RandomState(9).randn(5, 21)
    x0, V0, ref_x, ref_dx = l96_tlm_reference(20, 7, ks=ks, V=V)
    out, dX, _, _, geo = _host_run(check_exe, tmp_path, x0, ks, V0, 1, 1)
    assert geo[:3] == [1, 2, 3]
    assert np.abs(out - ref_x).max() <= TOL_X and row_error(dX, ref_dx) <= TOL
    assert row_error(ref_dx[1], ref_dx[0]) > 1e-2                                           # (the forcings matter)


NVECS = [1, 2, 21, 65, 96]


@pytest.mark.parametrize("nvec", NVECS)
def test_geometry(check_exe, nvec):
    """widths 1 .. 1025, planned for T = 3 (a part-filled or a lone workgroup wherever trajectories share one) and one parameter: the check program runs the kernel's own load phase on every
    lane of every workgroup and counts"""
    out = subprocess.run([check_exe, "geo", str(nvec), "1", "1025"], capture_output=True, text=True)
    assert out.returncode == 0
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 1025
    for D, ln in zip(range(1, 1026), lines):
        w = ln.split()
        assert int(w[1]) == D
        if D == 1025:
            assert w[0] == "NO" and "1024" in ln                      # k_predict's limit, with the reason
            continue
        assert w[0] == "OK", ln
        RW, chunk, nchunks, threads, E, wave, lds, grid = (int(v) for v in w[2:10])
        # every (trajectory, direction, column) and every nominal output column has exactly one lane; every workgroup
        # carries the nominal of its trajectories once
        assert w[10:15] == ["1"] * 5, ln
        assert chunk >= 1 and chunk * nchunks >= nvec > chunk * (nchunks - 1)
        assert grid == -(-3 // RW) * nchunks
        assert lds == 8 * RW * (chunk + 1) * (2 * D + 1) and lds <= 64 * 1024
        assert E * threads >= RW * (chunk + 1) * D
        if 2 * D <= 64:
            assert wave == 1 and threads == 64 and E == 1 and RW * (chunk + 1) * D <= 64
            assert (RW == 64 // ((nvec + 1) * D) and chunk == nvec) if (nvec + 1) * D <= 64 else (RW == 1 and chunk <= 64 // D - 1)
        else:
            assert wave == 0 and RW == 1 and threads % 64 == 0 and threads == min(256, -(-(chunk + 1) * D // 64) * 64)
            assert E == -(-(chunk + 1) * D // threads)
            assert E <= 4 if D <= 512 else (chunk == 1 and 5 <= E <= 8)
    if nvec == 21:
        assert lines[4].split()[2:8] == ["1", "11", "2", "64", "1", "1"]       # D = 5: 12 slots to the wave
        assert lines[19].split()[2:8] == ["1", "2", "11", "64", "1", "1"]      # D = 20: nominal and two directions
        assert lines[66].split()[2:8] == ["1", "11", "2", "256", "4", "0"]     # D = 67
    if nvec == 2:
        assert lines[4].split()[2:8] == ["4", "2", "1", "64", "1", "1"]        # D = 5: four trajectories side by side


# ---------------------------------------------------------------------------------------------------------------
class _Recorder(object):
    """device stand-in: answers anneal() with recognisable minimising paths, laplace() with a known covariance per point
    (point 1 not positive definite in the Hessian, point 2 with a covariance whose Cholesky fails), and records what
    predict_tangent() is handed"""
    made = []

    def __init__(self, batch, D, N_model, Y, Lidx, dt_model, RM, RF0, P, Pidx, **kw):
        self.B, self.D, self.N, self.NPest = batch, D, N_model, len(Pidx)
        self.P, self.kw = np.array(P), kw
        self.calls, self.laplace_calls = [], []
        _Recorder.made.append(self)

    def close(self):
        pass

    def anneal(self, XP, rf_scale, opt_args=None, want_paths=False, **kw):
        B, nb = self.B, len(rf_scale)
        z = np.zeros((B, nb))
        tdp = self.kw.get("p_time_dependent")
        mp = np.random.RandomState(7).randn(B, nb, self.N * self.D + (self.N * self.NPest if tdp else self.P.shape[-1]))
        return dict(x=None, A=z, me=z, fe=z, status=np.zeros((B, nb), np.int32), nit=np.zeros((B, nb), np.int32),
                    nfev=np.zeros((B, nb), np.int64), minpaths=mp, pest=np.zeros((B, nb, self.NPest)))

    def sigma0(self, j):
        """the joint covariance of (x_{N-1}, p_est) the stand-in gives point j"""
        n = self.D + self.NPest
        A = np.random.RandomState(50 + j).randn(n, n)
        return np.dot(A, A.T) / n + 0.5 * np.eye(n)

    def laplace(self, XP, rf_scale, P=None, gauss_newton=False, full=False, chunk_pts=0):
        npts, N, D, NPe = len(XP), self.N, self.D, self.NPest
        self.laplace_calls.append(dict(XP=np.array(XP), rf=np.array(rf_scale), P=np.array(P), gauss_newton=gauss_newton, full=full))
        rng = np.random.RandomState(11)
        r = dict(var_x=rng.rand(npts, N, D), cov_xx=rng.randn(npts, N, D, D), cov_px=rng.randn(npts, NPe, N * D),
                 cov_pp=rng.randn(npts, NPe, NPe), logdet=np.zeros(npts), status=np.zeros(npts, np.int32))
        for j in range(npts):
            S = self.sigma0(j)
            r["cov_xx"][j, N - 1] = S[:D, :D]
            r["cov_px"][j].reshape(NPe, N, D)[:, N - 1] = S[D:, :D]
            r["cov_pp"][j] = S[D:, D:]
            r["var_x"][j, N - 1] = np.diag(S)[:D]
        if npts > 1:                                                   # the Hessian stopped being positive definite
            for k in ("var_x", "cov_xx", "cov_px", "cov_pp"):
                r[k][1] = np.nan
            r["status"][1] = 4
        if npts > 2:                                                   # laplace succeeded, but its last block is indefinite
            r["cov_xx"][2, N - 1, 0, 0] = -1.0
        return r

    def predict_tangent(self, x0, p, V0, n_steps, t0=0.0, substeps=1, every=1, stim=None, want=("dx", "var")):
        x0, V0 = np.array(x0), np.array(V0)
        self.calls.append(dict(x0=x0, p=np.array(p), V0=V0, n_steps=n_steps, t0=t0, substeps=substeps, every=every, stim=stim,
                               want=tuple(want)))
        T, n_out, D = x0.shape[0], n_steps // every + 1, self.D
        # trajectory j, output row r, column i -> 100 j + r + i / 100
        out = 100.0 * np.arange(T)[:, None, None] + np.arange(n_out)[None, :, None] + 0.01 * np.arange(D)[None, None, :]
        r = dict(out=out)
        # the spread stays what the directions say at row 0: var = diag(V V^T), cov = V V^T, at every row
        Vx = V0[:, :, :D]
        if "var" in want:
            r["var"] = np.repeat(np.einsum("tci,tci->ti", Vx, Vx)[:, None, :], n_out, axis=1)
        if "cov" in want:
            r["cov"] = np.repeat(np.einsum("tci,tcj->tij", Vx, Vx)[:, None], n_out, axis=1)
        return r


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
    else:
        a.set_model(_l96, D)
        P0 = np.array([8.0]) if B is None else 8.0 + rng.rand(B, 1)
    a.set_data(rng.randn(N, len(Lidx)), t=0.5 + DT * np.arange(N))
    X0 = rng.randn(N, D) if B is None else rng.randn(B, N, D)
    a.anneal(X0, P0, 2.0, list(range(nb)), 4.0, 1e-2, Lidx, [0], disc="trapezoid", verbose=False)
    return a, _Recorder.made[-1], D, N, nb


def test_annealer_predict_spread_plain_run(monkeypatch):
    a, dev, D, N, nb = _annealed(monkeypatch, None)
    r = a.predict_spread(12, substeps=2, every=4, gauss_newton=True)
    (lc,), (c,) = dev.laplace_calls, dev.calls
    mp = a.minpaths
    # one laplace(full=True) call at the selected minimisers, each with its own rung's RF
    assert lc["full"] is True and lc["gauss_newton"] is True and lc["XP"].shape == (nb, N * D + 1)
    assert np.array_equal(lc["XP"][:, :N * D], mp[:, :N * D]) and np.array_equal(lc["rf"], a._rf_scale)
    # one predict_tangent call: the last fitted states, the full parameter vectors, t0, and the Cholesky factor of the last
    # row's blocks as directions
    assert np.array_equal(c["x0"], mp[:, (N - 1) * D:N * D]) and np.array_equal(c["p"], mp[:, N * D:])
    assert c["t0"] == a.t_model[-1] == 0.5 + DT * (N - 1) and c["stim"] is None
    assert (c["n_steps"], c["substeps"], c["every"]) == (12, 2, 4) and c["want"] == ("var",)
    assert c["V0"].shape == (nb, D + 1, D + 1)
    for j in (0, 2):
        S = dev.sigma0(j)
        if j == 2:
            S[0, 0] = -1.0
            assert np.array_equal(c["V0"][j], np.zeros((D + 1, D + 1)))          # (nothing to propagate)
            continue
        # direction c is column c of the lower Cholesky factor: V0[c] = L[:, c]
        assert np.array_equal(c["V0"][j].T, np.linalg.cholesky(S))
        assert np.abs(np.dot(c["V0"][j].T, c["V0"][j]) - S).max() <= 1e-14 * np.abs(S).max()
    assert set(r) == {"mean", "std", "status"}
    assert r["mean"].shape == r["std"].shape == (nb, 4, D) and r["status"].shape == (nb,)
    assert r["mean"][2, 3, 5] == 200.0 + 3 + 0.05
    # the NaN / status convention: laplace's status where the Hessian failed, -2 where Sigma_0 has no Cholesky factor
    assert list(r["status"]) == [0, 4, -2]
    assert np.all(np.isnan(r["std"][1:])) and np.all(np.isfinite(r["mean"]))
    assert np.abs(r["std"][0] ** 2 - np.diag(dev.sigma0(0))[:D]).max() <= 1e-14


def test_annealer_predict_spread_batch_selection_and_full(monkeypatch):
    B = 4
    a, dev, D, N, nb = _annealed(monkeypatch, B)
    mp = a.minpaths
    r = a.predict_spread(6, beta=[1, 2], seeds=[3, 0, 2], full=True)
    (lc,), (c,) = dev.laplace_calls, dev.calls
    assert c["want"] == ("var", "cov")
    assert np.array_equal(c["x0"].reshape(3, 2, D), mp[[3, 0, 2]][:, [1, 2], (N - 1) * D:N * D])
    assert np.array_equal(c["p"].reshape(3, 2, 1), mp[[3, 0, 2]][:, [1, 2], N * D:])
    assert np.array_equal(lc["rf"], np.tile(np.asarray(a._rf_scale)[[1, 2]], 3))
    assert set(r) == {"mean", "std", "status", "cov"}
    assert r["mean"].shape == r["std"].shape == (3, 2, 7, D) and r["cov"].shape == (3, 2, 7, D, D) and r["status"].shape == (3, 2)
    assert r["mean"][2, 1, 2, 0] == 100.0 * (2 * 2 + 1) + 2                                  # seed-major, then rung
    assert list(r["status"].ravel()) == [0, 4, -2, 0, 0, 0]
    assert np.all(np.isnan(r["cov"][0, 1])) and np.all(np.isnan(r["cov"][1, 0])) and np.all(np.isnan(r["std"][0, 1]))
    S = dev.sigma0(4)
    assert np.abs(r["cov"][2, 0, 3] - S[:D, :D]).max() <= 1e-14 * np.abs(S).max()
    assert np.all(np.isfinite(r["mean"]))


def test_annealer_predict_spread_refusals(monkeypatch):
    a, dev, D, N, nb = _annealed(monkeypatch, None)
    with pytest.raises(ValueError):
        a.predict_spread(5, seeds=[0])                 # not a batch
    with pytest.raises(IndexError):
        a.predict_spread(5, beta=nb)
    assert not dev.calls and not dev.laplace_calls
    with pytest.raises(ValueError, match="anneal"):
        va_ode.Annealer().predict_spread(5)
    at, devt, _, _, _ = _annealed(monkeypatch, None, tdp=True)
    with pytest.raises(NotImplementedError, match="time-dependent"):
        at.predict_spread(5)
    assert not devt.calls and not devt.laplace_calls
