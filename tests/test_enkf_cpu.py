"""CPU: the ensemble Kalman filter (csrc/va_enkf.h) without a GPU -- the forecast, the statistics, the inflation and the serial
square-root analysis with the kernel's element / LDS mapping, run lane by lane on the host by a g++ build of
tests/cpu_emul/enkf_check.cpp (the same headers the kernel includes), against the filter written in NumPy (tests/_enkf_ref.py,
where the tolerance is derived); the plan and the argument checks of csrc/va_enkf_geo.h; a twin experiment in which the filter
has to filter; and what va_ode.Annealer.track hands to the device layer and makes of its answer."""
import os
import subprocess

import numpy as np
import pytest

import _enkf_ref
from _enkf_ref import COMBOS, KEYS, MISSING_CASE, OBS_EVERY, OBS_VAR, SHAPES, TOL, TWIN, l96_case, l96_enkf_reference
from _predict_ref import DT, K_TRUE, l96, rk4
from _predict_ref import TOL as TOL_X
from varanneal_amd import _capi, va_ode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (D, M) -> threads, E, wave
GEOMETRY = {(5, 4): (64, 1, 1), (5, 12): (64, 1, 1), (5, 13): (128, 1, 0), (20, 8): (192, 1, 0), (20, 30): (256, 3, 0),
            (33, 31): (256, 4, 0), (64, 32): (256, 8, 0), (20, 102): (256, 8, 0)}


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("enkf") / "enkf_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "varanneal_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpu_emul", "enkf_check.cpp")])
    return exe


def _host_run(exe, tmp_path, x0, p, Y, NQ=0, obs_every=OBS_EVERY, substeps=1, inflation=1.0, obs_var=OBS_VAR, t0=0.0):
    """x0 (T, M, D), p (T, M, 1), Y (T, n_obs, L) with every second column observed"""
    T, M, D = x0.shape
    n_obs, L = Y.shape[1:]
    assert L == (D + 1) // 2
    f, o = tmp_path / "in.bin", tmp_path / "out.bin"
    np.concatenate([np.asarray(a, dtype=np.float64).ravel() for a in (x0, p, Y, np.full(L, obs_var))]).tofile(str(f))
    run = subprocess.run([exe, "run", str(D), str(T), str(M), str(NQ), str(n_obs), str(obs_every), str(substeps), repr(DT), repr(float(t0)),
                          repr(float(inflation)), str(f), str(o)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    raw = np.fromfile(str(o))
    NV = D + NQ
    sizes = [T * n_obs * NV] * 4 + [T * M * D, T * M, T]
    assert raw.size == sum(sizes)
    mf, sf, ma, sa, xe, pe, st = np.split(raw, np.cumsum(sizes)[:-1])
    sh = (T, n_obs, NV)
    return dict(mean_f=mf.reshape(sh), sd_f=sf.reshape(sh), mean_a=ma.reshape(sh), sd_a=sa.reshape(sh), x_end=xe.reshape(T, M, D),
                p_end=pe.reshape(T, M, 1), status=st.astype(np.int64), geo=[int(v) for v in run.stdout.split()])


def test_reference_self_check():
    wm, wc = _enkf_ref.self_check()
    print("one analysis against the batch Kalman update: mean %.3e  covariance %.3e (relative)" % (wm, wc))
    assert wm <= 1e-12 and wc <= 1e-12


def _compare(got, ref, what):
    errs = {k: float(np.abs(got[k] - ref[k]).max()) for k in KEYS}
    print("%s: |C++ - NumPy| %s" % (what, "  ".join("%s %.3e" % (k, errs[k]) for k in KEYS)))
    assert np.all(got["status"] == 0) and np.all(ref["status"] == 0)
    for k in KEYS:
        assert errs[k] <= TOL, k


@pytest.mark.parametrize("D,M", SHAPES)
@pytest.mark.parametrize("NQ,substeps,inflation", COMBOS)
def test_host_path_matches_numpy(check_exe, tmp_path, D, M, NQ, substeps, inflation):
    """3 points, a forcing of its own each, one workgroup each.  (5, 4), (5, 12): one wave; (5, 13): 65 elements, two waves, idle
    lanes; (20, 8): 192 threads; (20, 30): 256 x 3; (33, 31): 256 x 4, an odd width, idle lanes; (64, 32): 256 x 8 full, the even
    width padded to 65; (20, 102): 256 x 8, idle lanes.  NQ = 1 estimates the forcing."""
    x0, p, Y, Lidx, ref = l96_enkf_reference(D, M, NQ, substeps, inflation)
    got = _host_run(check_exe, tmp_path, x0, p, Y, NQ=NQ, substeps=substeps, inflation=inflation)
    assert tuple(got["geo"][:3]) == GEOMETRY[(D, M)] and got["geo"][3] == D | 1 and got["geo"][5] == 3
    _compare(got, ref, "D=%d M=%d NQ=%d substeps=%d inflation=%.2f geometry %s" % (D, M, NQ, substeps, inflation, got["geo"]))
    if NQ == 0:
        assert np.array_equal(got["p_end"], p)
    else:
        assert np.all(got["p_end"] != p)                                   # (every member's forcing was moved)


def test_missing_observations(check_exe, tmp_path):
    """NaN entries scattered over Y, and one whole row of point 1 missing: that row's analysis is its forecast"""
    D, M, NQ, substeps, inflation = MISSING_CASE
    x0, p, Y, Lidx, ref = l96_enkf_reference(D, M, NQ, substeps, inflation, missing=True)
    assert np.isnan(Y).sum() > 20 and np.all(np.isnan(Y[1, 3]))
    got = _host_run(check_exe, tmp_path, x0, p, Y, NQ=NQ, substeps=substeps, inflation=inflation)
    _compare(got, ref, "missing data")
    full = l96_enkf_reference(D, M, NQ, substeps, inflation)[4]
    assert np.abs(full["mean_a"] - ref["mean_a"]).max() > 1e-3             # (the missing entries do matter)
    # the whole row missing: the analysis statistics are those of the inflated forecast -- the same mean to rounding
    assert np.abs(got["mean_a"][1, 3] - got["mean_f"][1, 3]).max() <= TOL
    assert np.abs(got["sd_a"][1, 3] - inflation * got["sd_f"][1, 3]).max() <= TOL


def test_without_observations_it_is_the_forecast(check_exe, tmp_path):
    """every observation NaN, inflation 1: x_end is _predict_ref.rk4 of every member, p_end is p, exactly"""
    D, M = 20, 8
    x0, p, Y, Lidx = l96_case(D, M)
    got = _host_run(check_exe, tmp_path, x0, p, np.full_like(Y, np.nan), NQ=1, substeps=2)
    want = np.array([[rk4(l96, x0[t, m], p[t, m, 0], Y.shape[1] * OBS_EVERY, DT, substeps=2)[-1] for m in range(M)] for t in range(x0.shape[0])])
    err = np.abs(got["x_end"] - want).max()
    print("all observations missing: |x_end - rk4| = %.3e" % err)
    assert err <= TOL_X and np.array_equal(got["p_end"], p) and not got["status"].any()
    assert np.array_equal(got["mean_a"], got["mean_f"]) and np.array_equal(got["sd_a"], got["sd_f"])


def test_the_filter_filters(check_exe, tmp_path):
    """Twin experiment (_enkf_ref.twin_case): D = 20, every second column observed with noise of variance 0.25 every 2 steps,
    30 members spread by 1 around a start 1 off the truth, inflation 1.05, 60 rows (120 steps).  RMS error of the analysis mean
    on the UNOBSERVED columns over the second half: below half that of the same ensemble's mean run without observations.
    The NumPy reference alone gives 0.187 with the data against 3.543 without (a factor of 19)."""
    c = TWIN
    x0, p, Y, Lidx, un, truth = _enkf_ref.twin_case()
    kw = dict(obs_every=c["obs_every"], inflation=c["inflation"], obs_var=c["obs_var"])
    ov = np.full(len(Lidx), c["obs_var"])
    ra = _enkf_ref.enkf_ref(_enkf_ref.l96_rows, x0, p, [], Y, Lidx, ov, DT, obs_every=c["obs_every"], inflation=c["inflation"], batched=True)
    rf = _enkf_ref.enkf_ref(_enkf_ref.l96_rows, x0, p, [], np.full_like(Y, np.nan), Lidx, ov, DT, obs_every=c["obs_every"],
                            inflation=c["inflation"], batched=True)
    ea, ef = _enkf_ref.twin_errors(ra["mean_a"], rf["mean_a"])
    print("reference: RMS error on the unobserved columns, second half: %.3f with the data, %.3f without" % (ea, ef))
    assert ea < 0.25 * ef                                                 # (the reference keeps another factor of 2)
    a = _host_run(check_exe, tmp_path, x0[None], p[None], Y[None], **kw)
    f = _host_run(check_exe, tmp_path, x0[None], p[None], np.full_like(Y, np.nan)[None], **kw)
    ea, ef = _enkf_ref.twin_errors(a["mean_a"][0], f["mean_a"][0])
    print("host emulation: %.3f with the data, %.3f without" % (ea, ef))
    assert not a["status"].any() and not f["status"].any()
    assert ea < 0.5 * ef


def test_nan_member_loses_its_point_only(check_exe, tmp_path):
    D, M = 20, 8
    x0, p, Y, Lidx = l96_case(D, M)
    good = _host_run(check_exe, tmp_path, x0, p, Y, NQ=1, inflation=1.05)
    bad0 = np.array(x0)
    bad0[1, 3, 7] = np.nan
    got = _host_run(check_exe, tmp_path, bad0, p, Y, NQ=1, inflation=1.05)
    assert list(got["status"]) == [0, 1, 0] and not good["status"].any()
    for k in ("mean_f", "sd_f", "mean_a", "sd_a"):
        assert np.all(np.isnan(got[k][1]))
    for k in KEYS:
        assert np.array_equal(got[k][[0, 2]], good[k][[0, 2]]), k


def test_plan(check_exe):
    plan = lambda *a: subprocess.run([check_exe, "plan"] + [str(v) for v in a], capture_output=True, text=True).stdout.strip()
    for (D, M), (threads, E, wave) in GEOMETRY.items():
        for NQ in (0, 1):
            w = plan(D, M, 1, NQ, 0).split()
            assert w[0] == "OK", w
            assert [int(v) for v in w[1:7]] == [D, M, threads, E, wave, D | 1]
            assert int(w[7]) == 8 * (2 * M * (D | 1) + M + 3 * (D + NQ) + 4) and int(w[7]) <= 64 * 1024
            assert w[8] == "3" and w[9:11] == ["1", "1"]                    # one workgroup per point, one lane per element
            assert E * threads >= M * D and threads % 64 == 0 and (wave == 1) == (M * D <= 64)
    # every ensemble of a few widths: one lane per element, one wave exactly while M D <= 64
    for D in (1, 3, 20, 33, 64):
        for M in (2, 3, 2048 // D):
            w = plan(D, M, 1, 1, 0).split()
            assert w[0] == "OK" and w[9:11] == ["1", "1"] and (w[5] == "1") == (M * D <= 64), w
    for args, word in (((20, 1, 1, 0, 0), "at least 2 members"), ((20, 103, 1, 0, 0), "2048"), ((64, 33, 1, 0, 0), "2048"),
                       ((64, 32, 200, 0, 0), "LDS"), ((5, 4, 1, 0, 65), "stimulus"), ((0, 4, 1, 0, 0), "bad sizes"),
                       ((5, 4, 1, 2, 0), "bad sizes"), ((5, 4, -1, 0, 0), "bad sizes")):
        ln = plan(*args)
        assert ln.startswith("NO") and word in ln, ln


@pytest.mark.parametrize("args,word", [
    (("3", "8", "4", "2", "10", "10", "4", "1", "1.0", "ok", "ok"), None),
    (("3", "8", "4", "0", "10", "10", "4", "2", "1.05", "null", "ok"), None),
    (("0", "8", "4", "0", "10", "10", "4", "1", "1.0", "ok", "ok"), "at least 1"),
    (("3", "0", "4", "0", "10", "10", "4", "1", "1.0", "ok", "ok"), "at least 1"),
    (("3", "8", "4", "0", "10", "0", "4", "1", "1.0", "ok", "ok"), "at least 1"),
    (("3", "8", "4", "0", "10", "10", "0", "1", "1.0", "ok", "ok"), "at least 1"),
    (("3", "8", "4", "0", "10", "10", "4", "0", "1.0", "ok", "ok"), "at least 1"),
    (("3", "8", "4", "5", "10", "10", "4", "1", "1.0", "ok", "ok"), "NQ=5"),
    (("3", "8", "4", "-1", "10", "10", "4", "1", "1.0", "ok", "ok"), "NQ=-1"),
    (("3", "8", "4", "2", "10", "10", "4", "1", "1.0", "null", "ok"), "est is NULL"),
    (("3", "8", "4", "2", "10", "10", "4", "1", "1.0", "out", "ok"), "outside"),
    (("3", "8", "4", "2", "10", "10", "4", "1", "1.0", "neg", "ok"), "outside"),
    (("3", "8", "4", "3", "10", "10", "4", "1", "1.0", "rep", "ok"), "repeated"),
    (("3", "8", "4", "2", "10", "10", "4", "1", "1.0", "ok", "zero"), "variances"),
    (("3", "8", "4", "2", "10", "10", "4", "1", "1.0", "ok", "neg"), "variances"),
    (("3", "8", "4", "2", "10", "10", "4", "1", "1.0", "ok", "nan"), "variances"),
    (("3", "8", "4", "2", "10", "10", "4", "1", "1.0", "ok", "inf"), "variances"),
    (("3", "8", "4", "2", "10", "10", "4", "1", "1.0", "ok", "null"), "obs_var is NULL"),
    (("3", "8", "4", "2", "10", "10", "4", "1", "0.99", "ok", "ok"), "inflation"),
    (("3", "8", "4", "2", "10", "10", "4", "1", "nan", "ok", "ok"), "inflation"),
    (("3", "8", "4", "2", "10", "10", "4", "1", "inf", "ok", "ok"), "inflation"),
])
def test_check_args(check_exe, args, word):
    """T M NP NQ L n_obs obs_every substeps inflation est obs_var"""
    ln = subprocess.run([check_exe, "args"] + list(args), capture_output=True, text=True).stdout.strip()
    if word is None:
        assert ln == "OK"
    else:
        assert ln.startswith("NO ") and word in ln, ln


# ---------------------------------------------------------------------------------------------------------------
class _Recorder(object):
    """device stand-in: answers anneal() with recognisable minimising paths, laplace() with a known covariance, and records what
    enkf() is handed; its statistics are a known function of the members"""
    made = []
    lap_status = None

    def __init__(self, batch, D, N_model, Y, Lidx, dt_model, RM, RF0, P, Pidx, **kw):
        self.B, self.D, self.N, self.NPest, self.Pidx = batch, D, N_model, len(Pidx), list(Pidx)
        self.P, self.kw, self.dt = np.array(P), kw, dt_model
        self.calls, self.lap_calls = [], []
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

    @staticmethod
    def joint_cov(j, nw):
        A = np.random.RandomState(50 + j).randn(nw, nw)
        return np.dot(A, A.T) / nw + 0.1 * np.eye(nw)

    def laplace(self, XP, rf_scale, P=None, gauss_newton=False, full=False, chunk_pts=0):
        npts, N, D, NPe = XP.shape[0], self.N, self.D, self.NPest
        self.lap_calls.append(dict(npts=npts, gauss_newton=gauss_newton, full=full))
        out = dict(var_x=np.ones((npts, N, D)), cov_pp=np.zeros((npts, NPe, NPe)), logdet=np.zeros(npts), status=np.zeros(npts, np.int32),
                   cov_xx=np.zeros((npts, N, D, D)), cov_px=np.zeros((npts, NPe, N * D)))
        for j in range(npts):
            S = self.joint_cov(j, D + NPe)
            out["cov_xx"][j, N - 1], out["cov_pp"][j] = S[:D, :D], S[D:, D:]
            out["cov_px"][j].reshape(NPe, N, D)[:, N - 1] = S[D:, :D]
        if _Recorder.lap_status is not None:
            out["status"][:] = _Recorder.lap_status[:npts]
            out["cov_xx"][out["status"] != 0] = np.nan
        return out

    def enkf(self, x0, p, Y, obs_var, obs_every=1, est=(), inflation=1.0, t0=0.0, substeps=1, stim=None):
        x0, p, Y = np.array(x0), np.array(p), np.array(Y)
        self.calls.append(dict(x0=x0, p=p, Y=Y, obs_var=np.array(obs_var), obs_every=obs_every, est=list(est), inflation=inflation, t0=t0,
                               substeps=substeps, stim=stim))
        T, M, D = x0.shape
        n_obs = Y.shape[0]
        z = np.concatenate([x0, p[:, :, list(est)]], axis=2).mean(axis=1)           # (T, NV)
        rows = np.arange(n_obs)[None, :, None]
        st = np.zeros(T, dtype=np.int32)
        if T > 2:
            st[2] = 4
        return dict(mean_f=z[:, None, :] + rows, sd_f=0 * z[:, None, :] + 2.0 + rows, mean_a=z[:, None, :] + rows + 0.5,
                    sd_a=0 * z[:, None, :] + 1.0 + rows, x_end=x0 + 1.0, p_end=p + 2.0, status=st)


def _l96(t, x, k):
    return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - x + k


def _noise(seed, chain, iteration, n):
    r = np.random.RandomState(1000 * seed + chain + 7 * iteration).randn(n)
    return None, r, None


def _annealed(monkeypatch, B, RM=4.0, tdp=False, Pidx=(0,)):
    from varanneal_amd import codegen
    monkeypatch.setattr(_capi, "Problem", _Recorder)
    monkeypatch.setattr(_capi, "hmc_noise", _noise)
    _Recorder.made, _Recorder.lap_status = [], None
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
    a.anneal(X0, P0, 2.0, list(range(nb)), RM, 1e-2, Lidx, list(Pidx), disc="trapezoid", verbose=False)
    return a, _Recorder.made[-1], D, N, nb, Lidx


def test_track_members_from_the_laplace_factor(monkeypatch):
    a, dev, D, N, nb, Lidx = _annealed(monkeypatch, None)
    L, n_obs, M = len(Lidx), 6, 5
    Yf = np.random.RandomState(4).randn(n_obs, L)
    Yf[2, 1] = np.nan
    r = a.track(Yf, obs_every=3, members=M, inflation=1.02, substeps=2, seed=9, gauss_newton=True)
    (c,) = dev.calls
    assert dev.lap_calls == [dict(npts=1, gauss_newton=True, full=True)]
    mp = a.minpaths
    nw = D + 1
    F = np.linalg.cholesky(_Recorder.joint_cov(0, nw))
    z = _noise(9, 0, 0, M * nw)[1].reshape(M, nw)
    want = np.concatenate([mp[nb - 1, (N - 1) * D:N * D], mp[nb - 1, N * D:]])[None, :] + np.dot(z, F.T)
    assert c["x0"].shape == (1, M, D) and c["p"].shape == (1, M, 1)
    assert np.array_equal(c["x0"][0], want[:, :D]) and np.array_equal(c["p"][0], want[:, D:])
    assert np.array_equal(c["Y"], Yf, equal_nan=True) and np.array_equal(c["obs_var"], np.full(L, 0.25))       # 1 / RM
    assert (c["obs_every"], c["est"], c["inflation"], c["substeps"], c["stim"]) == (3, [0], 1.02, 2, None)
    assert c["t0"] == a.t_model[-1] == 0.5 + DT * (N - 1)
    assert set(r) == {"mean", "std", "mean_forecast", "std_forecast", "params", "params_std", "innovation", "x_end", "p_end", "status",
                      "seeds", "rungs"}
    assert r["mean"].shape == r["std"].shape == r["mean_forecast"].shape == r["std_forecast"].shape == (1, n_obs, D)
    assert r["params"].shape == r["params_std"].shape == (1, n_obs, 1) and r["innovation"].shape == (1, n_obs, L)
    assert r["x_end"].shape == (1, M, D) and r["p_end"].shape == (1, M, 1) and r["status"].shape == (1,)
    zbar = np.concatenate([c["x0"][0], c["p"][0]], axis=1).mean(axis=0)
    rows = np.arange(n_obs)[:, None]
    assert np.array_equal(r["mean"][0], zbar[:D] + rows + 0.5) and np.array_equal(r["mean_forecast"][0], zbar[:D] + rows)
    assert np.array_equal(r["params"][0], zbar[D:] + rows + 0.5) and np.array_equal(r["params_std"][0], 1.0 + rows + 0 * zbar[D:])
    assert np.array_equal(r["innovation"][0], Yf - (zbar[:D] + rows)[:, Lidx], equal_nan=True) and np.isnan(r["innovation"][0, 2, 1])
    assert np.array_equal(r["x_end"][0], c["x0"][0] + 1.0) and list(r["rungs"]) == [nb - 1]


def test_track_batch_selection_and_failed_points(monkeypatch):
    B = 4
    a, dev, D, N, nb, Lidx = _annealed(monkeypatch, B, RM=[2.0] * 5 + [8.0] * 5)
    _Recorder.lap_status = np.array([0, 3, 0, 0, -1, 0], dtype=np.int32)
    L, n_obs, M = len(Lidx), 5, 4
    Yf = np.random.RandomState(5).randn(n_obs, L)
    r = a.track(Yf, members=M, beta=[1, 2], seeds=[3, 0, 2], estimate_params=False)
    (c,) = dev.calls                                                               # all selected points in ONE call
    mp = a.minpaths
    assert c["x0"].shape == (6, M, D) and c["est"] == []
    assert np.array_equal(c["obs_var"], 1.0 / np.array([2.0] * 5 + [8.0] * 5))     # per-column RM
    # a point without a factor goes down unperturbed and comes back NaN with its own status; the stand-in lost point 2 at row 3
    assert np.array_equal(c["x0"][1], np.broadcast_to(mp[3, 2, (N - 1) * D:N * D], (M, D)))
    assert np.array_equal(c["p"][1], np.broadcast_to(mp[3, 2, N * D:], (M, 1))) and np.array_equal(c["p"][4], np.broadcast_to(mp[2, 1, N * D:], (M, 1)))
    # (estimate_params=False: the members keep the parameters the posterior gave them, the filter leaves them alone)
    assert np.all(c["p"][0] != mp[3, 1, N * D:]) and abs(c["p"][0].mean() - mp[3, 1, N * D]) < 2.0
    assert r["status"].shape == (3, 2) and list(r["status"].ravel()) == [0, 3, 4, 0, -1, 0]
    assert r["mean"].shape == (3, 2, n_obs, D) and r["params"].shape == (3, 2, n_obs, 0) and r["x_end"].shape == (3, 2, M, D)
    for k in ("mean", "std", "mean_forecast", "std_forecast", "innovation", "x_end", "p_end"):
        assert np.all(np.isnan(r[k][0, 1])) and np.all(np.isnan(r[k][2, 0])) and np.all(np.isfinite(r[k][0, 0])), k
    assert list(r["seeds"]) == [3, 0, 2] and list(r["rungs"]) == [1, 2]
    # the draws of point j are keyed by j: point 0's differ from point 2's
    assert not np.array_equal(c["x0"][0] - c["x0"][0].mean(axis=0), c["x0"][2] - c["x0"][2].mean(axis=0))


def test_track_members_from_samples(monkeypatch):
    B = 3
    a, dev, D, N, nb, Lidx = _annealed(monkeypatch, B)
    rng = np.random.RandomState(8)
    S, sb, kb = 7, np.array([2, 0]), np.array([1])
    samples = dict(x_last=rng.randn(2, 1, S, D), params=rng.randn(2, 1, S, 1), seeds=sb, rungs=kb)
    Yf = rng.randn(4, len(Lidx))
    r = a.track(Yf, samples=samples, obs_var=np.full(len(Lidx), 0.3))
    (c,) = dev.calls
    assert not dev.lap_calls
    assert np.array_equal(c["x0"], samples["x_last"].reshape(2, S, D)) and np.array_equal(c["p"], samples["params"].reshape(2, S, 1))
    assert np.array_equal(c["obs_var"], np.full(len(Lidx), 0.3)) and c["est"] == [0]
    assert r["mean"].shape == (2, 1, 4, D) and r["x_end"].shape == (2, 1, S, D) and not r["status"].any()
    with pytest.raises(ValueError, match="keep=None"):
        a.track(Yf, samples=dict(kept=1, seeds=sb, rungs=kb))


def test_track_refusals(monkeypatch):
    a, dev, D, N, nb, Lidx = _annealed(monkeypatch, None)
    L = len(Lidx)
    Yf = np.zeros((4, L))
    with pytest.raises(ValueError):
        a.track(np.zeros((4, L + 1)))
    with pytest.raises(ValueError):
        a.track(np.zeros(L))
    with pytest.raises(ValueError):
        a.track(Yf, members=1)
    with pytest.raises(ValueError):
        a.track(Yf, inflation=0.9)
    with pytest.raises(ValueError):
        a.track(Yf, obs_var=np.zeros(L))
    with pytest.raises(ValueError):
        a.track(Yf, obs_var=np.ones(L + 1))
    with pytest.raises(ValueError):
        a.track(Yf, seeds=[0])                         # not a batch
    with pytest.raises(IndexError):
        a.track(Yf, beta=nb)
    assert not dev.calls
    with pytest.raises(ValueError, match="anneal"):
        va_ode.Annealer().track(Yf)
    # RM that changes along the window, and full RM matrices: an explicit obs_var
    rm = np.full((N, L), 4.0)
    rm[3] = 5.0
    ar, devr, _, _, _, _ = _annealed(monkeypatch, None, RM=rm)
    with pytest.raises(ValueError, match="obs_var"):
        ar.track(Yf)
    ar.track(Yf, obs_var=0.5)
    assert np.array_equal(devr.calls[0]["obs_var"], np.full(L, 0.5))
    am, devm, _, _, _, _ = _annealed(monkeypatch, None, RM=4.0 * np.eye(L))
    with pytest.raises(ValueError, match="obs_var"):
        am.track(Yf)
    at, devt, _, _, _, _ = _annealed(monkeypatch, None, tdp=True)
    with pytest.raises(NotImplementedError):
        at.track(Yf)
