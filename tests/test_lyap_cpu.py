"""CPU: Lyapunov spectra (csrc/va_lyap.h) without a GPU -- the tangent-linear RK4 rule with the gain term, the kernel's
element / LDS mapping and its Gram-Schmidt QR, run lane by lane on the host by a g++ build of tests/cpu_emul/lyap_check.cpp
(the same headers the kernel includes), against Benettin's method written in NumPy (tests/_lyap_ref.py, where the tolerance
is derived); the plan and the argument checks of csrc/va_lyap_geo.h; and what va_ode.Annealer.lyapunov / sync_exponents hand
to the device layer and make of its answer."""
import os
import subprocess

import numpy as np
import pytest

import _lyap_ref
from _lyap_ref import FORCINGS, TOL, gain_every_second, l96_lyap_reference
from _predict_ref import DT, K_TRUE, STEPS, attractor_starts, l96
from _predict_ref import TOL as TOL_X
from _tlm_ref import l96_jvp, tlm_rk4
from varanneal_amd import _capi, va_ode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("lyap") / "lyap_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "varanneal_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpu_emul", "lyap_check.cpp")])
    return exe


def _host_run(exe, tmp_path, x0, ks, K, n_steps=STEPS, substeps=1, qr_every=1, n_skip=0, Q0=None, gain=None, t0=0.0):
    T, D = x0.shape
    f, o = tmp_path / "in.bin", tmp_path / "out.bin"
    parts = [np.asarray(x0, dtype=np.float64).ravel(), np.asarray(ks, dtype=np.float64).ravel()]
    if Q0 is not None:
        parts.append(np.asarray(Q0, dtype=np.float64).ravel())
    if gain is not None:
        parts.append(np.asarray(gain, dtype=np.float64).ravel())
    np.concatenate(parts).tofile(str(f))
    run = subprocess.run([exe, "traj", str(D), str(T), str(K), str(n_steps), str(substeps), str(qr_every), str(n_skip), repr(DT), repr(float(t0)),
                          str(int(Q0 is not None)), str(int(gain is not None)), str(f), str(o)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    n_qr = n_steps // qr_every
    raw = np.fromfile(str(o))
    sizes = [T * K, T * D, T * K * D, T * n_qr * K, T]
    assert raw.size == sum(sizes)
    ls, xe, qe, tr, st = np.split(raw, np.cumsum(sizes)[:-1])
    return dict(logsum=ls.reshape(T, K), x_end=xe.reshape(T, D), Q_end=qe.reshape(T, K, D), trace=tr.reshape(T, n_qr, K),
                status=st.astype(np.int64), geo=[int(v) for v in run.stdout.split()])


def test_reference_self_check():
    wa, wb = _lyap_ref.self_check()
    print("coupled tangent step against the complex step of the drive-response pair: %.3e; Gram-Schmidt QR against np.linalg.qr: %.3e"
          % (wa, wb))
    assert wa <= 1e-13 and wb <= 1e-13


def _compare(got, ref, K, n_skip, what):
    el, eq = np.abs(got["logsum"] - ref["logsum"]).max(), np.abs(got["Q_end"] - ref["Q_end"]).max()
    ex, et = np.abs(got["x_end"] - ref["x_end"]).max(), np.abs(got["trace"] - ref["trace"]).max()
    eo = np.abs(np.einsum("tki,tli->tkl", got["Q_end"], got["Q_end"]) - np.eye(K)).max()
    print("%s: |C++ - NumPy| logsum %.3e  Q_end %.3e  x_end %.3e  trace %.3e; |Q Q^T - I| %.3e" % (what, el, eq, ex, et, eo))
    assert np.all(got["status"] == 0) and np.all(ref["status"] == 0)
    assert el <= TOL and eq <= TOL and et <= TOL and ex <= TOL_X
    assert eo <= TOL
    if n_skip == 0:
        assert np.abs(got["trace"].sum(axis=1) - got["logsum"]).max() <= TOL
    else:
        assert np.abs(got["trace"][:, n_skip:].sum(axis=1) - got["logsum"]).max() <= TOL
        assert np.abs(got["trace"][:, :n_skip]).max() > 0.0                       # (the transient is in the trace all the same)


@pytest.mark.parametrize("D", [5, 20, 33])
@pytest.mark.parametrize("kk", ["1", "3", "D"])
@pytest.mark.parametrize("substeps,qr_every", [(1, 1), (2, 4)])
@pytest.mark.parametrize("n_skip", [0, 2])
@pytest.mark.parametrize("gain", [False, True])
def test_host_path_matches_numpy(check_exe, tmp_path, D, kk, substeps, qr_every, n_skip, gain):
    """3 trajectories, a forcing of its own each.  D = 5: one wave -- K = 1 six trajectories to a wave (three live), K = 3 three,
    K = 5 two (a second, part-filled workgroup); D = 20: K = 1 one wave, K = 3 two waves, K = 20 256 lanes x 2 elements;
    D = 33 (an odd width above 32, idle lanes): K = 33 1122 elements on 256 lanes x 5"""
    T, K = 3, D if kk == "D" else int(kk)
    x0, ks, g, ref = l96_lyap_reference(D, T, K, substeps, qr_every, n_skip, gain)
    got = _host_run(check_exe, tmp_path, x0, ks, K, substeps=substeps, qr_every=qr_every, n_skip=n_skip, gain=g)
    _compare(got, ref, K, n_skip, "D=%d K=%d substeps=%d qr_every=%d n_skip=%d gain=%s geometry %s" % (D, K, substeps, qr_every, n_skip, gain, got["geo"]))
    if gain and K == D:
        free = l96_lyap_reference(D, T, K, substeps, qr_every, n_skip, False)[3]
        assert np.all(ref["logsum"].sum(axis=1) < free["logsum"].sum(axis=1) - 1.0)        # (the gain does contract)


def _logdet_propagator(x0, k, D):
    """log |det M| of the propagator of STEPS steps, from the tangent-linear reference with identity directions"""
    V = np.hstack([np.eye(D), np.zeros((D, 1))])
    M = tlm_rk4(l96, l96_jvp, x0, k, V, STEPS, DT)[1][:, -1, :]
    return np.linalg.slogdet(M)[1]


@pytest.mark.parametrize("D", [5, 20])
def test_sum_of_the_spectrum_is_the_log_determinant(check_exe, tmp_path, D):
    """K = D, no gain: sum_j logsum_j = log |det M| whatever the QR interval"""
    T = 3
    x0, ks = attractor_starts(D, T), FORCINGS[:T]
    want = np.array([_logdet_propagator(x0[i], ks[i], D) for i in range(T)])
    for qr_every in (1, 4, 8, 40):
        got = _host_run(check_exe, tmp_path, x0, ks, D, qr_every=qr_every)
        err = np.abs(got["logsum"].sum(axis=1) - want).max()
        print("D=%d qr_every=%d: |sum logsum - log|det M|| = %.3e (log|det M| %s)" % (D, qr_every, err, want))
        assert np.all(got["status"] == 0) and err <= TOL * D


def test_continuation_is_bit_equal(check_exe, tmp_path):
    D, T, K = 20, 3, 7
    x0, ks = attractor_starts(D, T), FORCINGS[:T]
    g = np.broadcast_to(gain_every_second(D, 2.0), (T, D))
    one = _host_run(check_exe, tmp_path, x0, ks, K, n_steps=40, substeps=2, qr_every=4, gain=g)
    a = _host_run(check_exe, tmp_path, x0, ks, K, n_steps=20, substeps=2, qr_every=4, gain=g)
    b = _host_run(check_exe, tmp_path, a["x_end"], ks, K, n_steps=20, substeps=2, qr_every=4, gain=g, Q0=a["Q_end"], t0=20 * DT)
    assert np.array_equal(b["x_end"], one["x_end"]) and np.array_equal(b["Q_end"], one["Q_end"])
    assert np.array_equal(np.concatenate([a["trace"], b["trace"]], axis=1), one["trace"])


def test_rank_deficient_start(check_exe, tmp_path):
    """two equal tangents in trajectory 1: R_22 is an exact zero there (the projection coefficient is exactly 1)"""
    D, T, K = 20, 3, 4
    x0, ks = attractor_starts(D, T), FORCINGS[:T]
    Q0 = np.array(np.broadcast_to(np.linalg.qr(np.random.RandomState(2).randn(D, K))[0].T, (T, K, D)))
    good = _host_run(check_exe, tmp_path, x0, ks, K, Q0=Q0, qr_every=4)
    Q0[1, 1] = Q0[1, 0]
    got = _host_run(check_exe, tmp_path, x0, ks, K, Q0=Q0, qr_every=4)
    assert list(got["status"]) == [0, 2, 0] and list(good["status"]) == [0, 0, 0]
    assert np.all(np.isnan(got["logsum"][1])) and np.all(np.isfinite(got["x_end"]))
    for k in ("logsum", "x_end", "Q_end", "trace"):
        assert np.array_equal(got[k][[0, 2]], good[k][[0, 2]]), k
    assert np.array_equal(got["x_end"][1], good["x_end"][1])


def test_plan(check_exe):
    out = subprocess.run([check_exe, "geo", "66"], capture_output=True, text=True)
    assert out.returncode == 0
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 66 * 67 // 2
    it = iter(lines)
    for D in range(1, 67):
        for K in range(1, D + 1):
            ln = next(it)
            w = ln.split()
            assert (int(w[1]), int(w[2])) == (D, K)
            if D > 64 or (K + 1) * D > 2048:
                assert w[0] == "NO" and len(w) > 4 and ("64 columns" in ln if D > 64 else "2048" in ln), ln
                continue
            assert w[0] == "OK", ln                                                 # every (D <= 64, K <= D, (K + 1) D <= 2048) is carried
            RW, threads, E, wave, pitch, lds, grid = (int(v) for v in w[3:10])
            assert w[10:14] == ["1"] * 4, ln                                         # one lane per element, one per tangent's dot products
            elems = (K + 1) * D
            assert pitch >= D and pitch % 2 == 1
            assert 1 <= E <= 8 and threads <= 256 and threads % 64 == 0 and E * threads >= RW * elems and RW * K <= threads
            assert lds == 8 * (RW * (2 * (K + 1) * pitch + 1 + D + 2 * K + 1) + 1) and lds <= 64 * 1024
            assert grid == -(-3 // RW)
            if elems <= 64:
                assert wave == 1 and threads == 64 and E == 1 and RW == 64 // elems
            else:
                assert wave == 0 and RW == 1 and threads == min(256, -(-elems // 64) * 64) and E == -(-elems // threads)
    first = {(int(w.split()[1]), int(w.split()[2])): w.split() for w in lines}
    assert first[(5, 1)][3:7] == ["6", "64", "1", "1"] and first[(5, 5)][3:7] == ["2", "64", "1", "1"]
    assert first[(20, 20)][3:7] == ["1", "256", "2", "0"] and first[(33, 33)][3:7] == ["1", "256", "5", "0"]
    assert first[(44, 44)][3:7] == ["1", "256", "8", "0"] and first[(64, 31)][3:7] == ["1", "256", "8", "0"]
    # refusals beyond the sizes: K > D, stimulus columns, parameters past the LDS
    for args, word in ((("5", "6", "1", "0"), "more exponents"), (("5", "1", "1", "65"), "stimulus"), (("64", "31", "8000", "0"), "LDS")):
        ln = subprocess.run([check_exe, "plan"] + list(args), capture_output=True, text=True).stdout
        assert ln.startswith("NO") and word in ln, ln


@pytest.mark.parametrize("args,word", [
    (("3", "20", "20", "40", "1", "4", "0", "ok"), None),
    (("3", "20", "20", "40", "1", "4", "9", "none"), None),
    (("3", "20", "3", "40", "1", "3", "0", "none"), "multiple"),
    (("3", "20", "0", "40", "1", "1", "0", "none"), "K=0"),
    (("3", "20", "21", "40", "1", "1", "0", "none"), "K=21"),
    (("3", "20", "3", "40", "1", "4", "10", "none"), "n_skip"),
    (("3", "20", "3", "40", "1", "4", "-1", "none"), "n_skip"),
    (("3", "20", "3", "40", "1", "4", "0", "neg"), "gains"),
    (("3", "20", "3", "40", "1", "4", "0", "nan"), "gains"),
    (("3", "20", "3", "40", "1", "4", "0", "inf"), "gains"),
    (("0", "20", "3", "40", "1", "4", "0", "none"), "at least 1"),
    (("3", "20", "3", "40", "0", "4", "0", "none"), "at least 1"),
    (("3", "20", "3", "40", "1", "0", "0", "none"), "at least 1"),
])
def test_check_args(check_exe, args, word):
    ln = subprocess.run([check_exe, "args"] + list(args), capture_output=True, text=True).stdout.strip()
    if word is None:
        assert ln == "OK"
    else:
        assert ln.startswith("NO ") and word in ln, ln


# ---------------------------------------------------------------------------------------------------------------
class _Recorder(object):
    """device stand-in: answers anneal() with recognisable minimising paths and records what lyapunov() is handed; its logsum
    is a known function of the trajectory and the gain"""
    made = []

    def __init__(self, batch, D, N_model, Y, Lidx, dt_model, RM, RF0, P, Pidx, **kw):
        self.B, self.D, self.N, self.NPest = batch, D, N_model, len(Pidx)
        self.P, self.kw, self.dt = np.array(P), kw, dt_model
        self.calls = []
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
    def spectrum(K):
        """exponents 1.5, 0.5, -0.5, ... : Kaplan-Yorke 2 + (1.5 + 0.5) / 0.5 ... worked out in the test"""
        return 1.5 - np.arange(K)

    def lyapunov(self, x0, p, K, n_steps, t0=0.0, substeps=1, qr_every=1, n_skip=0, Q0=None, coupling=None, stim=None, trace=False):
        x0 = np.array(x0)
        T = x0.shape[0]
        self.calls.append(dict(x0=x0, p=np.array(p), K=K, n_steps=n_steps, t0=t0, substeps=substeps, qr_every=qr_every, n_skip=n_skip,
                               Q0=Q0, coupling=None if coupling is None else np.array(coupling), stim=stim, trace=trace))
        span = (n_steps // qr_every - n_skip) * qr_every * self.dt
        lam = np.tile(self.spectrum(K), (T, 1))
        if coupling is not None:                              # the largest conditional exponent falls by a tenth of the gain
            lam = lam - 0.1 * np.asarray(coupling).max(axis=1)[:, None]
        status = np.zeros(T, dtype=np.int32)
        if coupling is None and T > 1:
            lam[1] = np.nan
            status[1] = 3
        return dict(logsum=lam * span, exponents=lam, x_end=x0 + 1.0, Q_end=np.tile(np.eye(K, self.D), (T, 1, 1)), status=status)


def _l96(t, x, k):
    return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - x + k


def _annealed(monkeypatch, B, tdp=False):
    from varanneal_amd import codegen
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
    return a, _Recorder.made[-1], D, N, nb, Lidx


def test_annealer_lyapunov_plain_run(monkeypatch):
    a, dev, D, N, nb, Lidx = _annealed(monkeypatch, None)
    r = a.lyapunov(48, substeps=2, qr_every=4, transient=9)
    (c,) = dev.calls
    mp = a.minpaths
    # the last rung's minimiser by default: its last row, its parameters, t0 the last fitted time; K = D
    assert np.array_equal(c["x0"], mp[[nb - 1], (N - 1) * D:N * D]) and np.array_equal(c["p"], mp[[nb - 1], N * D:])
    assert c["t0"] == a.t_model[-1] == 0.5 + DT * (N - 1) and c["stim"] is None and c["coupling"] is None and c["Q0"] is None
    assert (c["K"], c["n_steps"], c["substeps"], c["qr_every"]) == (D, 48, 2, 4)
    assert c["n_skip"] == 3                                                      # 9 steps of transient: three whole QR intervals
    assert set(r) == {"exponents", "logsum", "horizon", "kaplan_yorke", "x_end", "Q_end", "status"}
    assert r["exponents"].shape == r["logsum"].shape == (1, D) and r["x_end"].shape == (1, D) and r["Q_end"].shape == (1, D, D)
    assert r["horizon"].shape == r["kaplan_yorke"].shape == r["status"].shape == (1,)
    lam = _Recorder.spectrum(D)
    assert np.array_equal(r["exponents"][0], lam) and np.allclose(r["logsum"][0], lam * 36 * DT, rtol=1e-15)
    assert r["horizon"][0] == 1.0 / 1.5
    # 1.5 + 0.5 - 0.5 - 1.5 = 0 >= 0, the next partial sum is negative: 4 + 0 / 2.5
    assert r["kaplan_yorke"][0] == 4.0
    assert np.array_equal(r["x_end"][0], mp[nb - 1, (N - 1) * D:N * D] + 1.0)


def test_annealer_lyapunov_batch_selection(monkeypatch):
    B = 4
    a, dev, D, N, nb, Lidx = _annealed(monkeypatch, B)
    mp = a.minpaths
    r = a.lyapunov(40, k=3, beta=[1, 2], seeds=[3, 0, 2], transient=0)
    (c,) = dev.calls
    assert np.array_equal(c["x0"].reshape(3, 2, D), mp[[3, 0, 2]][:, [1, 2], (N - 1) * D:N * D])
    assert np.array_equal(c["p"].reshape(3, 2, 1), mp[[3, 0, 2]][:, [1, 2], N * D:])
    assert (c["K"], c["qr_every"], c["n_skip"]) == (3, 4, 0)
    assert "kaplan_yorke" not in r                                               # (a part of the spectrum has none)
    assert r["exponents"].shape == (3, 2, 3) and r["Q_end"].shape == (3, 2, 3, D) and r["status"].shape == (3, 2)
    # NaN passes through: the stand-in's second trajectory failed
    assert list(r["status"].ravel()) == [0, 3, 0, 0, 0, 0]
    assert np.all(np.isnan(r["exponents"][0, 1])) and np.isnan(r["horizon"][0, 1])
    assert r["horizon"][1, 0] == 1.0 / 1.5
    # a leading exponent that is not positive: no horizon
    r1 = a.lyapunov(40, k=1, beta=0, seeds=0, coupling=np.full(D, 20.0))
    assert r1["exponents"][0, 0, 0] == 1.5 - 2.0 and r1["horizon"][0, 0] == np.inf
    assert np.array_equal(dev.calls[-1]["coupling"], np.full((1, D), 20.0))


def test_annealer_kaplan_yorke_edges(monkeypatch):
    assert va_ode.kaplan_yorke(np.array([1.0, 0.0, -3.0])) == 2.0 + 1.0 / 3.0
    assert va_ode.kaplan_yorke(np.array([-0.5, -1.0])) == 0.0
    assert va_ode.kaplan_yorke(np.array([1.0, 0.5])) == 2.0                      # (nothing contracts: the whole space)
    assert np.isnan(va_ode.kaplan_yorke(np.array([1.0, np.nan, -3.0])))
    ky = va_ode.kaplan_yorke(np.array([[2.0, -1.0, -4.0], [1.0, -2.0, -3.0]]))
    assert np.array_equal(ky, [2.0 + 0.25, 1.5])


def test_annealer_sync_exponents(monkeypatch):
    B = 2
    a, dev, D, N, nb, Lidx = _annealed(monkeypatch, B)
    mp = a.minpaths
    gains = [0.0, 5.0, 10.0, 20.0]
    r = a.sync_exponents(40, gains, k=2, beta=[0, 2], transient=5, qr_every=4)
    (c,) = dev.calls
    # (points x gains) as one batch, the gains of a point side by side; the gain on the measured columns only
    assert c["x0"].shape == (2 * 2 * 4, D) and c["coupling"].shape == (16, D) and c["K"] == 2 and c["n_skip"] == 2
    want = np.zeros((4, D))
    want[:, Lidx] = np.array(gains)[:, None]
    assert np.array_equal(c["coupling"].reshape(4, 4, D), np.broadcast_to(want, (4, 4, D)))
    assert np.array_equal(c["x0"].reshape(2, 2, 4, D), np.broadcast_to(mp[:, [0, 2], None, (N - 1) * D:N * D], (2, 2, 4, D)))
    assert np.array_equal(c["p"].reshape(2, 2, 4, 1), np.broadcast_to(mp[:, [0, 2], None, N * D:], (2, 2, 4, 1)))
    assert set(r) == {"exponents", "critical_gain", "gains", "status"}
    assert r["exponents"].shape == (2, 2, 4, 2) and r["critical_gain"].shape == (2, 2) and r["status"].shape == (2, 2, 4)
    assert np.allclose(r["exponents"][1, 0, :, 0], 1.5 - 0.1 * np.array(gains), rtol=0, atol=1e-15)
    assert np.all(r["critical_gain"] == 20.0)                                    # 1.5 - 0.1 c < 0 first at c = 20 of those listed
    r2 = a.sync_exponents(40, [0.0, 5.0], k=1)
    assert np.all(np.isnan(r2["critical_gain"])) and r2["critical_gain"].shape == (2, 1)      # (default rung: the last)
    with pytest.raises(ValueError):
        a.sync_exponents(40, [1.0, -1.0])


def test_annealer_lyapunov_refusals(monkeypatch):
    a, dev, D, N, nb, Lidx = _annealed(monkeypatch, None)
    with pytest.raises(ValueError):
        a.lyapunov(40, seeds=[0])                      # not a batch
    with pytest.raises(IndexError):
        a.lyapunov(40, beta=nb)
    with pytest.raises(ValueError):
        a.lyapunov(40, k=D + 1)
    with pytest.raises(ValueError):
        a.lyapunov(42, qr_every=4)                     # not a multiple
    with pytest.raises(ValueError):
        a.lyapunov(40, qr_every=4, transient=40)       # nothing left to sum
    assert not dev.calls
    with pytest.raises(ValueError, match="anneal"):
        va_ode.Annealer().lyapunov(40)
    # time-dependent parameters: the last row's parameters, as predict() takes them
    at, devt, _, _, _, _ = _annealed(monkeypatch, None, tdp=True)
    at.lyapunov(40, k=2)
    NX = N * D
    assert np.array_equal(devt.calls[0]["p"], at.minpaths[[nb - 1], NX + (N - 1) * 2:NX + N * 2])
