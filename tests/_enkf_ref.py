"""The ensemble Kalman filter's reference: forecast and serial square-root analysis in NumPy, written from the statement of the
computation (shared by tests/test_enkf_cpu.py, tests/test_gpu_enkf.py and tools/enkf_timed.py).

    A point has M members x (M, D), their full parameter vectors p (M, NP), a list est of NQ positions in p that the filter
    updates, observations Y (n_obs, L) of the columns Lidx (NaN: missing), variances obs_var (L,), inflation >= 1.
    For row k = 0 .. n_obs - 1:
      1  every member moves obs_every model steps by _predict_ref.rk4, each with its own parameter vector
      2  mean_f = sum_m z_m / M in member order, sd_f = sqrt(sum_m (z_m - mean)^2 / (M - 1)) of z = (x, p[est])
      3  unless inflation == 1.0:  z_m = mean + inflation (z_m - mean)
      4  for j = 0 .. L-1 in order, unless Y[k, j] is NaN, with c = Lidx[j], r = obs_var[j]:
             h_m = x_m[c], hbar = sum_m h_m / M, a_m = h_m - hbar, s = sum_m a_m^2 / (M - 1), d = s + r
             zbar_i = sum_m z_mi / M, c_i = sum_m (z_mi - zbar_i) a_m / (M - 1), K_i = c_i / d
             alpha = 1 / (1 + sqrt(r / d)),   z_mi += K_i (y - hbar) - alpha K_i a_m
      5  mean_a, sd_a by 2's formulas
    status = 0, or k + 1 of the first row at whose forecast some z of some member is not finite: from that row on the four
    statistics are NaN; x_end / p_end hold what the arithmetic gave.

The forecast goes through _predict_ref.rk4: per member, or (batched=True, what the Lorenz-96 cases use, because a hundred
members a call at a time cost seconds) ONE rk4 call on the (M, D) array with a right-hand side written for rows -- the same
element-wise arithmetic, and self_check() holds the two to the same bits.  The analysis is plain loops over the members.
Everything runs in np.longdouble as well.

A coding slip here cannot hide: self_check() compares, once per process, one analysis without missing data against the batch
Kalman update formed from the forecast sample covariance P_f with np.linalg.solve -- mean xbar + K (y - H xbar), covariance
(I - K H) P_f, K = P_f H^T (H P_f H^T + R)^-1 -- which a serial square-root filter with diagonal R reproduces exactly.
Measured: 4.0e-16 (mean) and 2.4e-16 (covariance) relative to the largest entry, asserted <= 1e-12.

TOL: |device or host C++ - NumPy| <= TOL, absolute, on mean_f, sd_f, mean_a, sd_a, x_end and p_end (states of size 10-15, a
forcing near 8), for 40 steps of dt = 0.025, obs_every = 4, every second column observed, obs_var = 0.25, 3 points with a
forcing of their own.  Derived by the project's rule: derive() runs enkf_ref in float64 and in longdouble at exactly the shapes
the tests use -- (D, M) = (5, 4), (5, 12), (5, 13), (20, 8), (20, 30), (33, 31), (64, 32), (20, 102), each with NQ = 0 and 1,
substeps 1 and 2, inflation 1.0 and 1.05, and the (20, 30) case with missing data -- and takes the largest absolute difference
over all outputs: 3.22e-14 (x_end at (64, 32), NQ = 1, substeps 2, inflation 1.05; between 4.6e-15 and that over the 65
cases; the statistics alone stay below 1.2e-14).  The project's 250-fold margin for FMA contraction and summation order gives
TOL = 8.1e-12.  A wrong coefficient, a gain formed from members already updated or an
observation taken out of order shows at 1e-3 or worse.  Do not lengthen the horizon without deriving this again."""
import numpy as np

from _lyap_ref import FORCINGS
from _predict_ref import DT, STEPS, attractor_starts, l96, rk4

TOL = 8.1e-12

OBS_EVERY, OBS_VAR = 4, 0.25
SHAPES = [(5, 4), (5, 12), (5, 13), (20, 8), (20, 30), (33, 31), (64, 32), (20, 102)]


def l96_rows(t, X, P, st=None):
    """Lorenz-96 on the rows of X (M, D), row m with the forcing P[m, 0]: l96's arithmetic, member by member"""
    return np.roll(X, 1, axis=1) * (np.roll(X, -1, axis=1) - np.roll(X, 2, axis=1)) - X + P[:, :1]


def _l96_member(t, x, p, st=None):
    return l96(t, x, p[0])


def _msum(A, dtype):
    """sum over the members (axis 0) in member order"""
    s = np.zeros(A.shape[1:], dtype=dtype)
    for m in range(A.shape[0]):
        s = s + A[m]
    return s


def stats(Z, dtype=np.float64):
    M = Z.shape[0]
    mean = _msum(Z, dtype) / dtype(M)
    dev = Z - mean
    return mean, np.sqrt(_msum(dev * dev, dtype) / dtype(M - 1))


def analysis(Z, y_row, Lidx, obs_var, dtype=np.float64):
    """step 4 on the augmented members Z (M, D + NQ); returns the updated copy"""
    Z = np.array(Z, dtype=dtype)
    M = Z.shape[0]
    one = dtype(1.0)
    for j in range(len(Lidx)):
        if np.isnan(y_row[j]):
            continue
        y, r = dtype(y_row[j]), dtype(obs_var[j])
        h = Z[:, Lidx[j]].copy()
        hbar = _msum(h, dtype) / dtype(M)
        a = h - hbar
        d = _msum(a * a, dtype) / dtype(M - 1) + r
        zbar = _msum(Z, dtype) / dtype(M)
        c = _msum((Z - zbar) * a[:, None], dtype) / dtype(M - 1)
        K = c / d
        alpha = one / (one + np.sqrt(r / d))
        Z = Z + (K * (y - hbar) - alpha * K * a[:, None])
    return Z


def enkf_ref(f, x0, p, est, Y, Lidx, obs_var, dt, obs_every=1, substeps=1, inflation=1.0, t0=0.0, stim=None, dtype=np.float64,
             batched=False):
    """one point.  f(t, x (D,), p (NP,), stimulus row or None) -> (D,); with batched=True f takes x (M, D) and p (M, NP).
    Returns dict(mean_f, sd_f, mean_a, sd_a (n_obs, D + NQ), x_end (M, D), p_end (M, NP), status)."""
    x = np.array(x0, dtype=dtype)
    p = np.array(p, dtype=dtype)
    M, D = x.shape
    est = [int(e) for e in est]
    Y = np.asarray(Y, dtype=np.float64)
    n_obs, NV = Y.shape[0], D + len(est)
    out = {k: np.full((n_obs, NV), np.nan, dtype=dtype) for k in ("mean_f", "sd_f", "mean_a", "sd_a")}
    status = 0
    with np.errstate(all="ignore"):
        for k in range(n_obs):
            n0 = k * obs_every
            tk = dtype(t0) + dtype(n0) * dtype(dt)
            sk = None if stim is None else stim[n0:n0 + obs_every + 1]
            if batched:
                x = rk4(f, x, p, obs_every, dt, t0=tk, substeps=substeps, stim=sk, dtype=dtype)[-1]
            else:
                x = np.array([rk4(f, x[m], p[m], obs_every, dt, t0=tk, substeps=substeps, stim=sk, dtype=dtype)[-1] for m in range(M)])
            Z = np.concatenate([x, p[:, est]], axis=1)
            if status == 0 and not np.all(np.isfinite(Z)):
                status = k + 1
            mean, sd = stats(Z, dtype)
            if status == 0:
                out["mean_f"][k], out["sd_f"][k] = mean, sd
            if inflation != 1.0:
                Z = mean + dtype(inflation) * (Z - mean)
            Z = analysis(Z, Y[k], Lidx, obs_var, dtype)
            mean, sd = stats(Z, dtype)
            if status == 0:
                out["mean_a"][k], out["sd_a"][k] = mean, sd
            x = Z[:, :D].copy()
            if est:
                p[:, est] = Z[:, D:]
    out.update(x_end=x, p_end=p, status=status)
    return out


_checked = []


def self_check():
    """(a) the batched Lorenz-96 forecast against rk4 member by member: the same bits; (b) one analysis, nothing missing,
    against the batch Kalman update from the forecast sample covariance.  Returns the two relative figures of (b)."""
    if _checked:
        return _checked[0]
    rng = np.random.RandomState(5)
    D, M = 7, 9
    X = attractor_starts(D, 1)[0] + 0.5 * rng.randn(M, D)
    P = 8.0 + 0.3 * rng.randn(M, 1)
    for substeps in (1, 2):
        a = rk4(l96_rows, X, P, 4, DT, substeps=substeps)[-1]
        b = np.array([rk4(_l96_member, X[m], P[m], 4, DT, substeps=substeps)[-1] for m in range(M)])
        assert np.array_equal(a, b), "the batched forecast is not rk4 member by member"
    worst_m = worst_c = 0.0
    for D, M, NQ in ((6, 4, 0), (6, 15, 1), (9, 30, 2)):
        NV = D + NQ
        Z = rng.randn(M, NV) * (0.5 + rng.rand(NV)) + 3.0 * rng.randn(NV)
        Lidx = list(range(0, D, 2))
        ov = 0.1 + rng.rand(len(Lidx))
        y = rng.randn(len(Lidx)) * 2.0
        Za = analysis(Z, y, Lidx, ov)
        zbar = Z.mean(axis=0)
        Pf = np.dot((Z - zbar).T, Z - zbar) / (M - 1)
        H = np.zeros((len(Lidx), NV))
        H[np.arange(len(Lidx)), Lidx] = 1.0
        S = np.dot(H, np.dot(Pf, H.T)) + np.diag(ov)
        K = np.linalg.solve(S.T, np.dot(H, Pf.T)).T
        want_mean = zbar + np.dot(K, y - np.dot(H, zbar))
        want_cov = np.dot(np.eye(NV) - np.dot(K, H), Pf)
        got_mean = Za.mean(axis=0)
        got_cov = np.dot((Za - got_mean).T, Za - got_mean) / (M - 1)
        worst_m = max(worst_m, np.abs(got_mean - want_mean).max() / np.abs(want_mean).max())
        worst_c = max(worst_c, np.abs(got_cov - want_cov).max() / np.abs(Pf).max())
    assert worst_m <= 1e-12 and worst_c <= 1e-12, "the serial square-root analysis disagrees with the batch Kalman update: mean %.3e cov %.3e" % (worst_m, worst_c)
    _checked.append((worst_m, worst_c))
    return _checked[0]


KEYS = ("mean_f", "sd_f", "mean_a", "sd_a", "x_end", "p_end")
T = 3
_cases, _refs = {}, {}


def l96_case(D, M, missing=False):
    """(x0 (T, M, D), p (T, M, 1), Y (T, n_obs, L), Lidx) of the Lorenz-96 case: point i with the forcing FORCINGS[i], members drawn
    around attractor_starts with a fixed NumPy seed, the observations the point's own truth plus noise of variance OBS_VAR.
    missing: NaN entries scattered over Y and one whole row of point 1 missing.  Read-only."""
    key = (D, M, missing)
    if key not in _cases:
        rng = np.random.RandomState(1000 + 17 * D + M)
        starts = attractor_starts(D, T)
        Lidx = list(range(0, D, 2))
        n_obs = STEPS // OBS_EVERY
        x0 = starts[:, None, :] + 0.5 * rng.randn(T, M, D)
        p = np.array(FORCINGS[:T])[:, None, None] + 0.2 * rng.randn(T, M, 1)
        truth = np.array([rk4(l96, starts[i], FORCINGS[i], STEPS, DT, every=OBS_EVERY)[1:] for i in range(T)])
        Y = truth[:, :, Lidx] + np.sqrt(OBS_VAR) * rng.randn(T, n_obs, len(Lidx))
        if missing:
            Y[rng.rand(*Y.shape) < 0.2] = np.nan
            Y[1, 3] = np.nan
            Y[0, 0, 0] = np.nan
        for a in (x0, p, Y):
            a.setflags(write=False)
        _cases[key] = (x0, p, Y, Lidx)
    return _cases[key]


def l96_enkf_reference(D, M, NQ=0, substeps=1, inflation=1.0, missing=False, dtype=np.float64):
    """(x0, p, Y, Lidx, dict of stacked outputs) of l96_case through enkf_ref.  Computed once per case, read-only."""
    self_check()
    key = (D, M, NQ, substeps, inflation, missing, dtype)
    if key not in _refs:
        x0, p, Y, Lidx = l96_case(D, M, missing)
        ov = np.full(len(Lidx), OBS_VAR)
        res = [enkf_ref(l96_rows, x0[i], p[i], [0] if NQ else [], Y[i], Lidx, ov, DT, obs_every=OBS_EVERY, substeps=substeps,
                        inflation=inflation, dtype=dtype, batched=True) for i in range(T)]
        out = {k: np.array([r[k] for r in res]) for k in res[0]}
        for a in out.values():
            a.setflags(write=False)
        _refs[key] = (x0, p, Y, Lidx, out)
    return _refs[key]


COMBOS = [(NQ, substeps, inflation) for NQ in (0, 1) for substeps in (1, 2) for inflation in (1.0, 1.05)]
MISSING_CASE = (20, 30, 1, 2, 1.05)      # (D, M, NQ, substeps, inflation) of the case with missing data


def derive(shapes=SHAPES):
    """the figures of the docstring: float64 against longdouble, largest absolute difference over all outputs, per case"""
    worst = {}
    todo = [(D, M, NQ, ss, infl, False) for D, M in shapes for NQ, ss, infl in COMBOS] + [MISSING_CASE + (True,)]
    for D, M, NQ, ss, infl, missing in todo:
        a = l96_enkf_reference(D, M, NQ, ss, infl, missing)[4]
        b = l96_enkf_reference(D, M, NQ, ss, infl, missing, dtype=np.longdouble)[4]
        assert not a["status"].any() and not b["status"].any()
        e = {k: float(np.abs(np.asarray(a[k], dtype=np.longdouble) - b[k]).max()) for k in KEYS}
        worst[(D, M, NQ, ss, infl, missing)] = max(e.values())
        print("D=%d M=%d NQ=%d substeps=%d inflation=%.2f missing=%s  float64 vs longdouble: %s" %
              (D, M, NQ, ss, infl, missing, "  ".join("%s %.2e" % (k, e[k]) for k in KEYS)), flush=True)
    return worst

TWIN = dict(D=20, M=30, n_obs=60, obs_every=2, obs_var=0.25, inflation=1.05, seed=1)


def twin_case():
    """the behavioural test's twin experiment: (x0 (M, D), p (M, 1), Y (n_obs, L), Lidx, unobserved columns, truth (n_obs, D)).
    Truth from rk4 at the true forcing; every second column observed with noise of variance obs_var; the members spread by 1
    around a start whose RMS distance from the truth is 1."""
    from _predict_ref import K_TRUE
    if "twin" not in _cases:
        c = TWIN
        rng = np.random.RandomState(c["seed"])
        D, M, n_obs, oe = c["D"], c["M"], c["n_obs"], c["obs_every"]
        start = attractor_starts(D, 1)[0]
        truth = rk4(l96, start, K_TRUE, n_obs * oe, DT, every=oe)[1:]
        Lidx = list(range(0, D, 2))
        Y = truth[:, Lidx] + np.sqrt(c["obs_var"]) * rng.randn(n_obs, len(Lidx))
        off = rng.randn(D)
        off /= np.sqrt(np.mean(off ** 2))
        x0 = start + off + rng.randn(M, D)
        p = np.full((M, 1), K_TRUE)
        for a in (x0, p, Y, truth):
            a.setflags(write=False)
        _cases["twin"] = (x0, p, Y, Lidx, [i for i in range(D) if i not in Lidx], truth)
    return _cases["twin"]


def twin_errors(mean_with, mean_without):
    """RMS error of the two analysis means (n_obs, D) on the unobserved columns over the second half of the run"""
    _, _, _, _, un, truth = twin_case()
    h = truth.shape[0] // 2
    rms = lambda m: float(np.sqrt(np.mean((np.asarray(m)[h:][:, un] - truth[h:][:, un]) ** 2)))
    return rms(mean_with), rms(mean_without)


if __name__ == "__main__":
    print("self check: mean %.2e  covariance %.2e" % self_check())
    w = derive()
    print("least %.2e  largest %.2e   x 250 = %.2e" % (min(w.values()), max(w.values()), 250 * max(w.values())))
