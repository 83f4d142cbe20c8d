"""The Lyapunov spectrum's reference: Benettin's method in NumPy, written from the statement of the computation (shared by
tests/test_lyap_cpu.py, tests/test_gpu_lyap.py and tools/lyap_timed.py).

    A trajectory has a state x (D), parameters p, K <= D tangents V (K, D) and a gain vector g (D) >= 0 (None: zeros).
    Per RK4 substep of h = dt / substeps the state moves as _predict_ref.rk4 moves it and every tangent as _tlm_ref.tlm_rk4
    moves a state direction, the parameter tangent zero, with the gain taken off every stage:
        k1' = J(x) v - g v,  k2' = J(x + h/2 k1)(v + h/2 k1') - g (v + h/2 k1'),  ...,  v += h/6 (k1' + 2 k2' + 2 k3' + k4')
    which is the derivative with respect to y, at y = x, of one RK4 step of the PAIR  x' = f(x), y' = f(y) + g (x - y).
    After every qr_every model steps: V^T = Q R (thin, R_jj > 0), V <- Q^T, and for QR index m >= n_skip  S_j += log R_jj.
    Out: logsum = S (K), x_end (D), Q_end (K, D), trace (n_qr, K) of every log R_jj, status = 0 or j + 1 of the first R_jj
    that is zero or not finite (logsum then NaN).  Exponents: logsum / ((n_qr - n_skip) qr_every dt).

The QR is modified Gram-Schmidt written element by element (qr_rows), so that it runs in np.longdouble as well; the thin QR
with a positive diagonal is unique, so whichever scheme the device uses has to agree with it to rounding.  A coding slip here
cannot hide: self_check() compares, once per process, (a) the gain-coupled tangent step against the complex-step derivative
of _predict_ref.rk4 applied to the joint drive-response system, and (b) qr_rows against np.linalg.qr with the signs fixed.

TOL: |device or host C++ - NumPy| <= TOL, absolute, on logsum, on the trace rows and on the entries of Q_end (unit vectors),
for 40 steps of dt = 0.025 from the attractor starts of _predict_ref.  Derived as _tlm_ref.TOL is: derive() runs lyap_ref in
float64 and in longdouble at the shapes the tests use -- (D, K) = (5, 1), (5, 3), (5, 5), (20, 1), (20, 3), (20, 20), (33, 1),
(33, 3), (33, 33), (64, 31), both (substeps, qr_every) pairs (1, 1) and (2, 4), without a gain and with gain 5 on every
second column, 7 trajectories each with a forcing of its own -- and takes the largest absolute difference: 1.57e-14 on
logsum ((33, 33), substeps 2, gain; between 5.1e-16 and 1.6e-14 over the cases) and 2.66e-14 on Q_end ((33, 33), substeps 2,
no gain; from 8.5e-16).  The project's 250-fold margin for FMA contraction and summation order on the larger of the two
gives 6.6e-12; x_end is held to _predict_ref.TOL as every forecast is.  A wrong coefficient, a
tangent stage that reads another stage's nominal input or a QR that skips a projection shows at 1e-4 or worse.  Do not
lengthen the horizon or the QR interval without deriving this again: Q_end is as sensitive as the gaps between neighbouring
exponents are small."""
import numpy as np

from _predict_ref import DT, K_TRUE, STEPS, attractor_starts, l96, rk4
from _tlm_ref import l96_jvp

TOL = 6.6e-12


def qr_rows(V, dtype=np.float64):
    """thin QR of V^T with a positive diagonal, modified Gram-Schmidt on the rows of V (K, D), element by element.
    Returns (Q (K, D) with orthonormal rows, R (K, K) upper triangular: V[k] = sum_j R[j, k] Q[j])."""
    V = np.array(V, dtype=dtype)
    K, D = V.shape
    R = np.zeros((K, K), dtype=dtype)
    zero = dtype(0.0)
    for j in range(K):
        s = zero
        for i in range(D):
            s = s + V[j, i] * V[j, i]
        R[j, j] = np.sqrt(s)
        for i in range(D):
            V[j, i] = V[j, i] / R[j, j]
        for k in range(j + 1, K):
            s = zero
            for i in range(D):
                s = s + V[j, i] * V[k, i]
            R[j, k] = s
            for i in range(D):
                V[k, i] = V[k, i] - s * V[j, i]
    return V, R


def qr_rows_fast(V, dtype=np.float64):
    """qr_rows with the inner loops over the columns as array operations (the sums in another order): what lyap_ref calls"""
    V = np.array(V, dtype=dtype)
    K = V.shape[0]
    R = np.zeros((K, K), dtype=dtype)
    for j in range(K):
        R[j, j] = np.sqrt((V[j] * V[j]).sum())
        V[j] = V[j] / R[j, j]
        if j + 1 < K:
            R[j, j + 1:] = (V[j + 1:] * V[j]).sum(axis=1)
            V[j + 1:] = V[j + 1:] - R[j, j + 1:, None] * V[j]
    return V, R


def tangent_step(f, jvp, x, V, p, g, t, h, sa, sb, sc, dtype=np.float64):
    """one RK4 substep of the state and the tangents; sa, sb, sc: the stimulus at the three stage times (or None)"""
    half, two, six, one = dtype(0.5), dtype(2.0), dtype(6.0), dtype(1.0)
    vp = np.zeros((V.shape[0], np.size(p)), dtype=dtype)
    ta, tb, tc = t, t + half * h, t + one * h

    def dv(tt, xx, st, vv):
        d = jvp(tt, xx, p, st, vv, vp)
        return d if g is None else d - g * vv
    k1, d1 = f(ta, x, p, sa), dv(ta, x, sa, V)
    x2, v2 = x + half * h * k1, V + half * h * d1
    k2, d2 = f(tb, x2, p, sb), dv(tb, x2, sb, v2)
    x3, v3 = x + half * h * k2, V + half * h * d2
    k3, d3 = f(tb, x3, p, sb), dv(tb, x3, sb, v3)
    x4, v4 = x + h * k3, V + h * d3
    k4, d4 = f(tc, x4, p, sc), dv(tc, x4, sc, v4)
    return x + h / six * (k1 + two * k2 + two * k3 + k4), V + h / six * (d1 + two * d2 + two * d3 + d4)


def lyap_ref(f, jvp, x0, p, K, n_steps, dt, t0=0.0, substeps=1, qr_every=1, n_skip=0, Q0=None, gain=None, stim=None,
             dtype=np.float64, qr=qr_rows_fast):
    """one trajectory.  f, jvp as _tlm_ref.tlm_rk4 takes them.  Returns dict(logsum, x_end, Q_end, trace, status)."""
    assert n_steps % qr_every == 0 and 0 <= n_skip < n_steps // qr_every and 1 <= K <= np.size(x0)
    one = dtype(1.0)
    h = dtype(dt) / dtype(substeps)
    x = np.array(x0, dtype=dtype)
    D = x.size
    V = np.eye(K, D, dtype=dtype) if Q0 is None else np.array(Q0, dtype=dtype).reshape(K, D)
    p = np.asarray(p, dtype=dtype)
    g = None if gain is None else np.asarray(gain, dtype=dtype)
    n_qr = n_steps // qr_every
    S = np.zeros(K, dtype=dtype)
    trace = np.zeros((n_qr, K), dtype=dtype)
    status = 0

    def st(n, s, c):
        if stim is None:
            return None
        w = dtype(s + c) / dtype(substeps)
        return (one - w) * stim[n] + w * stim[n + 1]
    with np.errstate(all="ignore"):
        for n in range(n_steps):
            for s in range(substeps):
                q = n * substeps + s
                x, V = tangent_step(f, jvp, x, V, p, g, dtype(t0) + dtype(q) * h, h, st(n, s, 0.0), st(n, s, 0.5), st(n, s, 1.0), dtype)
            if (n + 1) % qr_every == 0:
                m = (n + 1) // qr_every - 1
                V, R = qr(V, dtype)
                diag = np.diagonal(R)
                bad = ~(np.isfinite(diag) & (diag > 0))
                if status == 0 and bad.any():
                    status = int(np.argmax(bad)) + 1
                trace[m] = np.log(diag)
                if m >= n_skip:
                    S = S + trace[m]
    if status:
        S = np.full(K, np.nan, dtype=dtype)
    return dict(logsum=S, x_end=x, Q_end=V, trace=trace, status=status)


def complex_jvp(f, eps=1e-30):
    """a jvp for lyap_ref from the complex step of f itself (models whose Jacobian is not written out): exact to rounding"""
    def jvp(t, x, p, st, vx, vp):
        return np.array([f(t, x + 1j * eps * v, p, st).imag / eps for v in vx])
    return jvp


def gain_every_second(D, c=5.0):
    g = np.zeros(D)
    g[::2] = c
    return g


_checked = []


def self_check():
    """(a) 10 steps of tangent_step (no QR), gain 5 on every second column, D = 7, against the complex-step derivative, with
    respect to the response's start, of _predict_ref.rk4 on the joint drive-response system; (b) qr_rows and qr_rows_fast
    against np.linalg.qr with the signs fixed.  Returns the two worst figures."""
    if _checked:
        return _checked[0]
    D, n, eps = 7, 10, 1e-30
    x0 = attractor_starts(D, 2)[1]
    g = gain_every_second(D)
    rng = np.random.RandomState(11)
    V0 = rng.randn(3, D)
    worst_a = 0.0
    for substeps in (1, 2):
        h = DT / substeps
        x, V = x0.copy(), V0.copy()
        for q in range(n * substeps):
            x, V = tangent_step(l96, l96_jvp, x, V, K_TRUE, g, q * h, h, None, None, None)
        for c in range(len(V0)):
            shift = np.concatenate([np.zeros(D), 1j * eps * V0[c]])      # (rk4 takes a real start: the perturbation rides in f)

            def pair(t, z, p, st):
                z = z + shift
                xx, yy = z[:D], z[D:]
                return np.concatenate([l96(t, xx, p), l96(t, yy, p) + g * (xx - yy)])
            z = rk4(pair, np.concatenate([x0, x0]), K_TRUE, n, DT, substeps=substeps)[-1]
            assert np.abs(z[:D].real - x).max() <= 1e-12
            worst_a = max(worst_a, np.abs(z[D:].imag / eps + V0[c] - V[c]).max() / np.abs(V[c]).max())
    assert worst_a <= 1e-13, "the coupled tangent step disagrees with the complex step of the drive-response pair: %.3e" % worst_a
    worst_b = 0.0
    for K, Dq in ((1, 4), (3, 7), (6, 6)):
        A = rng.randn(K, Dq)
        Qn, Rn = np.linalg.qr(A.T)
        sg = np.sign(np.diagonal(Rn))
        Qn, Rn = Qn * sg, Rn * sg[:, None]
        for fn in (qr_rows, qr_rows_fast):
            Q, R = fn(A)
            worst_b = max(worst_b, np.abs(Q - Qn.T).max(), np.abs(R - Rn).max(), np.abs(np.dot(Q, Q.T) - np.eye(K)).max())
    assert worst_b <= 1e-13, "the Gram-Schmidt QR disagrees with np.linalg.qr: %.3e" % worst_b
    _checked.append((worst_a, worst_b))
    return _checked[0]


FORCINGS = [8.17, 7.5, 9.0, 8.0, 6.5, 10.0, 8.6]      # a forcing of its own per trajectory
_refs = {}


def l96_lyap_reference(D, T, K, substeps=1, qr_every=1, n_skip=0, gain=False, n_steps=STEPS, Q0=None):
    """(x0 (T, D), ks (T,), g (T, D) or None, dict of stacked outputs) for n_steps steps of DT from the attractor starts, trajectory
    i with the forcing FORCINGS[i]; gain: 5 on every second column.  Computed once per case, read-only."""
    self_check()
    key = (D, T, K, substeps, qr_every, n_skip, gain, n_steps, None if Q0 is None else np.asarray(Q0).tobytes())
    if key not in _refs:
        x0 = attractor_starts(D, T)
        ks = np.array(FORCINGS[:T])
        g = np.ascontiguousarray(np.broadcast_to(gain_every_second(D), (T, D))) if gain else None
        res = [lyap_ref(l96, l96_jvp, x0[i], ks[i], K, n_steps, DT, substeps=substeps, qr_every=qr_every, n_skip=n_skip,
                        Q0=None if Q0 is None else np.asarray(Q0)[i], gain=None if g is None else g[i]) for i in range(T)]
        out = {k: np.array([r[k] for r in res]) for k in res[0]}
        for a in out.values():
            a.setflags(write=False)
        _refs[key] = (x0, ks, g, out)
    return _refs[key]


SHAPES = [(5, 1), (5, 3), (5, 5), (20, 1), (20, 3), (20, 20), (33, 1), (33, 3), (33, 33), (64, 31)]


def derive(shapes=SHAPES, T=7):
    """the figures of the docstring: float64 against longdouble, per shape, (substeps, qr_every) and gain"""
    worst = {}
    for D, K in shapes:
        x0 = attractor_starts(D, T)
        for substeps, qr_every in ((1, 1), (2, 4)):
            for gain in (None, gain_every_second(D)):
                el = eq = 0.0
                for i in range(T):
                    a = lyap_ref(l96, l96_jvp, x0[i], FORCINGS[i], K, STEPS, DT, substeps=substeps, qr_every=qr_every, gain=gain)
                    b = lyap_ref(l96, l96_jvp, x0[i], FORCINGS[i], K, STEPS, DT, substeps=substeps, qr_every=qr_every, gain=gain,
                                 dtype=np.longdouble)
                    el = max(el, float(np.abs(a["logsum"] - b["logsum"]).max()))
                    eq = max(eq, float(np.abs(a["Q_end"] - b["Q_end"]).max()))
                worst[(D, K, substeps, qr_every, gain is not None)] = (el, eq)
                print("D=%d K=%d substeps=%d qr_every=%d gain=%s  float64 vs longdouble: logsum %.2e  Q_end %.2e"
                      % (D, K, substeps, qr_every, gain is not None, el, eq), flush=True)
    return worst


if __name__ == "__main__":
    print("self check: tangent %.2e  qr %.2e" % self_check())
    w = derive()
    ml, mq = max(v[0] for v in w.values()), max(v[1] for v in w.values())
    print("largest: logsum %.2e  Q_end %.2e   x 250 = %.2e" % (ml, mq, 250 * max(ml, mq)))
