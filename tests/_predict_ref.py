"""The forecast's reference: classical RK4 in NumPy, written from the rule csrc/va_predict.h states (shared by
tests/test_predict_cpu.py and tests/test_gpu_predict.py).

    h = dt / substeps;  k1 = f(x), k2 = f(x + 0.5 h k1), k3 = f(x + 0.5 h k2), k4 = f(x + h k3),
    x += h/6 (k1 + 2 k2 + 2 k3 + k4)
    stage time t0 + (n substeps + s + c) h,  c = 0, 1/2, 1/2, 1
    stimulus (n_steps + 1, nstim) at the model-step times, interpolated linearly at the stage times with weight
    (s + c) / substeps between rows n and n + 1

TOL: |device or host C++ - NumPy| <= 1e-11 absolute on states of size 10-15, for 40 steps of dt = 0.025.  The same
trajectories in float64 and in longdouble differ by at most 4e-14 after 40 steps at D = 5 ... 200 (3e-12 after 80 steps at
D = 200), which leaves a 250-fold margin for FMA contraction and summation order; a wrong coefficient or stage time
shows at 1e-4 or worse.  The system is chaotic (roundoff alone reaches 4e-9 at 200 steps): do not lengthen the horizon
without deriving this again.

TOL_WIDE: the same bound for the wide states of _forecast_shapes.py (D = 257, 513, 769, 1024), used by the tests of those
shapes only.  derive() (python tests/_predict_ref.py: 7 attractor states per width, both (substeps, every) pairs the tests
use) gives, float64 against longdouble after 40 steps: at most 7.0e-14 over D = 5 ... 200; 6.6e-14 at D = 257, 8.0e-14 at
513, 1.52e-13 at 769 ((2, 3); 8.0e-14 at (1, 1)) and 9.2e-14 at 1024, on states up to 14.4.  250 x 1.52e-13 = 3.8e-11 is
past TOL, so the wide shapes take TOL_WIDE = 3.8e-11 with the same 250-fold margin; the older tests keep TOL."""
import numpy as np

TOL = 1e-11
TOL_WIDE = 3.8e-11
K_TRUE, DT, STEPS = 8.17, 0.025, 40


def l96(t, x, p, st=None):
    return np.roll(x, 1) * (np.roll(x, -1) - np.roll(x, 2)) - x + p


def rk4(f, x0, p, n_steps, dt, t0=0.0, substeps=1, every=1, stim=None, dtype=np.float64):
    """f(t, x (D,), p, stimulus row or None) -> (D,).  Returns (n_steps // every + 1, D): steps 0, every, ...
    dtype=np.longdouble carries the integration in extended precision (derive(); no stimulus there)."""
    h = dtype(dt) / dtype(substeps)
    x = np.array(x0, dtype=dtype)
    out = [x.copy()]

    def st(n, s, c):
        if stim is None:
            return None
        w = (s + c) / substeps
        return (1.0 - w) * stim[n] + w * stim[n + 1]
    for n in range(n_steps):
        for s in range(substeps):
            q = n * substeps + s
            k1 = f(t0 + (q + 0.0) * h, x, p, st(n, s, 0.0))
            k2 = f(t0 + (q + 0.5) * h, x + 0.5 * h * k1, p, st(n, s, 0.5))
            k3 = f(t0 + (q + 0.5) * h, x + 0.5 * h * k2, p, st(n, s, 0.5))
            k4 = f(t0 + (q + 1.0) * h, x + h * k3, p, st(n, s, 1.0))
            x = x + h / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
        if (n + 1) % every == 0:
            out.append(x.copy())
    return np.array(out)


_starts = {}


def attractor_starts(D, T, k=K_TRUE):
    """T states on the Lorenz-96 attractor: a 400-step spin-up from a perturbed fixed point, then 25 steps apart"""
    if (D, T, k) not in _starts:
        rng = np.random.RandomState(100 + D)
        x = k * np.ones(D) + 0.01 * rng.randn(D)
        x = rk4(l96, x, k, 400, DT)[-1]
        xs = [x]
        for _ in range(T - 1):
            xs.append(rk4(l96, xs[-1], k, 25, DT)[-1])
        _starts[(D, T, k)] = np.array(xs)
        _starts[(D, T, k)].setflags(write=False)
    return _starts[(D, T, k)]


_refs = {}


def l96_reference(D, T, substeps=1, every=1, ks=None):
    """(x0 (T, D), reference (T, n_out, D)) for STEPS steps of DT; ks: one forcing per trajectory (default K_TRUE)"""
    key = (D, T, substeps, every, None if ks is None else tuple(ks))
    if key not in _refs:
        x0 = attractor_starts(D, T)
        kk = [K_TRUE] * T if ks is None else list(ks)
        ref = np.array([rk4(l96, x0[i], kk[i], STEPS, DT, substeps=substeps, every=every) for i in range(T)])
        ref.setflags(write=False)
        _refs[key] = (x0, ref)
    return _refs[key]


def derive(widths=(5, 20, 64, 67, 200, 257, 513, 769, 1024), T=7):
    """the figures of the docstring: float64 against longdouble, absolute, per width and (substeps, every)"""
    worst = {}
    for D in widths:
        x0 = attractor_starts(D, T)
        for substeps, every in ((1, 1), (2, 3)):
            e, big = 0.0, 0.0
            for i in range(T):
                a = rk4(l96, x0[i], K_TRUE, STEPS, DT, substeps=substeps, every=every)
                b = rk4(l96, x0[i], K_TRUE, STEPS, DT, substeps=substeps, every=every, dtype=np.longdouble)
                e = max(e, float(np.abs(np.asarray(a, dtype=np.longdouble) - b).max()))
                big = max(big, float(np.abs(b).max()))
            worst[(D, substeps, every)] = e
            print("D=%d substeps=%d every=%d  float64 vs longdouble, absolute: %.2e  largest state %.3g" % (D, substeps, every, e, big))
    return worst


if __name__ == "__main__":
    w = derive()
    print("largest %.2e  x 250 = %.2e  (TOL %.1e)" % (max(w.values()), 250 * max(w.values()), TOL))
