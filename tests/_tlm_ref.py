"""The forecast spread's reference: the tangent-linear model of classical RK4 in NumPy, written from the rule
csrc/va_predict_tlm.h states (shared by tests/test_predict_tlm_cpu.py and tests/test_gpu_predict_tlm.py).

    k1 = f(x)            k1' = jvp(x;            v_x,             v_p)
    k2 = f(x + h/2 k1)   k2' = jvp(x + h/2 k1;   v_x + h/2 k1',   v_p)
    k3 = f(x + h/2 k2)   k3' = jvp(x + h/2 k2;   v_x + h/2 k2',   v_p)
    k4 = f(x + h k3)     k4' = jvp(x + h k3;     v_x + h k3',     v_p)
    x += h/6 (k1 + 2 k2 + 2 k3 + k4),  v_x += h/6 (k1' + 2 k2' + 2 k3' + k4'),  v_p constant
    jvp(x; v, q) = J(x) v + (df/dp) q;  stage times and stimulus as in _predict_ref.py (the stimulus has no tangent)

For Lorenz-96 the Jacobian is analytic.  A coding slip here cannot hide: complex_step() differentiates
_predict_ref.rk4 itself (exact to rounding: no difference is formed), and self_check() compares the two once per
process before any reference leaves this module.

TOL: |device or host C++ - NumPy| <= TOL max|row|, where a row is the D tangent entries of one trajectory, one direction
and one output time -- tangents grow along the horizon (unit directions reach entries of 8 to 27 after 40 steps of
0.025), so the bound is relative per row.  Derived as _predict_ref.TOL is: derive() runs tlm_rk4 in float64 and in
longdouble for 40 steps of dt = 0.025 from 7 attractor states with the D + 1 directions (identity, forcing) at D = 5, 20,
64, 67, 200 and both (substeps, every) pairs the tests use; the largest difference relative to the row's largest entry is
3.12e-14 (D = 200, substeps = 1; between 4.1e-15 and 3.1e-14 over the cases).  The same 250-fold margin for FMA
contraction and summation order gives 7.8e-12.  A wrong coefficient or stage time, or a tangent stage that reads the
nominal input of another stage, shows at 1e-4 or worse.  Do not lengthen the horizon without deriving this again.

The wide shapes of _forecast_shapes.SLOTS_WIDE ((D, nvec) = (33, 2) ... (1024, 1), 3 attractor states, the mixed random
directions of _forecast_shapes.directions) keep TOL: derive_wide() measures between 3.8e-15 and 2.71e-14 (D = 700,
substeps = 1; 2.5e-14 at D = 513, 2.0e-14 at D = 1024; tangent entries up to 175), and 250 x 2.71e-14 = 6.8e-12 stays
under 7.8e-12."""
import numpy as np

from _predict_ref import DT, K_TRUE, STEPS, attractor_starts, l96, rk4

TOL = 7.8e-12


def l96_jvp(t, x, p, st, vx, vp):
    """J(x) vx + (df/dp) vp for vx (..., D), vp (..., 1): the forcing enters every column with derivative 1"""
    r = lambda a, k: np.roll(a, k, -1)
    return r(vx, 1) * (r(x, -1) - r(x, 2)) + r(x, 1) * (r(vx, -1) - r(vx, 2)) - vx + vp


def tlm_rk4(f, jvp, x0, p, V, n_steps, dt, t0=0.0, substeps=1, every=1, stim=None, dtype=np.float64):
    """V (nvec, D + NPe): directions [state part | parameter part].  f as _predict_ref.rk4 takes it; jvp(t, x, p,
    stimulus row, vx (nvec, D), vp (nvec, NPe)) -> (nvec, D).  Returns (out (n_out, D), dX (nvec, n_out, D))."""
    one = dtype(1.0)
    h = dtype(dt) / dtype(substeps)
    x = np.array(x0, dtype=dtype)
    D = x.size
    V = np.array(V, dtype=dtype)
    vx, vp = V[:, :D].copy(), V[:, D:]
    p = np.asarray(p, dtype=dtype)
    out, dX = [x.copy()], [vx.copy()]

    def st(n, s, c):
        if stim is None:
            return None
        w = dtype(s + c) / dtype(substeps)
        return (one - w) * stim[n] + w * stim[n + 1]
    half, two, six = dtype(0.5), dtype(2.0), dtype(6.0)
    for n in range(n_steps):
        for s in range(substeps):
            q = n * substeps + s
            ta, tb, tc = dtype(t0) + dtype(q) * h, dtype(t0) + (dtype(q) + half) * h, dtype(t0) + (dtype(q) + one) * h
            sa, sb, sc = st(n, s, 0.0), st(n, s, 0.5), st(n, s, 1.0)
            k1, d1 = f(ta, x, p, sa), jvp(ta, x, p, sa, vx, vp)
            x2, v2 = x + half * h * k1, vx + half * h * d1
            k2, d2 = f(tb, x2, p, sb), jvp(tb, x2, p, sb, v2, vp)
            x3, v3 = x + half * h * k2, vx + half * h * d2
            k3, d3 = f(tb, x3, p, sb), jvp(tb, x3, p, sb, v3, vp)
            x4, v4 = x + h * k3, vx + h * d3
            k4, d4 = f(tc, x4, p, sc), jvp(tc, x4, p, sc, v4, vp)
            x = x + h / six * (k1 + two * k2 + two * k3 + k4)
            vx = vx + h / six * (d1 + two * d2 + two * d3 + d4)
        if (n + 1) % every == 0:
            out.append(x.copy())
            dX.append(vx.copy())
    return np.array(out), np.array(dX).transpose(1, 0, 2)


def complex_step(f, x0, p, vx, vp_full, n_steps, dt, eps=1e-30, dtype=np.float64, **kw):
    """d/d eps of _predict_ref.rk4(f, x0 + eps vx, p + eps vp_full) at eps = 0, (n_out, D), by the complex step.  rk4
    takes a real start, so the state's perturbation rides in f: z = x - i eps vx starts real and obeys z' = f(z + i eps vx),
    and RK4 commutes with the constant shift.  dtype=np.longdouble carries the whole integration in extended precision
    (the complex parameters promote it)."""
    vx = np.asarray(vx, dtype=dtype)
    shift = 1j * dtype(eps) * vx
    pc = np.asarray(p, dtype=dtype) + 1j * dtype(eps) * np.asarray(vp_full, dtype=dtype)
    z = rk4(lambda t, y, pp, st: f(t, y + shift, pp, st), x0, pc, n_steps, dt, **kw)
    return z.imag / dtype(eps) + vx


def identity_directions(D):
    """the D + 1 directions of the Lorenz-96 cases: a unit vector per state, then the forcing alone"""
    return np.eye(D + 1)


def row_error(got, ref):
    """largest |got - ref| of a row of D entries relative to the row's largest |ref|, over all rows; a row of zeros (the
    forcing direction's state part at row 0) has to be met exactly"""
    err, scale = np.abs(got - ref).max(axis=-1), np.abs(ref).max(axis=-1)
    rel = np.where(scale > 0, err / np.where(scale > 0, scale, 1.0), np.where(err > 0, np.inf, 0.0))
    return float(rel.max())


def ordered_sums(dX):
    """var and cov as k_spread forms them: products and sums rounded one by one, in direction order"""
    var = np.zeros(dX.shape[:1] + dX.shape[2:])
    cov = np.zeros(dX.shape[:1] + dX.shape[2:] + dX.shape[-1:])
    for c in range(dX.shape[1]):
        var = var + dX[:, c] * dX[:, c]
        cov = cov + dX[:, c, :, :, None] * dX[:, c, :, None, :]
    return var, cov


_checked = []


def self_check():
    """tlm_rk4 with the analytic Jacobian against the complex-step derivative of _predict_ref.rk4: D = 7, a state
    direction, the forcing direction and a mixed one, both (substeps, every) pairs"""
    if _checked:
        return _checked[0]
    D = 7
    x0 = attractor_starts(D, 2)[1]
    rng = np.random.RandomState(5)
    V = np.vstack([np.eye(D + 1)[2], np.eye(D + 1)[D], rng.randn(D + 1)])
    worst = 0.0
    for substeps, every in ((1, 1), (2, 3)):
        _, dX = tlm_rk4(l96, l96_jvp, x0, K_TRUE, V, STEPS, DT, substeps=substeps, every=every)
        for c in range(len(V)):
            cs = complex_step(l96, x0, K_TRUE, V[c, :D], V[c, D], STEPS, DT, substeps=substeps, every=every)
            worst = max(worst, row_error(dX[c], cs))
    assert worst <= 1e-13, "the tangent-linear reference disagrees with the complex-step derivative of rk4: %.3e" % worst
    _checked.append(worst)
    return worst


_refs = {}


def l96_tlm_reference(D, T, substeps=1, every=1, ks=None, V=None):
    """(x0 (T, D), V0 (T, nvec, D + 1), out (T, n_out, D), dX (T, nvec, n_out, D)) for STEPS steps of DT; ks: one forcing
    per trajectory (default K_TRUE); V (nvec, D + 1): the directions of every trajectory (default identity_directions)"""
    self_check()
    key = (D, T, substeps, every, None if ks is None else tuple(ks), None if V is None else np.asarray(V).tobytes())
    if key not in _refs:
        x0 = attractor_starts(D, T)
        kk = [K_TRUE] * T if ks is None else list(ks)
        Vd = identity_directions(D) if V is None else np.asarray(V, dtype=np.float64)
        res = [tlm_rk4(l96, l96_jvp, x0[i], kk[i], Vd, STEPS, DT, substeps=substeps, every=every) for i in range(T)]
        V0 = np.ascontiguousarray(np.broadcast_to(Vd, (T,) + Vd.shape))
        out, dX = np.array([r[0] for r in res]), np.array([r[1] for r in res])
        for a in (V0, out, dX):
            a.setflags(write=False)
        _refs[key] = (x0, V0, out, dX)
    return _refs[key]


def derive(widths=(5, 20, 64, 67, 200), T=7):
    """the figures of the docstring: float64 against longdouble, per width and (substeps, every)"""
    worst = {}
    for D in widths:
        x0 = attractor_starts(D, T)
        for substeps, every in ((1, 1), (2, 3)):
            e = 0.0
            for i in range(T):
                a = tlm_rk4(l96, l96_jvp, x0[i], K_TRUE, identity_directions(D), STEPS, DT, substeps=substeps, every=every)[1]
                b = tlm_rk4(l96, l96_jvp, x0[i], K_TRUE, identity_directions(D), STEPS, DT, substeps=substeps, every=every,
                            dtype=np.longdouble)[1]
                e = max(e, row_error(np.asarray(a, dtype=np.longdouble), b))
            worst[(D, substeps, every)] = e
            print("D=%d substeps=%d every=%d  float64 vs longdouble, relative per row: %.2e  largest tangent entry %.3g"
                  % (D, substeps, every, e, float(np.abs(b).max())))
    return worst


def derive_wide():
    """the same figure at the wide shapes of _forecast_shapes.SLOTS_WIDE with their mixed directions and their T = 3"""
    import _forecast_shapes as fs
    worst = {}
    for (D, nvec), _, _ in fs.SLOTS_WIDE:
        x0, V = attractor_starts(D, fs.T), fs.directions(D, nvec)
        for substeps, every in ((1, 1), (2, 3)):
            e = 0.0
            for i in range(fs.T):
                a = tlm_rk4(l96, l96_jvp, x0[i], K_TRUE, V, STEPS, DT, substeps=substeps, every=every)[1]
                b = tlm_rk4(l96, l96_jvp, x0[i], K_TRUE, V, STEPS, DT, substeps=substeps, every=every, dtype=np.longdouble)[1]
                e = max(e, row_error(np.asarray(a, dtype=np.longdouble), b))
            worst[(D, nvec, substeps, every)] = e
            print("D=%d nvec=%d substeps=%d every=%d  float64 vs longdouble, relative per row: %.2e  largest tangent entry %.3g"
                  % (D, nvec, substeps, every, e, float(np.abs(b).max())))
    return worst


if __name__ == "__main__":
    print("self check: %.2e" % self_check())
    w = derive()
    print("largest %.2e  x 250 = %.2e" % (max(w.values()), 250 * max(w.values())))
    w = derive_wide()
    print("wide shapes, mixed directions: largest %.2e  x 250 = %.2e  (TOL %.1e)" % (max(w.values()), 250 * max(w.values()), TOL))
