"""The adjoint predictor's reference: the transpose of the tangent-linear RK4 map in NumPy, written from the rule
csrc/va_predict_adj.h states (shared by tests/test_predict_adj_cpu.py, tests/test_gpu_predict_adj.py and
tests/test_gpu_shoot.py).

    forward, per RK4 step of h = dt / substeps:  X1 = x, X2 = x + h/2 k1, X3 = x + h/2 k2, X4 = x + h k3, all kept
    backward, with the cotangent l+ of the step's result:
        k4~ = h/6 l+                 X4~ = J(X4)^T k4~    gp += (df/dp)(X4)^T k4~
        k3~ = h/3 l+ + h   X4~       X3~ = J(X3)^T k3~    gp += (df/dp)(X3)^T k3~
        k2~ = h/3 l+ + h/2 X3~       X2~ = J(X2)^T k2~    gp += (df/dp)(X2)^T k2~
        k1~ = h/6 l+ + h/2 X2~       X1~ = J(x)^T  k1~    gp += (df/dp)(x)^T  k1~
        l   = l+ + X1~ + X2~ + X3~ + X4~
    l takes an output row's cotangent before the step below that row; row 0's is added to the result.
    misfit: G = 2 w (out[:, Lidx] - Y) at the observed columns, cost = sum w (out[:, Lidx] - Y)^2

A coding slip here cannot hide: self_check() verifies <G, dX> = <gx0, v_x> + <gp, v_p> against _tlm_ref.tlm_rk4 (itself
checked against the complex step of _predict_ref.rk4) in longdouble, once per process, before any reference leaves this
module.

TOL_ADJ: |device or host C++ - NumPy| <= TOL_ADJ max|row|, where a row is one gx0 (D entries of one trajectory and cotangent
set) or one gp (NPest entries).  Derived as _tlm_ref.TOL is: derive() runs adj_rk4 in float64 and in longdouble for 40 steps
of dt = 0.025 from 7 attractor states with 3 sets of standard normal cotangents on every output row at D = 5, 20, 64, 67
and both (substeps, every) pairs the tests use; the largest difference relative to the row's largest entry is 2.05e-13
(D = 20, substeps = 2, every = 3; between 9.9e-15 and 2.05e-13 over the cases: a gp row is ONE entry, a sum over all
steps and columns that may cancel, so its relative error is the larger one).  The project's 250-fold margin for FMA
contraction and summation order gives 5.1e-11.  The gradients grow backward along the horizon as the tangents grow forward
(entries of 10 to 60 from unit cotangents), hence relative per row.  A wrong coefficient, a stage cotangent applied at
another stage's linearisation point, or a row's cotangent taken a step late shows at 1e-4 or worse.  Do not lengthen the
horizon without deriving this again.

The wide shapes of _forecast_shapes.SLOTS_WIDE ((D, ncot) = (33, 2) ... (1024, 1), 3 attractor states, cotangent mode) keep
TOL_ADJ: derive_wide() measures between 4.5e-15 and 1.49e-13 (D = 200, substeps = 1; 7.7e-14 at D = 100, 1.8e-14 at D = 1024;
gx0 entries up to 615), and 250 x 1.49e-13 = 3.7e-11 stays under 5.1e-11.

TOL_ADJ_MISFIT_WIDE: misfit mode at D = 300 and 1024 (misfit_inputs(): every third column observed, (substeps, every) =
(2, 3)), used by the tests of those two shapes only.  There the cotangents 2 w (x - y) are the observation noise, and the
one-entry gp row sums them over all steps and columns with more cancellation than standard normal cotangents leave:
derive_wide() measures, over cost, gx0 rows and gp rows, 1.32e-12 at D = 300 and 3.3e-13 at D = 1024.  250 x 1.32e-12 =
3.3e-10 is past TOL_ADJ, so these two calls take 3.3e-10 with the same 250-fold margin.

The transpose identity <G, dX_c> = <gx0, v_x> + gp v_p, relative to |G| |dX_c| as test_transpose_of_the_tangent_kernel forms
it, keeps that test's TOL + TOL_ADJ = 5.9e-11 at the wide shapes: derive_transpose() finds the float64 reference pair off by
4.5e-18 (D = 1024) to 6.9e-17 (D = 33) with the sums in float64, the longdouble pair by 4e-21 to 4e-20 (the references are
transposes of each other; what the float64 pair leaves is rounding), and 250 x 6.9e-17 = 1.7e-14 is far under 5.9e-11."""
import numpy as np

import _tlm_ref
from _predict_ref import DT, K_TRUE, STEPS, attractor_starts, l96

TOL_ADJ = 5.1e-11
TOL_ADJ_MISFIT_WIDE = 3.3e-10


def l96_vjp(t, x, p, st, s):
    """J(x)^T s for s (ncot, D): (J^T s)_j = s_{j+1} (x_{j+2} - x_{j-1}) + s_{j-1} x_{j-2} - s_{j+2} x_{j+1} - s_j"""
    r = lambda a, k: np.roll(a, k, -1)
    return r(s, -1) * (r(x, -2) - r(x, 1)) + r(s, 1) * r(x, 2) - r(s, -2) * r(x, -1) - s


def l96_pgrad(t, x, p, st, s):
    """(df/dp)^T s, (ncot, 1): the forcing enters every column with derivative 1"""
    return s.sum(axis=-1, keepdims=True)


def adj_rk4(f, vjp, pgrad, x0, p, G, n_steps, dt, t0=0.0, substeps=1, every=1, stim=None, dtype=np.float64, npe=1):
    """G (ncot, n_out, D): cotangents of the output rows.  f as _predict_ref.rk4 takes it; vjp(t, x, p, stimulus row,
    s (ncot, D)) -> (ncot, D); pgrad(...) -> (ncot, npe).  Returns (out (n_out, D), gx0 (ncot, D), gp (ncot, npe))."""
    one, half, two, three, six = (dtype(v) for v in (1.0, 0.5, 2.0, 3.0, 6.0))
    h = dtype(dt) / dtype(substeps)
    x = np.array(x0, dtype=dtype)
    p = np.asarray(p, dtype=dtype)
    G = np.array(G, dtype=dtype)
    ncot = G.shape[0]

    def st(n, s, c):
        if stim is None:
            return None
        w = dtype(s + c) / dtype(substeps)
        return (one - w) * stim[n] + w * stim[n + 1]
    out, tape = [x.copy()], []
    for n in range(n_steps):
        for s in range(substeps):
            q = n * substeps + s
            ta, tb, tc = dtype(t0) + dtype(q) * h, dtype(t0) + (dtype(q) + half) * h, dtype(t0) + (dtype(q) + one) * h
            sa, sb, sc = st(n, s, 0.0), st(n, s, 0.5), st(n, s, 1.0)
            k1 = f(ta, x, p, sa)
            x2 = x + half * h * k1
            k2 = f(tb, x2, p, sb)
            x3 = x + half * h * k2
            k3 = f(tb, x3, p, sb)
            x4 = x + h * k3
            k4 = f(tc, x4, p, sc)
            tape.append(((ta, x, sa), (tb, x2, sb), (tb, x3, sb), (tc, x4, sc)))
            x = x + h / six * (k1 + two * k2 + two * k3 + k4)
        if (n + 1) % every == 0:
            out.append(x.copy())
    out = np.array(out)
    assert G.shape == (ncot,) + out.shape, (G.shape, out.shape)
    lam = np.zeros((ncot, x.size), dtype=dtype)
    gp = np.zeros((ncot, npe), dtype=dtype)
    if n_steps % every == 0:
        lam = lam + G[:, n_steps // every]
    for n in range(n_steps - 1, -1, -1):
        for s in range(substeps - 1, -1, -1):
            (ta, x1, sa), (tb, x2, sb), (_, x3, _), (tc, x4, sc) = tape[n * substeps + s]
            k4t = h / six * lam
            X4 = vjp(tc, x4, p, sc, k4t)
            gp = gp + pgrad(tc, x4, p, sc, k4t)
            k3t = h / three * lam + h * X4
            X3 = vjp(tb, x3, p, sb, k3t)
            gp = gp + pgrad(tb, x3, p, sb, k3t)
            k2t = h / three * lam + half * h * X3
            X2 = vjp(tb, x2, p, sb, k2t)
            gp = gp + pgrad(tb, x2, p, sb, k2t)
            k1t = h / six * lam + half * h * X2
            X1 = vjp(ta, x1, p, sa, k1t)
            gp = gp + pgrad(ta, x1, p, sa, k1t)
            lam = lam + X1 + X2 + X3 + X4
        if n % every == 0:
            lam = lam + G[:, n // every]
    return out, lam, gp


def misfit_cotangent(out, Y, Lidx, w):
    """(G (1, n_out, D), cost) of cost = sum w_l (out[:, Lidx_l] - Y_l)^2"""
    d = out[:, list(Lidx)] - Y
    G = np.zeros((1,) + out.shape, dtype=out.dtype)
    G[0][:, list(Lidx)] = 2.0 * np.asarray(w) * d
    return G, float((np.asarray(w) * d * d).sum())


def misfit_rk4(f, vjp, pgrad, x0, p, Y, Lidx, w, n_steps, dt, **kw):
    """(cost, gx0 (D,), gp (npe,), out): the misfit and its gradient with respect to x0 and the parameters"""
    from _predict_ref import rk4
    fw = {k: v for k, v in kw.items() if k in ("t0", "substeps", "every", "stim")}
    out = rk4(f, x0, p, n_steps, dt, **fw)
    G, cost = misfit_cotangent(out, Y, Lidx, w)
    _, gx0, gp = adj_rk4(f, vjp, pgrad, x0, p, G, n_steps, dt, **kw)
    return cost, gx0[0], gp[0], out


def row_error(got, ref):
    return _tlm_ref.row_error(got, ref)


def cotangents(D, T, ncot, n_out, seed=1):
    """the cases' cotangents: standard normal on every output row.  (seed = 0 holds one set at D = 67 whose single-entry gp
    row cancels to 2.8e-4 from terms of size 50: relative to that row the float64 reference itself is only good to 3.9e-10,
    which would have set TOL_ADJ to 9.8e-8 for every case.)"""
    return np.random.RandomState(1000 * D + 10 * ncot + seed).randn(T, ncot, n_out, D)


_checked = []


def self_check():
    """<G, dX> = <gx0, v_x> + <gp, v_p> against _tlm_ref.tlm_rk4 in longdouble: D = 7, three directions, two cotangent
    sets, both (substeps, every) pairs.  Returns the largest defect relative to |G| |dX|."""
    if _checked:
        return _checked[0]
    _tlm_ref.self_check()
    ld = np.longdouble
    D = 7
    x0 = attractor_starts(D, 2)[1]
    rng = np.random.RandomState(6)
    V = np.vstack([np.eye(D + 1)[3], np.eye(D + 1)[D], rng.randn(D + 1)])
    worst = 0.0
    for substeps, every in ((1, 1), (2, 3)):
        _, dX = _tlm_ref.tlm_rk4(l96, _tlm_ref.l96_jvp, x0, K_TRUE, V, STEPS, DT, substeps=substeps, every=every, dtype=ld)
        G = rng.randn(2, dX.shape[1], D)
        _, gx0, gp = adj_rk4(l96, l96_vjp, l96_pgrad, x0, K_TRUE, G, STEPS, DT, substeps=substeps, every=every, dtype=ld)
        for c in range(len(V)):
            for g in range(2):
                lhs = (np.asarray(G[g], dtype=ld) * dX[c]).sum()
                rhs = (gx0[g] * V[c, :D]).sum() + gp[g, 0] * V[c, D]
                worst = max(worst, float(abs(lhs - rhs) / (np.linalg.norm(G[g]) * np.linalg.norm(np.asarray(dX[c], dtype=np.float64)))))
    assert worst <= 1e-16, "the adjoint reference is not the transpose of the tangent-linear reference: %.3e" % worst
    _checked.append(worst)
    return worst


_refs = {}


def l96_adj_reference(D, T, ncot, substeps=1, every=1, ks=None):
    """(x0 (T, D), G (T, ncot, n_out, D), out (T, n_out, D), gx0 (T, ncot, D), gp (T, ncot, 1)) for STEPS steps of DT"""
    self_check()
    key = (D, T, ncot, substeps, every, None if ks is None else tuple(ks))
    if key not in _refs:
        x0 = attractor_starts(D, T)
        kk = [K_TRUE] * T if ks is None else list(ks)
        G = cotangents(D, T, ncot, STEPS // every + 1)
        res = [adj_rk4(l96, l96_vjp, l96_pgrad, x0[i], kk[i], G[i], STEPS, DT, substeps=substeps, every=every) for i in range(T)]
        arrs = (x0, G) + tuple(np.array([r[k] for r in res]) for k in range(3))
        for a in arrs[1:]:
            a.setflags(write=False)
        _refs[key] = arrs
    return _refs[key]


def derive(widths=(5, 20, 64, 67), T=7, ncot=3):
    """the figures of the docstring: float64 against longdouble, per width and (substeps, every)"""
    worst = {}
    for D in widths:
        x0 = attractor_starts(D, T)
        for substeps, every in ((1, 1), (2, 3)):
            G = cotangents(D, T, ncot, STEPS // every + 1)
            e, big = 0.0, 0.0
            for i in range(T):
                a = adj_rk4(l96, l96_vjp, l96_pgrad, x0[i], K_TRUE, G[i], STEPS, DT, substeps=substeps, every=every)
                b = adj_rk4(l96, l96_vjp, l96_pgrad, x0[i], K_TRUE, G[i], STEPS, DT, substeps=substeps, every=every, dtype=np.longdouble)
                for k in (1, 2):
                    e = max(e, row_error(np.asarray(a[k], dtype=np.longdouble), b[k]))
                big = max(big, float(np.abs(b[1]).max()))
            worst[(D, substeps, every)] = e
            print("D=%d substeps=%d every=%d  float64 vs longdouble, relative per row: %.2e  largest gx0 entry %.3g" % (D, substeps, every, e, big))
    return worst


def misfit_inputs(D, T, substeps=2, every=3):
    """misfit mode at a wide shape: (x0 (T, D), Lidx: every third column, w (L,), Y (T, n_out, L): the NumPy trajectory's
    observed columns + 0.3 randn)"""
    from _predict_ref import l96_reference
    x0, ref_x = l96_reference(D, T, substeps, every)
    Lidx = list(range(0, D, 3))
    rng = np.random.RandomState(40 + D)
    w = (0.5 + rng.rand(len(Lidx))) / len(Lidx)
    return x0, Lidx, w, ref_x[:, :, Lidx] + 0.3 * rng.randn(T, ref_x.shape[1], len(Lidx))


def derive_wide(misfit_widths=(300, 1024)):
    """the same figure at the wide shapes of _forecast_shapes.SLOTS_WIDE with their T = 3, and in misfit mode (cost,
    gx0, gp relative) at misfit_widths"""
    import _forecast_shapes as fs
    ld = np.longdouble
    worst = {}
    for (D, ncot), _, _ in fs.SLOTS_WIDE:
        x0 = attractor_starts(D, fs.T)
        for substeps, every in ((1, 1), (2, 3)):
            G = cotangents(D, fs.T, ncot, STEPS // every + 1)
            e, big = 0.0, 0.0
            for i in range(fs.T):
                a = adj_rk4(l96, l96_vjp, l96_pgrad, x0[i], K_TRUE, G[i], STEPS, DT, substeps=substeps, every=every)
                b = adj_rk4(l96, l96_vjp, l96_pgrad, x0[i], K_TRUE, G[i], STEPS, DT, substeps=substeps, every=every, dtype=ld)
                for k in (1, 2):
                    e = max(e, row_error(np.asarray(a[k], dtype=ld), b[k]))
                big = max(big, float(np.abs(b[1]).max()))
            worst[(D, ncot, substeps, every)] = e
            print("D=%d ncot=%d substeps=%d every=%d  float64 vs longdouble, relative per row: %.2e  largest gx0 entry %.3g"
                  % (D, ncot, substeps, every, e, big))
    for D in misfit_widths:
        x0, Lidx, w, Y = misfit_inputs(D, fs.T)
        e = 0.0
        for i in range(fs.T):
            out = rk4_ld(x0[i], 2, 3)
            Gl, cl = misfit_cotangent(out, np.asarray(Y[i], dtype=ld), Lidx, np.asarray(w, dtype=ld))
            _, gl, ql = adj_rk4(l96, l96_vjp, l96_pgrad, x0[i], K_TRUE, Gl, STEPS, DT, substeps=2, every=3, dtype=ld)
            c, g, q, _ = misfit_rk4(l96, l96_vjp, l96_pgrad, x0[i], K_TRUE, Y[i], Lidx, w, STEPS, DT, substeps=2, every=3)
            e = max(e, abs(c - cl) / cl, row_error(np.asarray(g, dtype=ld), gl[0]), row_error(np.asarray(q, dtype=ld), ql[0]))
        worst[(D, "misfit")] = float(e)
        print("D=%d misfit mode (2, 3)  float64 vs longdouble, cost and gradient rows relative: %.2e" % (D, e))
    return worst


def rk4_ld(x0, substeps, every):
    from _predict_ref import rk4
    return rk4(l96, x0, K_TRUE, STEPS, DT, substeps=substeps, every=every, dtype=np.longdouble)


def derive_transpose():
    """the transpose identity at the wide shapes, as the tests form it: <G, dX_c> - (<gx0, v_x> + gp v_p) relative to
    |G| |dX_c| with the float64 reference pair (sums in float64), beside the same defect of the pair in longdouble (which
    shows that what the float64 pair leaves is rounding, not a property of the references)"""
    import _forecast_shapes as fs
    ld = np.longdouble
    worst = {}
    for (D, n), _, _ in fs.SLOTS_WIDE:
        x0, V = attractor_starts(D, fs.T), fs.directions(D, n)
        substeps, every = 2, 3
        G = cotangents(D, fs.T, n, STEPS // every + 1)
        e, el = 0.0, 0.0
        for i in range(fs.T):
            for dt_, which in ((np.float64, 0), (ld, 1)):
                _, dX = _tlm_ref.tlm_rk4(l96, _tlm_ref.l96_jvp, x0[i], K_TRUE, V, STEPS, DT, substeps=substeps, every=every, dtype=dt_)
                _, gx0, gp = adj_rk4(l96, l96_vjp, l96_pgrad, x0[i], K_TRUE, G[i], STEPS, DT, substeps=substeps, every=every, dtype=dt_)
                Gi, Vi = np.asarray(G[i], dtype=dt_), np.asarray(V, dtype=dt_)
                for g in range(n):
                    for c in range(n):
                        d = abs((Gi[g] * dX[c]).sum() - ((gx0[g] * Vi[c, :D]).sum() + gp[g, 0] * Vi[c, D]))
                        d = float(d / (np.linalg.norm(G[i, g]) * np.linalg.norm(np.asarray(dX[c], dtype=np.float64))))
                        if which:
                            el = max(el, d)
                        else:
                            e = max(e, d)
        worst[(D, n)] = e
        print("D=%d n=%d (2, 3)  transpose defect relative to |G| |dX_c|: float64 pair %.2e, longdouble pair %.2e" % (D, n, e, el))
    return worst


if __name__ == "__main__":
    print("self check: %.2e" % self_check())
    w = derive()
    print("largest %.2e  x 250 = %.2e" % (max(w.values()), 250 * max(w.values())))
    w = derive_wide()
    print("wide shapes: largest %.2e  x 250 = %.2e  (TOL_ADJ %.1e)" % (max(w.values()), 250 * max(w.values()), TOL_ADJ))
    w = derive_transpose()
    print("transpose identity: largest %.2e  x 250 = %.2e  (TOL + TOL_ADJ %.1e)" % (max(w.values()), 250 * max(w.values()), _tlm_ref.TOL + TOL_ADJ))
