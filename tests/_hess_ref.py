"""Reference Hessians of the action for the tests of hess_vec (TEST INFRASTRUCTURE): the action of
oracle.va_oracle.numpy_action_generic on an object array of SymPy symbols, differentiated twice and lambdified; the
Gauss-Newton Hessian 2 J^T W J from a residual list written here and checked against that action.  Built once per
case and process (functools.lru_cache) and shared by the CPU and GPU tests; nothing here is modified by a test."""
import functools

import numpy as np
import sympy as sp

import va_oracle

DT = 0.025
REL = 1e-10          # the project's bound for derivatives against an exact reference (gradients vs the complex step)


def l96(t, x, p):
    return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - x + p[0]


def two_param_stencil(t, x, p):
    """a stencil whose two parameters multiply states: d2f/dxdp and the (x, p) cross terms are non-zero"""
    return p[0] * np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - p[1] * x * x + 8.0


def linear_model(t, x, p):
    """linear in state and parameter: the Gauss-Newton Hessian is the Hessian"""
    return 0.5 * np.roll(x, 1, 1) - 1.5 * x + 0.25 * np.roll(x, -2, 1) + p[0]


_tanh = np.frompyfunc(sp.tanh, 1, 1)


def nakl_sym(t, x, pstim):
    """tests/models/nakl.py with SymPy's tanh (object arrays of expressions have no numpy tanh)"""
    dxdt = np.zeros_like(x)
    p, Iext = pstim
    V, m, h, n = (x[:, 0], x[:, 1], x[:, 2], x[:, 3])
    xi = lambda Vt, Vs: 0.5 * (1.0 + _tanh((V - Vt) / Vs))
    xt = lambda Vt, Vs, t1, t2: t1 + t2 * (1.0 - _tanh((V - Vt) / Vs) ** 2)
    dxdt[:, 0] = p[0] * m ** 3 * h * (p[3] - V) + p[1] * n ** 4 * (p[4] - V) + p[2] * (p[5] - V) + Iext
    dxdt[:, 1] = (xi(p[6], p[7]) - m) / xt(p[6], p[7], p[8], p[9])
    dxdt[:, 2] = (xi(p[10], p[11]) - h) / xt(p[10], p[11], p[12], p[13])
    dxdt[:, 3] = (xi(p[14], p[15]) - n) / xt(p[14], p[15], p[16], p[17])
    return dxdt


class SymbolicAction(object):
    """A(xp) of one problem with exact first and second derivatives.  RF is the model-error weight WITH its rung's scale."""

    def __init__(self, f, D, N, Y, Lidx, dt, RM, RF, P, Pidx, disc, t_model=None, stim=None, nskip=1, gauss_newton=True):
        self.n = n = N * D + len(Pidx)
        self.kw = dict(D=D, N=N, Y=Y, Lidx=list(Lidx), dt=dt, RM=RM, RF=RF, NP=len(P), Pidx=list(Pidx), P=np.asarray(P, float),
                       disc=disc, t_model=t_model, stim=stim, nskip=nskip)
        self.f = f
        syms = sp.symbols("z0:%d" % n, real=True)
        XP = np.array(syms, dtype=object)
        A = self._action(XP)
        grad = [sp.diff(A, s) for s in syms]
        idx = {s: k for k, s in enumerate(syms)}
        self._hij, ent = [], []
        for i in range(n):
            for s in sorted(grad[i].free_symbols, key=lambda s: idx.get(s, -1)):
                j = idx[s]
                if j >= i:
                    e = sp.diff(grad[i], s)
                    if e != 0:
                        self._hij.append((i, j)); ent.append(e)
        self._A = sp.lambdify(syms, A, modules="math", cse=True)
        self._h = sp.lambdify(syms, ent, modules="math", cse=True)
        if gauss_newton:
            r, self._w = self._residuals(XP)
            self._r = sp.lambdify(syms, list(r), modules="math", cse=True)
            self._jij, jent = [], []
            for k, rk in enumerate(r):
                for s in rk.free_symbols:
                    self._jij.append((k, idx[s])); jent.append(sp.diff(rk, s))
            self._j = sp.lambdify(syms, jent, modules="math", cse=True)
            # the residual list is this file's own: it must reproduce the oracle's action
            z = np.random.RandomState(11).randn(n) + 1.0
            a0 = self.A(z)
            assert abs(np.dot(self._w, np.square(self._r(*z))) - a0) <= 1e-12 * abs(a0)

    def _action(self, XP):
        k = self.kw
        return va_oracle.numpy_action_generic(self.f, XP, k["D"], k["N"], k["Y"], k["Lidx"], k["dt"], k["RM"], k["RF"], k["NP"],
                                              k["Pidx"], k["P"], k["disc"], t_model=k["t_model"], stim=k["stim"], nskip=k["nskip"])[0]

    def _residuals(self, XP):
        """(r, w) with A = sum w r^2: the measurement residuals, then the discretisation's"""
        k = self.kw
        D, N, dt, Lidx, nskip = k["D"], k["N"], k["dt"], k["Lidx"], k["nskip"]
        x = XP[:N * D].reshape(N, D)
        p = np.array(k["P"], dtype=object)
        p[k["Pidx"]] = XP[N * D:]
        t = np.zeros(N) if k["t_model"] is None else np.asarray(k["t_model"])
        Y = k["Y"]
        r = list((x[::nskip, Lidx] - Y).ravel())
        RM = k["RM"]
        w = list((RM if isinstance(RM, np.ndarray) else np.full(Y.shape, RM)).ravel() / (len(Lidx) * Y.shape[0]))
        arg = (lambda sl: p) if k["stim"] is None else (lambda sl: (p, k["stim"][sl]))
        f = self.f
        RF = k["RF"]
        rf = RF if isinstance(RF, np.ndarray) else np.full((N - 1, D), RF)
        if k["disc"] == "SimpsonHermite":
            a, m_, b = slice(None, -2, 2), slice(1, -1, 2), slice(2, None, 2)
            fn, fmid, fnp1 = f(t[a], x[a], arg(a)), f(t[m_], x[m_], arg(m_)), f(t[b], x[b], arg(b))
            d1 = x[2::2] - x[:-2:2] - (fn + 4.0 * fmid + fnp1) * (2.0 * dt) / 6.0
            d2 = x[1::2] - ((x[a] + x[b]) / 2.0 + (fn - fnp1) * (2.0 * dt) / 8.0)
            r += list(d1.ravel()) + list(d2.ravel())
            w += list(rf[::2].ravel() / (D * (N - 1))) + list(rf[1::2].ravel() / (D * (N - 1)))
        else:
            a, b = slice(None, -1), slice(1, None)
            if k["disc"] == "trapezoid":
                d = x[1:] - x[:-1] - dt * (f(t[a], x[a], arg(a)) + f(t[b], x[b], arg(b))) / 2.0
            elif k["disc"] == "euler":
                d = x[1:] - x[:-1] - dt * f(t[a], x[a], arg(a))
            else:
                d = x[1:] - f(t[a], x[a], arg(a))
            r += list(d.ravel())
            w += list(rf.ravel() / (D * (N - 1)))
        return [sp.sympify(e) for e in r], np.array(w, dtype=float)

    def A(self, z):
        return float(self._A(*z))

    def hessian(self, z):
        H = np.zeros((self.n, self.n))
        for (i, j), v in zip(self._hij, self._h(*z)):
            H[i, j] = H[j, i] = v
        return H

    def gauss_newton(self, z):
        J = np.zeros((len(self._w), self.n))
        for (k, j), v in zip(self._jij, self._j(*z)):
            J[k, j] = v
        return 2.0 * np.dot(J.T, self._w[:, None] * J)


# ---------------------------------------------------------------------------------------------------------------
# the Lorenz-96 cases at D = 5 shared by tests/test_hvp_cpu.py and tests/test_gpu_hvp.py
L96_N = {"euler": 6, "forwardmap": 6, "trapezoid": 7, "SimpsonHermite": 7}
RF_SCALE = 3.0
NPTS, NVEC = 3, 4


@functools.lru_cache(maxsize=None)
def l96_case(disc, variant="plain"):
    """variant: 'plain' (scalar weights), 'nskip' (merr_nskip = 2 and an RM array), 'rfarr' (an RF array)"""
    D, N = 5, L96_N[disc]
    rng = np.random.RandomState({"plain": 100, "nskip": 200, "rfarr": 300}[variant] + len(disc))
    nskip = 2 if variant == "nskip" else 1
    Lidx, Pidx = [0, 2], [0]
    N_data = (N - 1) // nskip + 1
    Y = 3.0 * rng.randn(N_data, len(Lidx))
    RM = 4.0 * (0.5 + rng.rand(N_data, len(Lidx))) if variant == "nskip" else 4.0
    RF0 = 0.5 * (0.5 + rng.rand(N - 1, D)) if variant == "rfarr" else 0.5
    P = np.array([8.0])
    n = N * D + 1
    X = 3.0 * rng.randn(NPTS, n)
    X[:, -1] = 8.0 + rng.rand(NPTS)
    V = rng.randn(NPTS, NVEC, n)
    sa = SymbolicAction(l96, D, N, Y, Lidx, DT, RM, RF0 * RF_SCALE, P, Pidx, disc, nskip=nskip)
    H = np.array([sa.hessian(x) for x in X])
    Hgn = np.array([sa.gauss_newton(x) for x in X])
    for a in (X, V, H, Hgn, Y):
        a.setflags(write=False)
    return dict(D=D, N=N, disc=disc, nskip=nskip, Lidx=Lidx, Pidx=Pidx, Y=Y, RM=RM, RF0=RF0, P=P, X=X, V=V, H=H, Hgn=Hgn,
                rf_scale=RF_SCALE, dt=DT)


def rel_err(got, want):
    """max |got - want| / max |want|, per product vector (last axis), the largest of them"""
    got, want = np.asarray(got), np.asarray(want)
    return float((np.abs(got - want).max(axis=-1) / np.abs(want).max(axis=-1)).max())
