"""Reference Hessian-vector products of the action at any size (TEST INFRASTRUCTURE): the action of
oracle.va_oracle.numpy_action_generic restated array operation for array operation on torch float64 CPU tensors and
differentiated twice by reverse-mode autograd (grad with create_graph, then grad of g . v); the Gauss-Newton product
2 J^T (w o (J v)) from the residual list of _hess_ref.SymbolicAction._residuals restated here and checked against that
action.  Nothing of the kernel's hand-written tangent phases is shared with it.  tests/test_hess_torch_ref_cpu.py holds it
to 1e-12 against the SymPy Hessians of tests/_hess_ref.py (measured: at most 2.6e-15); the cases at the end are the ones
tests/test_hess_torch_ref_cpu.py (host run of the phases) and tests/test_gpu_hvp_geometry.py (device) share.  CPU tensors
only; nothing here is modified by a test."""
import functools

import numpy as np
import torch

import _hess_ref as hr

F64 = torch.float64


# ---------------------------------------------------------------------------------------------------------------
# the models of tests/_hess_ref.py and tests/models/nakl.py on tensors: f(t [rows], x [rows, D], p) -> [rows, D]
def l96(t, x, p):
    return torch.roll(x, 1, 1) * (torch.roll(x, -1, 1) - torch.roll(x, 2, 1)) - x + p[0]


def two_param_stencil(t, x, p):
    return p[0] * torch.roll(x, 1, 1) * (torch.roll(x, -1, 1) - torch.roll(x, 2, 1)) - p[1] * x * x + 8.0


def nakl(t, x, pstim):
    p, Iext = pstim
    V, m, h, n = (x[:, 0], x[:, 1], x[:, 2], x[:, 3])
    xi = lambda Vt, Vs: 0.5 * (1.0 + torch.tanh((V - Vt) / Vs))
    xt = lambda Vt, Vs, t1, t2: t1 + t2 * (1.0 - torch.tanh((V - Vt) / Vs) ** 2)
    return torch.stack([p[0] * m ** 3 * h * (p[3] - V) + p[1] * n ** 4 * (p[4] - V) + p[2] * (p[5] - V) + Iext,
                        (xi(p[6], p[7]) - m) / xt(p[6], p[7], p[8], p[9]),
                        (xi(p[10], p[11]) - h) / xt(p[10], p[11], p[12], p[13]),
                        (xi(p[14], p[15]) - n) / xt(p[14], p[15], p[16], p[17])], dim=1)


def _t(a):
    return torch.tensor(np.array(a, dtype=np.float64), dtype=F64)


class TorchAction(object):
    """A(z), z = [X | p_est], of one problem.  RM: a scalar or (N_data, L); RF: a scalar or (N - 1, D), WITH its rung's scale;
    Lidx in any order (column l of Y and RM belongs to Lidx[l]); P: the full parameter vector, which every call may
    replace (a point of its own fixed parameters); stim: (N,) as the oracle's stimulus tuple."""

    def __init__(self, f, D, N, Y, Lidx, dt, RM, RF, P, Pidx, disc, t_model=None, stim=None, nskip=1):
        self.f, self.D, self.N, self.dt, self.disc, self.nskip = f, D, N, float(dt), disc, nskip
        self.Lidx, self.Pidx = [int(l) for l in Lidx], torch.tensor([int(k) for k in Pidx], dtype=torch.long)
        self.n = N * D + len(Pidx)
        self.Y = _t(Y)
        assert self.Y.shape == ((N - 1) // nskip + 1, len(self.Lidx))
        self.RM = _t(RM) if isinstance(RM, np.ndarray) else float(RM)
        self.RF = _t(RF) if isinstance(RF, np.ndarray) else float(RF)
        assert not isinstance(RM, np.ndarray) or RM.shape == tuple(self.Y.shape)
        assert not isinstance(RF, np.ndarray) or RF.shape == (N - 1, D)
        self.P = _t(P)
        self.t = torch.zeros(N, dtype=F64) if t_model is None else _t(t_model)
        self.stim = None if stim is None else _t(stim)
        # the residual list is this file's own: it must reproduce the action
        z = np.random.RandomState(11).randn(self.n) + 1.0
        a0 = self.A(z)
        r, w = self._residuals(_t(z), self.P)
        assert abs(float((w * r * r).sum()) - a0) <= 1e-12 * abs(a0)

    # ------------------------------------------------------------------ the action, as the oracle writes it
    def _xp(self, z, P):
        ND = self.N * self.D
        p = torch.index_copy(P, 0, self.Pidx, z[ND:]) if len(self.Pidx) else P
        arg = (lambda sl: p) if self.stim is None else (lambda sl: (p, self.stim[sl]))
        return z[:ND].reshape(self.N, self.D), arg

    def _defects(self, x, arg):
        """the discretisation's residual arrays, and for each the rows of RF that weigh it"""
        f, t, dt = self.f, self.t, self.dt
        if self.disc == "SimpsonHermite":
            a, m_, b = slice(None, -2, 2), slice(1, -1, 2), slice(2, None, 2)
            fn, fmid, fnp1 = f(t[a], x[a], arg(a)), f(t[m_], x[m_], arg(m_)), f(t[b], x[b], arg(b))
            v1 = (fn + 4.0 * fmid + fnp1) * (2.0 * dt) / 6.0
            v2 = (x[a] + x[b]) / 2.0 + (fn - fnp1) * (2.0 * dt) / 8.0
            return [(x[2::2] - x[:-2:2] - v1, slice(None, None, 2)), (x[1::2] - v2, slice(1, None, 2))]
        a, b = slice(None, -1), slice(1, None)
        if self.disc == "trapezoid":
            d = x[1:] - x[:-1] - dt * (f(t[a], x[a], arg(a)) + f(t[b], x[b], arg(b))) / 2.0
        elif self.disc == "euler":
            d = x[1:] - x[:-1] - dt * f(t[a], x[a], arg(a))
        else:
            assert self.disc == "forwardmap"
            d = x[1:] - f(t[a], x[a], arg(a))
        return [(d, slice(None))]

    def _action(self, z, P):
        x, arg = self._xp(z, P)
        diff = x[::self.nskip][:, self.Lidx] - self.Y
        norm = len(self.Lidx) * self.Y.shape[0]
        me = (torch.sum(self.RM * diff * diff) if torch.is_tensor(self.RM) else self.RM * torch.sum(diff * diff)) / norm
        fe = 0.0
        for d, rows in self._defects(x, arg):
            fe = fe + (torch.sum(self.RF[rows] * d * d) if torch.is_tensor(self.RF) else self.RF * torch.sum(d * d))
        return me + fe / (self.D * (self.N - 1))

    def _residuals(self, z, P):
        """(r, w) with A = sum w r^2: the measurement residuals, then the discretisation's"""
        x, arg = self._xp(z, P)
        D, N = self.D, self.N
        r = [(x[::self.nskip][:, self.Lidx] - self.Y).reshape(-1)]
        norm = len(self.Lidx) * self.Y.shape[0]
        w = [(self.RM if torch.is_tensor(self.RM) else torch.full(self.Y.shape, self.RM, dtype=F64)).reshape(-1) / norm]
        rf = self.RF if torch.is_tensor(self.RF) else torch.full((N - 1, D), self.RF, dtype=F64)
        for d, rows in self._defects(x, arg):
            r.append(d.reshape(-1))
            w.append(rf[rows].reshape(-1) / (D * (N - 1)))
        return torch.cat(r), torch.cat(w)

    # ------------------------------------------------------------------ what the tests call (NumPy in, NumPy out)
    def _args(self, z, P):
        z = _t(z).requires_grad_(True)
        assert z.shape == (self.n,)
        return z, (self.P if P is None else _t(P))

    def A(self, z, P=None):
        return float(self._action(_t(z), self.P if P is None else _t(P)))

    def hv(self, z, V, P=None):
        """H(z) v for every row v of V [nvec, n]: reverse over reverse"""
        z, P = self._args(z, P)
        g, = torch.autograd.grad(self._action(z, P), z, create_graph=True)
        out = np.zeros((len(V), self.n))
        for k, v in enumerate(np.asarray(V, dtype=np.float64)):
            h, = torch.autograd.grad(g, z, grad_outputs=_t(v), retain_graph=True, allow_unused=True)
            if h is not None:
                out[k] = h.numpy()
        return out

    def gn_hv(self, z, V, P=None):
        """2 J^T (w o (J v)): J v as the derivative of J^T u in u (J^T u is linear in u), then one more reverse pass"""
        z, P = self._args(z, P)
        r, w = self._residuals(z, P)
        u = torch.zeros_like(r, requires_grad=True)
        jtu, = torch.autograd.grad(r, z, grad_outputs=u, create_graph=True)
        out = np.zeros((len(V), self.n))
        for k, v in enumerate(np.asarray(V, dtype=np.float64)):
            jv, = torch.autograd.grad(jtu, u, grad_outputs=_t(v), retain_graph=True)
            h, = torch.autograd.grad(r, z, grad_outputs=2.0 * w * jv, retain_graph=True)
            out[k] = h.numpy()
        return out

    def dense(self, z, P=None):
        return self.hv(z, np.eye(self.n), P)

    def products(self, X, V, P=None):
        """(full, Gauss-Newton) products [npts, nvec, n] at the points X [npts, n]; P: None, (NP,) or (npts, NP)"""
        npts = len(X)
        Pp = [None] * npts if P is None else np.broadcast_to(np.asarray(P, float), (npts, self.P.shape[0]))
        return (np.array([self.hv(X[p], V[p], Pp[p]) for p in range(npts)]),
                np.array([self.gn_hv(X[p], V[p], Pp[p]) for p in range(npts)]))


def from_case(c, f=l96):
    """the action of a case as tests/_hess_ref.py writes them (RF0 and rf_scale apart)"""
    RF = c["RF0"] * c["rf_scale"]
    P = np.asarray(c["P"], float)
    return TorchAction(f, c["D"], c["N"], c["Y"], c["Lidx"], c["dt"], c["RM"], RF, P if P.ndim == 1 else P[0], c["Pidx"], c["disc"],
                       t_model=c.get("t_model"), stim=c.get("stim"), nskip=c["nskip"])


# ---------------------------------------------------------------------------------------------------------------
# the cases at the shapes k_hvp really runs, shared by tests/test_hess_torch_ref_cpu.py (host run of the phases) and
# tests/test_gpu_hvp_geometry.py (device).  `plan`: tile_rows asked for -> (T, ntiles) of csrc/va_hvp_geo.h plan_hvp;
# `kernel`: the evaluation kernel family the handle must report (None: not named).
NPTS = 3
UNSORTED = [12, 0, 7]                 # observed columns out of order, an odd count

GEOMETRY_CASES = {}


def _add(name, **kw):
    GEOMETRY_CASES[name] = kw


for _d in ("trapezoid", "SimpsonHermite", "euler", "forwardmap"):
    _N = 41 if _d in ("trapezoid", "SimpsonHermite") else 40
    # one tile of 820 / 800 elements (four strided steps per thread); three tiles, the last partial; four tiles of 260
    # elements, with Simpson-Hermite odd tiles that start on odd rows
    _add("d20-%s" % _d, model="l96", D=20, N=_N, disc=_d, kernel=4, seed=1,
         plan={0: (_N, 1), 16: (16, 3), 13: (13, 4)})
for _d in ("trapezoid", "SimpsonHermite"):
    _add("d20-weights-%s" % _d, model="l96", D=20, N=41, disc=_d, kernel=4, seed=2, nskip=2, Lidx=UNSORTED, rm_array=True,
         rf_array=True, plan={0: (41, 1), 13: (13, 4)})
    # the streaming kernel's handle: padded observation rows (odd L), scalars spread into arrays.  6 images of 15 + 2 / 14 + 3
    # rows of 200 fit the LDS, of 16 + 2 do not.
    _T = 15 if _d == "trapezoid" else 14
    _add("d200-weights-%s" % _d, model="l96", D=200, N=21, disc=_d, kernel=5, seed=3, nskip=2, Lidx=UNSORTED, rm_array=True,
         rf_array=True, plan={0: (_T, 2), 5: (5, 5)})
    _add("d200-rfarray-%s" % _d, model="l96", D=200, N=21, disc=_d, kernel=5, seed=4, Lidx=UNSORTED, rf_array=True,
         plan={0: (_T, 2), 5: (5, 5)})
    # widths: odd and no divisor of 256; wider than a workgroup (Simpson-Hermite: 7 + 6 rows do not fit, 6 + 3 do)
    _add("d67-%s" % _d, model="l96", D=67, N=9, disc=_d, kernel=None, seed=5, plan={0: (9, 1), 4: (4, 3), 3: (3, 3)})
    _add("d300-%s" % _d, model="l96", D=300, N=7, disc=_d, kernel=None, seed=6,
         plan={0: ((7, 1) if _d == "trapezoid" else (6, 2)), 3: (3, 3)})
# the LDS forces T down: 6 images of (3 + 2) rows of 600 fit, of (4 + 2) do not; Simpson-Hermite (2 + 3), not (3 + 6) or (4 + 3)
_add("d600-trapezoid", model="l96", D=600, N=5, disc="trapezoid", kernel=None, seed=7, plan={0: (3, 2)}, forced_T=3)
_add("d600-SimpsonHermite", model="l96", D=600, N=5, disc="SimpsonHermite", kernel=None, seed=7, plan={0: (2, 3)}, forced_T=2)
# generated models: parameter rows, pgrad2 and k_hvp_finish over several tiles with several steps per thread
_add("stencil-d20", model="stencil", D=20, N=21, disc="SimpsonHermite", kernel=None, seed=8, plan={0: (21, 1), 5: (5, 5)})
_add("nakl-n161", model="nakl", D=4, N=161, disc="trapezoid", kernel=None, seed=9, plan={0: (161, 1), 50: (50, 4)})

L96_GEOMETRY = [k for k, v in GEOMETRY_CASES.items() if v["model"] == "l96"]
MODELS = {"l96": l96, "stencil": two_param_stencil, "nakl": nakl}


def _directions(rng, D, N, NPe, plan):
    """per point: two random vectors; for every tiling, the unit vector of the last owned row of tile 0 (column 0) and of
    the first row of tile 1, column D - 1; the unit vector of each estimated parameter"""
    n = N * D + NPe
    at = []
    for T, ntiles in plan.values():
        at.append((min(T, N) - 1) * D)
        if ntiles > 1:
            at.append(T * D + D - 1)
    at = sorted(set(at)) + [N * D + e for e in range(NPe)]
    V = np.zeros((NPTS, 2 + len(at), n))
    V[:, :2] = rng.randn(NPTS, 2, n)
    for k, i in enumerate(at):
        V[:, 2 + k, i] = 1.0
    return V


@functools.lru_cache(maxsize=None)
def geometry_case(name):
    """a case dict as _hess_ref.l96_case makes them (what tests/_hvp_run.host_hv and _capi.Problem take), with `want` and
    `want_gn` from the reference above; P is [NPTS, NP]"""
    g = GEOMETRY_CASES[name]
    D, N, disc, nskip = g["D"], g["N"], g["disc"], g.get("nskip", 1)
    rng = np.random.RandomState(1000 + g["seed"])
    Lidx = list(g.get("Lidx", [0, 2]))
    N_data = (N - 1) // nskip + 1
    c = dict(name=name, D=D, N=N, disc=disc, nskip=nskip, Lidx=Lidx, dt=hr.DT, kernel=g["kernel"], plan=dict(g["plan"]),
             forced_T=g.get("forced_T"), model=g["model"], stim=None)
    if g["model"] == "l96":
        c.update(Pidx=[0], rf_scale=hr.RF_SCALE, Y=3.0 * rng.randn(N_data, len(Lidx)))
        c["RM"] = 4.0 * (0.5 + rng.rand(N_data, len(Lidx))) if g.get("rm_array") else 4.0
        c["RF0"] = 0.5 * (0.5 + rng.rand(N - 1, D)) if g.get("rf_array") else 0.5
        c["P"] = np.full((NPTS, 1), 8.0)
        X = 3.0 * rng.randn(NPTS, N * D + 1)
        X[:, -1] = 8.0 + rng.rand(NPTS)
    else:
        # as tests/test_gpu_hvp.py _generated: parameters in [0.6, 1.4]; here every point has fixed parameters of its own
        NP, c["Pidx"], scale = (2, [0, 1], 1.0) if g["model"] == "stencil" else (18, [0, 6, 7], 0.3)
        c.update(rf_scale=2.0, Y=rng.randn(N_data, len(Lidx)), RM=2.0, RF0=0.7, P=0.6 + 0.8 * rng.rand(NPTS, NP))
        X = scale * rng.randn(NPTS, N * D + len(c["Pidx"]))
        X[:, N * D:] = c["P"][:, c["Pidx"]] + 0.1 * rng.rand(NPTS, len(c["Pidx"]))
        if g["model"] == "nakl":
            c["stim"] = np.sin(0.7 * np.arange(N)) + 0.3
    c["X"] = X
    c["V"] = _directions(rng, D, N, len(c["Pidx"]), c["plan"])
    c["want"], c["want_gn"] = from_case(c, MODELS[g["model"]]).products(X, c["V"], c["P"])
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c
