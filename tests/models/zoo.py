"""A small zoo of user models for the generated tangent and second-order code (TEST INFRASTRUCTURE).  Every model is ONE
function text `body(ns, t, x, p, st)` on whole time slices -- t (rows,), x (rows, D), p indexable by parameter, st (rows,) or
None -- written against an array namespace `ns`, and bound to three namespaces:

    NumpyUser     NumPy as a user writes it (np.maximum / np.abs / np.clip / np.where on comparisons): the callable that
                  goes to codegen.module_for                                                         Model.numpy
    ComplexSafe   NumPy whose kinked primitives choose the branch by the REAL part and carry the value through, so that
                  the complex step differentiates the taken branch; float64 or np.longdouble, by its inputs
                                                                              Model.row, Model.jvp, Model.switch_row
    Torch         torch float64, for autograd (tests/_hess_torch_ref.TorchAction, torch.autograd.functional.jvp)
                                                                                                     Model.torch

The kinked primitives are ns.relu(a), ns.absval(a), ns.clip(a, lo, hi) and ns.select(a > c, u, v).  A kinked model also
states its switching arguments once, `switches(ns, t, x, p, st)` -> (rows, n_switch) of (argument - threshold): the tests
keep their inputs away from the thresholds with it and record which branches a run takes.
tests/test_zoo_cpu.py holds the three bindings of every model to each other before anything is compared with a kernel."""
import numpy as np

EPS = 1e-30


# ---------------------------------------------------------------------------------------------------------------
class NumpyUser(object):
    tanh, exp, sqrt, sin = np.tanh, np.exp, np.sqrt, np.sin
    roll = staticmethod(lambda x, k: np.roll(x, k, -1))
    stack = staticmethod(lambda cols: np.stack(cols, axis=-1))
    relu = staticmethod(lambda a: np.maximum(a, 0.0))
    absval = staticmethod(lambda a: np.abs(a))
    clip = staticmethod(lambda a, lo, hi: np.clip(a, lo, hi))
    select = staticmethod(lambda c, u, v: np.where(c, u, v))


class ComplexSafe(object):
    """comparisons of complex arrays order by the real part first (NumPy's lexicographic order), which is what
    ns.select(a > c, ...) needs as long as the real parts differ -- the tests' margins see to that"""
    tanh, exp, sqrt, sin = np.tanh, np.exp, np.sqrt, np.sin
    roll = staticmethod(lambda x, k: np.roll(x, k, -1))
    stack = staticmethod(lambda cols: np.stack(cols, axis=-1))
    relu = staticmethod(lambda a: np.where(np.real(a) >= 0.0, a, 0.0 * a))
    absval = staticmethod(lambda a: np.where(np.real(a) >= 0.0, a, -a))
    select = staticmethod(lambda c, u, v: np.where(c, u, v))

    @staticmethod
    def clip(a, lo, hi):
        r = np.where(np.real(a) >= lo, a, lo + 0.0 * a)
        return np.where(np.real(r) <= hi, r, hi + 0.0 * a)


def _torch():
    import torch
    return torch


class Torch(object):
    tanh = staticmethod(lambda a: _torch().tanh(a))
    exp = staticmethod(lambda a: _torch().exp(a))
    sqrt = staticmethod(lambda a: _torch().sqrt(a))
    sin = staticmethod(lambda a: _torch().sin(a))
    roll = staticmethod(lambda x, k: _torch().roll(x, k, -1))
    stack = staticmethod(lambda cols: _torch().stack(cols, dim=-1))
    relu = staticmethod(lambda a: _torch().where(a >= 0.0, a, _torch().zeros_like(a)))
    absval = staticmethod(lambda a: _torch().where(a >= 0.0, a, -a))

    @staticmethod
    def clip(a, lo, hi):
        torch = _torch()
        r = torch.where(a >= lo, a, torch.full_like(a, lo))
        return torch.where(r <= hi, r, torch.full_like(a, hi))

    @staticmethod
    def select(c, u, v):
        torch = _torch()
        as_t = lambda w: w if torch.is_tensor(w) else torch.tensor(float(w), dtype=torch.float64)
        return torch.where(c, as_t(u), as_t(v))


# ---------------------------------------------------------------------------------------------------------------
class Model(object):
    def __init__(self, name, D, NP, body, nstim=0, switches=None, timed=False, colparams=False):
        self.name, self.D, self.NP, self.nstim, self.body, self.switches = name, D, NP, nstim, body, switches
        self.timed, self.kinked, self.colparams = timed, switches is not None, colparams
        self.numpy = self._slices(NumpyUser)
        self.numpy.__name__ = "zoo_" + name
        self.torch = self._slices(Torch)

    def _slices(self, ns):
        body, nstim = self.body, self.nstim

        def f(t, x, pin):
            p, st = pin if nstim else (pin, None)
            return body(ns, t, x, p, st)
        return f

    def _one(self, fn, t, x, p, st):
        """a body on one row: t a scalar, x (D,), st the stimulus row (nstim,) or None; the dtype is the inputs'"""
        x = np.asarray(x)
        s = np.reshape(st, (-1,))[:1] if self.nstim else None
        return fn(ComplexSafe, np.reshape(t, (1,)), x[None, :], p, s)[0]

    def row(self, t, x, p, st=None):
        """f as _predict_ref.rk4, _tlm_ref.tlm_rk4 and _lyap_ref.lyap_ref take it, complex-safe"""
        return self._one(self.body, t, x, p, st)

    def switch_row(self, t, x, p, st=None):
        """(n_switch,) of (switching argument - threshold) at one row, real"""
        return np.real(self._one(self.switches, t, x, p, st))

    def switch_slices(self, t, x, p, st=None):
        """the same on whole slices: (rows, n_switch)"""
        return np.real(self.switches(ComplexSafe, np.asarray(t), np.asarray(x), p, st))

    def jvp(self, Pidx):
        """J(x) vx + (df/dp)[:, Pidx] vp as _tlm_ref.tlm_rk4 takes it (vx (nvec, D), vp (nvec, len(Pidx))) by the complex
        step: the state directions as the rows of one slice, one more row per estimated parameter"""
        Pidx = list(Pidx)

        def jvp(t, x, p, st, vx, vp):
            vx = np.asarray(vx)
            dt = vx.dtype
            eps = dt.type(EPS)
            nvec = vx.shape[0]
            tt = np.full(nvec, t, dtype=dt)
            s = np.broadcast_to(np.reshape(st, (-1,))[:1], (nvec,)) if self.nstim else None
            p = np.asarray(p, dtype=dt)
            out = self.body(ComplexSafe, tt, np.asarray(x, dtype=dt)[None, :] + 1j * eps * vx, p, s).imag / eps
            for e, k in enumerate(Pidx):
                pc = p.astype(np.result_type(dt, np.complex64))
                pc[k] += 1j * eps
                out = out + np.asarray(vp)[:, e:e + 1] * (self.row(t, np.asarray(x, dtype=dt), pc, st).imag / eps)[None, :]
            return out
        return jvp

    def torch_jvp(self, t, x, p, st, vx, vp_full):
        """the same product for ONE direction (vx (D,), vp_full (NP,)) from torch.autograd.functional.jvp"""
        torch = _torch()
        tt = lambda a: torch.tensor(np.array(a, dtype=np.float64), dtype=torch.float64)
        tr, sr = tt([t]), (tt(np.reshape(st, (-1,))[:1]) if self.nstim else None)

        def g(xx, pp):
            return self.torch(tr, xx[None, :], (pp, sr) if self.nstim else pp)[0]
        return torch.autograd.functional.jvp(g, (tt(x), tt(p)), (tt(vx), tt(vp_full)))[1].numpy()

    def torch_second_order(self, t, x, v, s, q, p, st):
        """what the emitted jvp, vjp2 and pgrad2 compute at one point, from autograd alone: fdot = J v + (df/dp) q (the
        derivative, in u, of J^T u), then the gradient of s . fdot in x [D] and in p [NP]"""
        torch = _torch()
        tt = lambda a: torch.tensor(np.array(a, dtype=np.float64), dtype=torch.float64)
        tr, sr = tt([t]), (tt(np.reshape(st, (-1,))[:1]) if self.nstim else None)
        xx, pp = tt(x).requires_grad_(True), tt(p).requires_grad_(True)
        y = self.torch(tr, xx[None, :], (pp, sr) if self.nstim else pp)[0]
        u = torch.zeros_like(y, requires_grad=True)
        jtu = torch.autograd.grad(y, (xx, pp), grad_outputs=u, create_graph=True, allow_unused=True)
        pairs = [(a, b) for a, b in zip(jtu, (tt(v), tt(q))) if a is not None]
        fdot, = torch.autograd.grad([a for a, _ in pairs], u, grad_outputs=[b for _, b in pairs], create_graph=True)
        gx, gp = torch.autograd.grad((tt(s) * fdot).sum(), (xx, pp), allow_unused=True)
        z = lambda g, n: np.zeros(n) if g is None else g.numpy()
        return fdot.detach().numpy(), z(gx, self.D), z(gp, self.NP)


# ---------------------------------------------------------------------------------------------------------------
# kinked models: a rectified neighbour times a neighbour, a leak whose rate is selected by x > 0.5, a clipped neighbour
# driven by sin(0.3 t), |x| times the neighbour after next.  Both parameters multiply states.
LEAK_AT, CLIP_LO, CLIP_HI = 0.5, -0.8, 0.9


def _kinked(ns, t, x, p, st):
    xm, xp, xpp = ns.roll(x, 1), ns.roll(x, -1), ns.roll(x, -2)
    leak = ns.select(x > LEAK_AT, 1.5, 0.4)
    return (p[0] * ns.relu(xm) * xp - p[1] * leak * x * x + ns.clip(xp, CLIP_LO, CLIP_HI) * ns.sin(0.3 * t)[:, None]
            + 0.5 * ns.absval(x) * xpp - 0.6 * x + 0.3)


def _kinked_switches(ns, t, x, p, st):
    """relu(x_{i-1}) and |x_i| switch at 0 (the same surfaces, listed once per primitive), the leak at 0.5, the clip at both ends"""
    xm, xp = ns.roll(x, 1), ns.roll(x, -1)
    return ns.stack([xm, x - LEAK_AT, xp - CLIP_LO, xp - CLIP_HI, x]).reshape(x.shape[0], -1)


kinked_small = Model("kinked_small", 6, 2, _kinked, switches=_kinked_switches, timed=True)      # D < 8: the switch form
kinked_stencil = Model("kinked_stencil", 12, 2, _kinked, switches=_kinked_switches, timed=True)  # the one-body form


def timed_mix(seed):
    """the five kinds of tests/test_gpu_fuzz._random_model (same generator, same seed -> same model) in namespace form"""
    rng = np.random.RandomState(15000 + seed)
    D = int(rng.randint(2, 7)); NP = int(rng.randint(1, 6)); stim = bool(rng.rand() < 0.5)
    A = rng.randn(D, D) * 0.3
    c = rng.randn(D) * 0.5
    kinds = rng.randint(0, 5, size=D)
    pk = rng.randint(0, NP, size=(D, 2))

    def body(ns, t, x, p, st):
        cols = []
        for i in range(D):
            lin = sum(float(A[i, j]) * x[:, j] for j in range(D))
            pa, pb = p[int(pk[i, 0])], p[int(pk[i, 1])]
            xi, xn = x[:, i], x[:, (i + 1) % D]
            if kinds[i] == 0:
                term = pa * xi * xn + float(c[i]) * xi * xi * xi
            elif kinds[i] == 1:
                term = pa * ns.tanh(xn / (1.0 + pb * pb)) - xi
            elif kinds[i] == 2:
                term = ns.exp(-0.1 * xi * xi) * pa + pb * xn
            elif kinds[i] == 3:
                term = pa / (1.0 + xn * xn) + ns.sqrt(1.0 + xi * xi) * pb
            else:
                term = pa * ns.sin(0.3 * t) * xn - pb * xi
            cols.append(lin + term + (st * float(c[i]) if stim else 0.0))
        return ns.stack(cols)
    m = Model("timed_mix%d" % seed, D, NP, body, nstim=int(stim), timed=bool((kinds == 4).any()))
    m.kinds = kinds
    return m


def _l96_damped(ns, t, x, p, st):
    """tests/models/nakl.py::l96_damped: forcing p[0] (1 + 0.1 sin t), damping p[1]"""
    return ns.roll(x, 1) * (ns.roll(x, -1) - ns.roll(x, 2)) - p[1] * x + p[0] * (1.0 + 0.1 * ns.sin(t))[:, None]


def l96_damped(D):
    return Model("l96_damped%d" % D, D, 2, _l96_damped, timed=True)


def _l96_colparams(ns, t, x, p, st):
    """Lorenz-96 with a forcing per site: p is the whole vector (NP = D)"""
    return ns.roll(x, 1) * (ns.roll(x, -1) - ns.roll(x, 2)) - x + p


l96_colparams = Model("l96_colparams", 20, 20, _l96_colparams, colparams=True)

MIX_SEEDS = (9, 0)        # 9: D = 5, NP = 4, a stimulus, kinds 1 0 4 1 4;  0: D = 6, NP = 1, kinds 3 4 4 4 2 4 -- all five between them


def all_models():
    """name -> Model, every model of the zoo at the shapes the tests use (made once)"""
    if not _all:
        for m in (kinked_small, kinked_stencil, timed_mix(MIX_SEEDS[0]), timed_mix(MIX_SEEDS[1]), l96_damped(20), l96_damped(67),
                  l96_colparams):
            _all[m.name] = m
    return _all


_all = {}
