"""GPU: the column-parameter form (shared scalars + per-site parameter vectors, codegen.colparam_form) at the shapes its
chooser accepts -- k_eval4 at every wave geometry (runs of 16, 8, 4, 2, 1 per wave, 0 to 16 idle lanes), k_eval5 past
one strip group (NSG = 2, 3, 5: colp_tail's walk over the tiles of the column's group), the form's limits (24 scalars,
4 vectors), Pidx in any order, line-search launches against the oracle's minimiser, and k_seed at its 24 parameters.

References: va_oracle.numpy_action_generic on the original Python model (A, me, fe), complex-step derivatives of it
(the parameter block in full, three random directions over all unknowns), the flat kernel where NP <= 128, and
va_oracle.lbfgs_generic driven by the device's own evaluation of the same handle (the arbiter of the minimisers)."""
import os

import numpy as np
import pytest

import va_oracle
from _util import GOLD, colparam_model
from varanneal_amd import _capi, codegen, va_ode

pytestmark = pytest.mark.gpu

OPTS = {'gtol': 1e-8, 'ftol': 1e-12, 'maxfun': 1000, 'maxiter': 20}


class Case(object):
    """one problem in column-parameter form: model, shape, weights, data, per-seed parameters and starting points"""

    def __init__(self, D, N, S, V, disc, B=1, interleaved=False, driven=False, rm_array=False, rf_array=False, nskip=1,
                 tile_rows=0, ek=0, Lidx=None, seed=0):
        rng = np.random.RandomState(seed)
        self.f = colparam_model(S, V, interleaved, driven)
        self.D, self.N, self.NP, self.B, self.disc, self.nskip, self.tile_rows = D, N, S + V * D, B, disc, nskip, tile_rows
        self.Lidx = list(range(0, D, 2)) if Lidx is None else list(Lidx)
        self.N_data = (N - 1) // nskip + 1
        self.Y = rng.randn(self.N_data, len(self.Lidx))
        self.RM = 2.0 + 2.0 * rng.rand(self.N_data, len(self.Lidx)) if rm_array else 4.0
        self.RF0 = 0.01 * (0.5 + rng.rand(N - 1, D)) if rf_array else 0.01
        self.t = 0.025 * np.arange(N) + 0.3 if driven else None
        # shared scalars near 1, vector entries near what their terms want (a forcing near 8, gains near 1)
        base = np.concatenate([0.5 + rng.rand(B, S)] + [(8.0 if v == 0 else 1.0) * (0.8 + 0.4 * rng.rand(B, D))
                                                         for v in range(V)], axis=1)
        if interleaved:
            base[:, S:] = base[:, S:].reshape(B, V, D).transpose(0, 2, 1).reshape(B, V * D)
        self.P = base
        self.rng = rng
        plan = dict(rm_array=rm_array, rf_array=rf_array, merr_nskip=nskip, eval_kernel=ek, tile_rows=tile_rows)
        self.m = codegen.module_for(self.f, D, self.NP, colparams=True,
                                    col_variant=lambda ne, gh, reach=None: _capi.eval_plan(
                                        B, D, N, disc, ne, gh, reach=reach, Lidx=self.Lidx, **plan))
        assert self.m["colp"] is not None and self.m["col_variant"] is not None
        self.rid = _capi.load_rhs_module(self.m["so"])
        self.ek = ek

    def xp(self, Pidx):
        return np.stack([np.append(3.0 * self.rng.randn(self.N * self.D), self.P[b][Pidx] + 0.1 * self.rng.randn(len(Pidx)))
                         for b in range(self.B)])

    def problem(self, Pidx, B=None, P=None, **kw):
        B = self.B if B is None else B
        kw = dict(dict(disc=self.disc, rhs=self.rid, merr_nskip=self.nskip, eval_kernel=self.ek, tile_rows=self.tile_rows,
                       t_model=self.t), **kw)
        return _capi.Problem(B, self.D, self.N, self.Y, self.Lidx, 0.025, self.RM, self.RF0,
                             self.P[:B] if P is None else P, Pidx, **kw)

    def action(self, Pidx, b, rf):
        return lambda z: va_oracle.numpy_action_generic(self.f, z, self.D, self.N, self.Y, self.Lidx, 0.025, self.RM,
                                                        self.RF0 * rf, self.NP, Pidx, self.P[b], self.disc,
                                                        t_model=self.t, nskip=self.nskip)


def check_reference(c, Pidx, A, me, fe, g, rf, ndir=3):
    """every seed's (A, me, fe) to 1e-12 of the oracle's, the parameter block of grad A to 1e-10 of its max by complex
    step, grad A . u to 1e-10 for random directions u over all unknowns"""
    ND = c.N * c.D
    XPs = c._xp
    for b in range(c.B):
        fun = c.action(Pidx, b, rf)
        A0, me0, fe0 = fun(XPs[b])
        assert abs(A[b] - A0) <= 1e-12 * abs(A0), (b, A[b], A0)
        assert abs(me[b] - me0) <= 1e-12 * abs(A0) and abs(fe[b] - fe0) <= 1e-12 * abs(A0), b
        z = np.asarray(XPs[b], dtype=np.complex128).copy()
        gp = np.empty(len(Pidx))
        for k in range(len(Pidx)):
            z[ND + k] = complex(XPs[b][ND + k], 1e-30)
            gp[k] = fun(z)[0].imag / 1e-30
            z[ND + k] = XPs[b][ND + k]
        assert np.abs(g[b, ND:] - gp).max() <= 1e-10 * np.abs(gp).max(), (b, np.argmax(np.abs(g[b, ND:] - gp)))
        for _ in range(ndir):
            u = c.rng.randn(len(z))
            du = fun(XPs[b] + 1e-30j * u)[0].imag / 1e-30
            assert abs(np.dot(g[b], u) - du) <= 1e-10 * np.dot(np.abs(g[b]), np.abs(u)), (b, np.dot(g[b], u), du)


def run_case(c, Pidx, want, rf=20.0, flat=False):
    c._xp = c.xp(Pidx)
    with c.problem(Pidx) as pr:
        assert pr.info()["eval_kernel"] == want
        A, me, fe, g = pr.action_grad(c._xp, rf)
    check_reference(c, Pidx, A, me, fe, g, rf)
    if flat:                                      # NP <= 128: the flat kernel of the same model
        rid = _capi.load_rhs_module(codegen.module_for(c.f, c.D, c.NP)["so"])
        with c.problem(Pidx, rhs=rid, eval_kernel=1) as pr:
            assert pr.info()["eval_kernel"] == 1
            A1, me1, fe1, g1 = pr.action_grad(c._xp, rf)
        assert np.all(np.abs(A - A1) <= 1e-12 * np.abs(A1))
        assert np.abs(g - g1).max() <= 1e-12 * np.abs(g1).max()
    return A, g


def estimated(c, S, frac, seed):
    """Pidx: the shared scalars but the first (when there are several), the vector entries but a random fraction"""
    rng = np.random.RandomState(seed)
    fixed = set((S + rng.choice(c.NP - S, int(round(frac * (c.NP - S))), replace=False)).tolist()) | ({0} if S > 1 else set())
    return [k for k in range(c.NP) if k not in fixed]


# ---- k_eval4: one module per wave geometry (RW = 64 // D runs per wave, 64 - RW * D idle lanes)
EVAL4 = {
    # D: Case arguments                                            RW  idle
    4: dict(N=97, S=2, V=2, disc="trapezoid", B=3, interleaved=True),                              # 16   0
    8: dict(N=81, S=3, V=1, disc="euler", rf_array=True, nskip=2),                                 #  8   0
    14: dict(N=69, S=0, V=4, disc="SimpsonHermite", B=3, rm_array=True, nskip=2),                  #  4   8
    24: dict(N=61, S=1, V=2, disc="forwardmap", driven=True, nskip=3),                             #  2  16
    64: dict(N=45, S=24, V=4, disc="trapezoid", interleaved=True, rf_array=True),                  #  1   0
}


def eval4_case(D):
    return Case(D, ek=4, seed=D, **EVAL4[D])


@pytest.mark.parametrize("D", sorted(EVAL4))
def test_k_eval4_wave_geometries(D):
    c = eval4_case(D)
    run_case(c, estimated(c, EVAL4[D]["S"], 0.2, 100 + D), 4, flat=c.NP <= 128 and D in (4, 24))


# ---- k_eval5 past one strip group
def strip_starts(D):
    """k_eval5's strips (va_tile5.h tile5_cols): the fewest NS whose widest strip holds at most 56 columns"""
    ns = (D + 55) // 56
    while True:
        c0 = [8 * ((s * (D // 8)) // ns) for s in range(ns)] + [D]
        if max(np.diff(c0)) <= 56:
            return c0
        ns += 1


def lidx_skipping(D, every=3, skip=(1, 3)):
    """every `every`-th column of the strips not in `skip` (strips without an observed column)"""
    c0 = strip_starts(D)
    return [c for s in range(len(c0) - 1) if s not in skip for c in range(c0[s], c0[s + 1], every)]


EVAL5 = {
    # D: NS strips, WPG = 4, NSG groups
    226: dict(N=97, S=3, V=2, disc="trapezoid", tile_rows=33),                                     # 5 strips, NSG 2
    450: dict(N=65, S=0, V=4, disc="SimpsonHermite", interleaved=True, rf_array=True),             # 10 strips, NSG 3
    1000: dict(N=33, S=3, V=1, disc="euler", rm_array=True),                                       # 18 strips, NSG 5
}


def eval5_case(D, B=1):
    return Case(D, B=B, Lidx=lidx_skipping(D), seed=D, **EVAL5[D])


@pytest.mark.parametrize("D,tile_rows,nseg", [(226, 97, 1), (226, 49, 2), (226, 33, 3), (450, 0, 2), (1000, 0, 1)])
def test_k_eval5_strip_groups(D, tile_rows, nseg):
    c = eval5_case(D)
    c.tile_rows = tile_rows
    Pidx = estimated(c, EVAL5[D]["S"], 0.1, 200 + D)
    c._xp = c.xp(Pidx)
    with c.problem(Pidx) as pr:
        info = pr.info()
        assert info["eval_kernel"] == 5 and info["ntiles"] == nseg * {226: 2, 450: 3, 1000: 5}[D]
        A, me, fe, g = pr.action_grad(c._xp, 20.0)
    check_reference(c, Pidx, A, me, fe, g, 20.0)


def test_k_eval5_seeds_and_fold():
    """D = 226 (NSG = 2): B = 3 equals three B = 1 runs bit for bit; the tail in its own kernel (fold = 0) agrees with
    the folded one to 1e-12"""
    c = eval5_case(226, B=3)
    Pidx = list(range(c.NP))
    c._xp = c.xp(Pidx)
    with c.problem(Pidx) as pr:
        assert pr.info()["eval_kernel"] == 5
        A, me, fe, g = pr.action_grad(c._xp, 30.0)
        pr.tune(fold=0)
        A0, _, _, g0 = pr.action_grad(c._xp, 30.0)
    assert np.all(np.abs(A0 - A) <= 1e-12 * np.abs(A))
    assert np.abs(g0 - g).max() <= 1e-12 * np.abs(g).max()
    for b in range(3):
        with c.problem(Pidx, B=1, P=c.P[b:b + 1]) as pr:
            A1, _, _, g1 = pr.action_grad(c._xp[b:b + 1], 30.0)
        assert A1[0] == A[b] and np.array_equal(g1[0], g[b]), b
    check_reference(c, Pidx, A, me, fe, g, 30.0, ndir=1)


# ---- Pidx in any order
@pytest.mark.parametrize("D,want", [(8, 4), (226, 5)])
def test_pidx_order(D, want):
    """Pidx interleaving shared scalars and vector entries in a random order: the gradient is the sorted-Pidx one
    permuted, bit for bit"""
    c = eval4_case(D) if want == 4 else eval5_case(D)
    rng = np.random.RandomState(300 + D)
    Ps = estimated(c, 0, 0.25, 300 + D)
    perm = rng.permutation(len(Ps))
    Pp = [Ps[k] for k in perm]
    assert Pp != Ps
    XPs = c.xp(Ps)
    ND = c.N * c.D
    XPp = np.concatenate([XPs[:, :ND], XPs[:, ND:][:, perm]], axis=1)
    out = []
    for Pidx, XP in ((Ps, XPs), (Pp, XPp)):
        with c.problem(Pidx) as pr:
            assert pr.info()["eval_kernel"] == want
            out.append(pr.action_grad(XP, 20.0))
    (As, _, _, gs), (Ap, _, _, gp) = out
    assert np.array_equal(As, Ap)
    assert np.array_equal(gp[:, :ND], gs[:, :ND]) and np.array_equal(gp[:, ND:], gs[:, ND:][:, perm])


# ---- line-search launches: the device's L-BFGS against the oracle's on the device's own evaluation
def same_path(pr, XP, rf, opts=OPTS):
    r = pr.minimize_lbfgs(XP, rf, opts)
    fg = lambda x: (lambda o: (o[0][0], o[3][0]))(pr.action_grad(x[None, :], rf))
    _, A, st, nit, nfev = va_oracle.lbfgs_generic(fg, XP[0], opts)
    assert (int(r["nit"][0]), int(r["nfev"][0]), int(r["status"][0])) == (nit, nfev, st)
    assert abs(r["A"][0] - A) <= 1e-10 * abs(A)
    return r


@pytest.mark.parametrize("D,want", [(64, 4), (226, 5)])
def test_line_search_against_the_oracle_minimiser(D, want):
    c = eval4_case(D) if want == 4 else eval5_case(D)
    Pidx = list(range(c.NP))
    XP = c.xp(Pidx)
    with c.problem(Pidx) as pr:
        assert pr.info()["eval_kernel"] == want and pr.persistent() is None
        r = same_path(pr, XP, 20.0)
    assert r["nit"][0] >= 10


# ---- k_seed at its 24 parameters (the reference's shipped example's shape: D = 20, N = 161, Simpson-Hermite, one seed)
@pytest.mark.parametrize("S", [4, 5])
def test_k_seed_at_its_parameter_limit(S):
    D, N = 20, 161
    rec = np.load(os.path.join(GOLD, "l96_D20_dt0p025_N161_sm0p5_sec1_mem1.npy"))
    Lidx = [0, 2, 4, 6, 8, 10, 14, 16]
    Y = rec[:N, 1:][:, Lidx]
    f = colparam_model(S, 1)
    NP = S + D
    m = codegen.module_for(f, D, NP, colparams=True,
                           col_variant=lambda ne, gh, reach=None: _capi.eval_plan(1, D, N, "SimpsonHermite", ne, gh,
                                                                                reach=reach, Lidx=Lidx))
    assert m["colp"] is not None
    rid = _capi.load_rhs_module(m["so"])
    rng = np.random.RandomState(400 + S)
    P = np.append(0.5 + rng.rand(S), 8.0 + rng.rand(D))[None, :]
    X0 = 20.0 * rng.rand(N, D) - 10.0
    X0[:, Lidx] = Y
    Pidx = list(range(NP))
    XP = np.append(X0.ravel(), P[0] + 0.1 * rng.randn(NP))[None, :]
    o = dict(OPTS, maxiter=25)
    # (RF at 2^15 of its start: lower, the unobserved columns are nearly free, and two minimisers that differ only in
    # rounding -- 3e-14 apart after the first iteration -- drift apart a hundredfold per iteration)
    rf = 2.0 ** 15
    with _capi.Problem(1, D, N, Y, Lidx, 0.025, 4.0, 4e-6, P, Pidx, disc="SimpsonHermite", rhs=rid) as pb:
        assert (pb.persistent() is not None) == (NP <= 24)
        r = same_path(pb, XP, rf, o)
        pb.tune(persist=0)
        assert pb.persistent() is None and pb.info()["eval_kernel"] == 4
        r3 = same_path(pb, XP, rf, o)
    assert (r["nit"][0], r["nfev"][0], r["status"][0]) == (r3["nit"][0], r3["nfev"][0], r3["status"][0])
    assert abs(r["A"][0] - r3["A"][0]) <= 1e-10 * abs(r3["A"][0]) and r["nit"][0] >= 10


def test_annealer_forcing_per_site_on_k_seed():
    """the reference's own l96 with P0 = np.full(20, 8.0) on the shipped example's shape: the Annealer's route is the
    column-parameter module's k_seed; every rung's A is a fresh evaluation's at the minimiser it returns"""
    D, N = 20, 161

    def l96(t, x, k):
        return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - x + k
    rec = np.load(os.path.join(GOLD, "l96_D20_dt0p025_N161_sm0p5_sec1_mem1.npy"))
    Lidx = [0, 2, 4, 6, 8, 10, 14, 16]
    rng = np.random.RandomState(500)
    X0 = 20.0 * rng.rand(N, D) - 10.0
    a = va_ode.Annealer()
    a.set_model(l96, D)
    a.set_data(rec[:N, 1:][:, Lidx], t=rec[:N, 0])
    beta = np.arange(4)
    a.anneal(X0, np.full(D, 8.0), 2.0, beta, 4.0, 1e-2, Lidx, list(range(D)), disc="SimpsonHermite",
             opt_args={'gtol': 1e-8, 'ftol': 1e-8, 'maxfun': 100000, 'maxiter': 200}, verbose=False)
    assert a._pb.persistent() is not None
    for k in range(len(beta)):
        A = a._pb.action_grad(a.minpaths[k][None, :], 2.0 ** beta[k], want_grad=False)[0][0]
        assert abs(A - a.A_array[k]) <= 1e-10 * abs(A), (k, A, a.A_array[k])
    assert np.any(a.minpaths[-1][N * D:] != 8.0)
