"""usage: python tools/gen_golden_colparams.py  -- writes tests/golden/colparams.npz.

The reference's own action for its Lorenz-96 `l96(t, x, k)` (examples/Lorenz96_D20/Lorenz96_anneal.py:15-16) called with
a forcing PER SITE, k of length D (upstream has no cap on NP, varanneal/va_ode.py:564-578), through the reference's
`A` / `me_gaussian` / `fe_gaussian` loaded read-only by oracle/_refload.py:

  D = 20,  N = 161 on the shipped recording (tests/golden/l96_D20_...npy, Lidx of the example), trapezoid, SimpsonHermite
  D = 200, N = 401 on synthetic data (every other column observed), trapezoid, euler, SimpsonHermite

For each case: A, me, fe and complex-step directional derivatives Im A(x + i h u) / h along 3 random directions u.  Only
the seeds of np.random.RandomState and the numbers are stored; tests/test_gpu_colparams.py rebuilds the inputs
(colparams_inputs there repeats the recipe below).  Test infrastructure: runs where the reference is at hand."""
import contextlib
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]

import _refload  # noqa: E402

SHIPPED = os.path.join(ROOT, "tests", "golden", "l96_D20_dt0p025_N161_sm0p5_sec1_mem1.npy")
EX_LIDX = [0, 2, 4, 6, 8, 10, 14, 16]        # Lorenz96_anneal.py:22
DISCS = ["trapezoid", "SimpsonHermite", "euler"]
# (D, N, data: 0 shipped recording / 1 synthetic, disc, seed, rf_scale)
CASES = [(20, 161, 0, "trapezoid", 101, 1.5 ** 12), (20, 161, 0, "SimpsonHermite", 102, 1.5 ** 12),
         (200, 401, 1, "trapezoid", 201, 1.5 ** 10), (200, 401, 1, "euler", 202, 1.5 ** 10),
         (200, 401, 1, "SimpsonHermite", 203, 1.5 ** 10)]
NDIR, H = 3, 1e-30


def l96(t, x, k):
    return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - x + k


def inputs(D, N, data, seed):
    """(t, Y, Lidx, X0, P0, Pidx, directions) of a case, from its seed alone (the test repeats this)"""
    rng = np.random.RandomState(seed)
    if data == 0:
        rec = np.load(SHIPPED)
        t, Y, Lidx = rec[:N, 0], rec[:N, 1:][:, EX_LIDX], EX_LIDX
    else:
        Lidx = list(range(0, D, 2))
        t = 0.025 * np.arange(N)
        Y = 3.0 * rng.randn(N, len(Lidx))
    X0 = 20.0 * rng.rand(N, D) - 10.0
    P0 = 8.0 + rng.rand(D)
    Pidx = [i for i in range(D) if i % 7 != 3]              # (a few sites keep a fixed forcing)
    U = rng.randn(NDIR, N * D + len(Pidx))
    return t, Y, Lidx, X0, P0, Pidx, U


def main():
    va = _refload.load_reference("va_ode")
    out = {"cases": np.array([[D, N, data, DISCS.index(disc), seed] for D, N, data, disc, seed, _ in CASES], dtype=np.int64),
           "rf_scale": np.array([c[5] for c in CASES])}
    A_, me_, fe_, dA_ = [], [], [], []
    for D, N, data, disc, seed, rf_scale in CASES:
        t, Y, Lidx, X0, P0, Pidx, U = inputs(D, N, data, seed)
        a = va.Annealer()
        a.set_model(l96, D)
        a.set_data(Y, t=t)
        with contextlib.redirect_stdout(io.StringIO()):
            a.anneal_init(X0, P0.copy(), 1.5, np.arange(2), 4.0, 4e-6, Lidx, Pidx, init_to_data=False, disc=disc)
        a.RF = a.RF0 * rf_scale
        XP = np.append(X0.ravel(), P0[Pidx])
        A = float(a.A(XP)); me = float(a.me_gaussian(XP[:N * D])); fe = float(a.fe_gaussian(XP))
        dA = [float(np.imag(a.A(XP + 1j * H * u)) / H) for u in U]
        A_.append(A); me_.append(me); fe_.append(fe); dA_.append(dA)
        print("D=%3d N=%3d %-15s A=%.16e dA=%s" % (D, N, disc, A, dA))
    out.update(A=np.array(A_), me=np.array(me_), fe=np.array(fe_), dA=np.array(dA_))
    np.savez(os.path.join(ROOT, "tests", "golden", "colparams.npz"), **out)


if __name__ == "__main__":
    main()
