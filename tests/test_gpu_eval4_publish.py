"""GPU: how k_eval4 publishes a workgroup's partial sums.  Every wave leaves its sums (and, in the column-parameter form, its
[NCV][D] vector partials) in LDS; one wave adds the four in wave order, stores the workgroup's row, runs its gather phase
while the row is acknowledged, counts the workgroup's arrival and later runs the seed's tail.  Line-search launches publish
after the gather phase.  The shapes are the smallest at which that hand-over can go wrong: waves without a row below N,
one tile against two, 16 runs and one run per wave, a seed whose workgroups return early, 200 launches of one evaluation.

Every case runs the problem on k_eval4 (eval_kernel = 4) and on the flat kernel (eval_kernel = 1).  Tolerances: the ones
tests/test_gpu_parity.py holds between two kernel configurations of one problem (test_runs_of_twelve_rows) -- A, me, fe within
1e-13 of |A|, the gradient within 1e-12 of max|g|, a minimisation with the same (nit, nfev, status) and A within 1e-10.
(The two kernels add the same ~N D terms in different orders: N D <= 2,000 terms of either sign, eps = 1.1e-16, leave
that two orders of margin.)"""
import os

import numpy as np
import pytest

from varanneal_amd import _capi, codegen, twin

pytestmark = pytest.mark.gpu

RTOL_A = 1e-13
RTOL_G = 1e-12
RTOL_MIN = 1e-10
OPTS = {'gtol': 1e-8, 'ftol': 1e-8, 'maxfun': 1000000, 'maxiter': 1000000}
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def inputs(D, N, B, seed=0):
    t, Y, _, Lidx = twin.make_twin(D, N)
    rng = np.random.RandomState(1000 * D + N + seed)
    XP = np.concatenate([3.0 * rng.randn(B, N * D), 6.0 + 3.0 * rng.rand(B, 1)], axis=1)
    return Y, Lidx, XP, XP[:, -1:].copy()


def both_kernels(B, D, N, Y, Lidx, P, disc, tile_rows, **kw):
    """the handles of one problem on the flat kernel and on k_eval4"""
    flat = _capi.Problem(B, D, N, Y, Lidx, twin.DT, 4.0, 4e-6, P, [0], disc=disc, eval_kernel=1, **kw)
    col = _capi.Problem(B, D, N, Y, Lidx, twin.DT, 4.0, 4e-6, P, [0], disc=disc, eval_kernel=4, tile_rows=tile_rows, **kw)
    assert flat.info()["eval_kernel"] == 1 and col.info()["eval_kernel"] == 4
    return flat, col


def assert_same_evaluation(e1, e4):
    (A1, me1, fe1, g1), (A4, me4, fe4, g4) = e1, e4
    print("   max rel diff A %.1e me %.1e fe %.1e grad %.1e" % (
        np.max(np.abs(A4 - A1) / np.abs(A1)), np.max(np.abs(me4 - me1) / np.abs(A1)), np.max(np.abs(fe4 - fe1) / np.abs(A1)),
        np.abs(g4 - g1).max() / np.abs(g1).max()))
    assert np.all(np.abs(A4 - A1) <= RTOL_A * np.abs(A1))
    assert np.all(np.abs(me4 - me1) <= RTOL_A * np.abs(A1)) and np.all(np.abs(fe4 - fe1) <= RTOL_A * np.abs(A1))
    assert np.abs(g4 - g1).max() <= RTOL_G * np.abs(g1).max()


# D = 20 with runs of 7 rows (tile_rows = 84: the C3 instantiation): a wave owns 21 rows, a workgroup 84
@pytest.mark.parametrize("D,N,disc,tile_rows,run_rows,ntiles", [
    (20, 22, "trapezoid", 84, 7, 1),          # one tile; waves 2 and 3 own no row below N and must still arrive
    (20, 84, "trapezoid", 84, 7, 1),          # exactly one tile
    (20, 85, "trapezoid", 84, 7, 2),          # one row more: two tiles, the second nearly empty
    (4, 40, "trapezoid", 0, 4, 1),            # 16 runs per wave
    (64, 30, "trapezoid", 0, 4, 2),           # one run per wave
    (20, 23, "SimpsonHermite", 0, 4, 1),      # the three-row stencil
])
def test_evaluation_matches_the_flat_kernel(D, N, disc, tile_rows, run_rows, ntiles):
    B = 2
    Y, Lidx, XP, P = inputs(D, N, B)
    flat, col = both_kernels(B, D, N, Y, Lidx, P, disc, tile_rows)
    with flat, col:
        info = col.info()
        assert (info["run_rows"], info["ntiles"]) == (run_rows, ntiles), info
        e1 = flat.action_grad(XP, 37.0)
        e4 = col.action_grad(XP, 37.0)
        again = col.action_grad(XP, 37.0)
    assert_same_evaluation(e1, e4)
    for a, b in zip(e4, again):
        assert np.array_equal(a, b)


def test_seeds_in_different_phases():
    """B = 3 in one minimisation: seed 0 starts at its own minimiser (max|g| two orders below gtol), is finished by the
    tail of the first launch, and its workgroups take the early return of every later launch while the others go on"""
    D, N, B = 20, 85, 3
    Y, Lidx, XP, P = inputs(D, N, B)
    rf = 1.5 ** 6
    o = dict(OPTS, gtol=1e-4, maxiter=15)
    flat, col = both_kernels(B, D, N, Y, Lidx, P, "trapezoid", 84)
    with flat, col:
        col.tune(persist=0); flat.tune(persist=0)
        x0 = flat.minimize_lbfgs(XP, rf, dict(OPTS, gtol=1e-9, ftol=1e-15, maxiter=5000))
        XP[0] = x0["x"][0]
        g0 = flat.action_grad(XP, rf)[3][0]
        assert np.abs(g0).max() <= 1e-6, np.abs(g0).max()
        r1 = flat.minimize_lbfgs(XP, rf, o)
        r4 = col.minimize_lbfgs(XP, rf, o)
    print("   nit %s nfev %s status %s" % (r4["nit"], r4["nfev"], r4["status"]))
    assert r4["nit"][0] == 0 and r4["nit"][1] > 0 and r4["nit"][2] > 0          # seed 0 was finished before the others
    for k in ("nit", "nfev", "status"):
        assert list(r1[k]) == list(r4[k]), k
    assert np.all(np.abs(r4["A"] - r1["A"]) <= RTOL_MIN * np.abs(r1["A"]))


def test_column_parameter_vectors():
    """the reference's Lorenz-96 with a forcing per site (tests/golden/colparams.npz, case 0: D = 20 on the shipped
    recording), its first 85 rows: every wave also leaves [NCV][D] vector partials for the publishing wave"""
    z = np.load(os.path.join(GOLD, "colparams.npz"))
    D, _, data, di, seed = (int(v) for v in z["cases"][0])
    assert (D, data, di) == (20, 0, 0)
    N, B, disc = 85, 2, "trapezoid"
    rf = float(z["rf_scale"][0])

    def l96(t, x, k):
        return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - x + k
    rng = np.random.RandomState(seed)
    rec = np.load(os.path.join(GOLD, "l96_D20_dt0p025_N161_sm0p5_sec1_mem1.npy"))
    Lidx = [0, 2, 4, 6, 8, 10, 14, 16]
    t, Y = rec[:N, 0], rec[:N, 1:][:, Lidx]
    P = np.tile(8.0 + rng.rand(D), (B, 1))
    Pidx = [i for i in range(D) if i % 7 != 3]
    XP = np.concatenate([20.0 * rng.rand(B, N * D) - 10.0, P[:, Pidx] + 0.1 * rng.randn(B, len(Pidx))], axis=1)
    m4 = codegen.module_for(l96, D, D, colparams=True,
                            col_variant=lambda ne, gh, reach=None: _capi.eval_plan(B, D, N, disc, ne, gh, eval_kernel=4, reach=reach, Lidx=Lidx))
    assert m4["colp"] is not None and m4["col_variant"] is not None
    m1 = codegen.module_for(l96, D, D)
    res = {}
    for ek, m in ((1, m1), (4, m4)):
        with _capi.Problem(B, D, N, Y, Lidx, t[1] - t[0], 4.0, 4e-6, P, Pidx, disc=disc, eval_kernel=ek,
                           rhs=_capi.load_rhs_module(m["so"])) as pb:
            assert pb.info()["eval_kernel"] == ek
            res[ek] = pb.action_grad(XP, rf)
    assert_same_evaluation(res[1], res[4])
    ND = N * D
    assert np.abs(res[4][3][:, ND:] - res[1][3][:, ND:]).max() <= RTOL_G * np.abs(res[1][3][:, ND:]).max()      # the vectors' block on its own scale


def test_three_rung_anneal_with_line_search_launches():
    """line-search launches publish after the gather phase: a three-rung ladder on the three-launch cycle"""
    D, N, B = 20, 85, 2
    Y, Lidx, _, _ = inputs(D, N, B)
    XP = np.empty((B, N * D + 1)); P = np.empty((B, 1))
    for b in range(B):
        X0, P0 = twin.initial_guess(N, D, b, Y, Lidx)
        XP[b, :-1] = X0.ravel(); XP[b, -1] = P0[0]; P[b] = P0
    rf = 1.5 ** np.arange(3)
    flat, col = both_kernels(B, D, N, Y, Lidx, P, "trapezoid", 84, max_beta=3)
    with flat, col:
        flat.tune(persist=0); col.tune(persist=0)
        r1 = flat.anneal(XP, rf, OPTS)
        r4 = col.anneal(XP, rf, OPTS)
    print("   nit %s nfev %s" % (r4["nit"].tolist(), r4["nfev"].tolist()))
    for k in ("nit", "nfev", "status"):
        assert np.array_equal(r1[k], r4[k]), k
    assert np.all(np.abs(r4["A"] - r1["A"]) <= RTOL_MIN * np.abs(r1["A"]))


def test_two_hundred_launches_leave_the_same_bits():
    """a race in the hand-over (a strip read before it was written, a row counted before it was acknowledged, a counter not
    back at zero) would change a bit"""
    D, N, B = 20, 85, 8
    Y, Lidx, XP, P = inputs(D, N, B)
    flat, col = both_kernels(B, D, N, Y, Lidx, P, "trapezoid", 84)
    with flat, col:
        e1 = flat.action_grad(XP, 37.0)
        e4 = col.action_grad(XP, 37.0)
        outs = []
        for iters in (1, 99, 100):          # after launches 1, 100 and 200
            col.eval_timed(37.0, iters)
            outs.append(col.read_eval_outputs())
    assert_same_evaluation(e1, e4)
    for o in outs:
        for a, b in zip(e4, o):
            assert np.array_equal(a, b)
