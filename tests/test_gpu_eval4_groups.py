"""GPU: k_eval4 with G row groups per workgroup (csrc/va_eval4.h; the `wide` knob of va_problem_tune).  A row group is four
waves and owns one row of the partial tables; a workgroup of G of them publishes G rows after ONE barrier, counts ONE
arrival and is decoded from blockIdx by the seed's workgroups, not its row groups.  None of that may change a bit: every
case runs one handle with wide=0 (4-wave workgroups, the geometry every other test runs) and with the width under test
and compares the raw float64 with np.array_equal -- there is no tolerance.

Shapes (D = 20, L = 7): trapezoid at runs of 7 rows (row group = 84 rows, G = 3 -> 252 rows per workgroup) with N = 30
(less than one wide workgroup: its second and third row group own no row), 253 (one row past a wide workgroup) and 505
(seven row groups: the third workgroup's last two are empty and must neither publish a row nor store a gradient);
Simpson-Hermite at runs of 4 and of 12 rows with G = 2; one and three seeds; a generated column-parameter model for
the rows of the vector table."""
import numpy as np
import pytest

from varanneal_amd import _capi, codegen, twin

pytestmark = pytest.mark.gpu

OPTS = {'gtol': 1e-8, 'ftol': 1e-8, 'maxfun': 100000, 'maxiter': 300}
RF = 1.5 ** np.arange(3)
_inputs = {}


def inputs(N, B, D=20):
    """data and start points of a problem: made once, shared, never written"""
    if (N, B, D) not in _inputs:
        _, Y, _, Lidx = twin.make_twin(D, N)
        XP = np.empty((B, N * D + 1)); P = np.empty((B, 1))
        for b in range(B):
            X0, P0 = twin.initial_guess(N, D, b, Y, Lidx)
            XP[b, :-1] = X0.ravel(); XP[b, -1] = P0[0]; P[b] = P0
        for a in (Y, XP, P):
            a.setflags(write=False)
        _inputs[(N, B, D)] = (Y, Lidx, XP, P)
    return _inputs[(N, B, D)]


def assert_bits(pb, XP, G, nwg, ladder=True):
    """one evaluation and one three-rung ladder at wide=0 and at G row groups per workgroup"""
    B = XP.shape[0]
    pb.tune(persist=0)                           # (the three-launch cycle: the line-search launches of k_eval4)
    info = pb.info()
    out = {}
    for wide in (0, G):
        pb.tune(wide=wide)
        now = pb.info()
        assert now["row_groups"] == max(wide, 1) and now["eval_grid"] == B * (nwg if wide else info["ntiles"]), now
        assert (now["ntiles"], now["tile_rows"], now["run_rows"]) == (info["ntiles"], info["tile_rows"], info["run_rows"])
        out[wide] = (pb.action_grad(XP, 37.0), pb.anneal(XP, RF, OPTS) if ladder else None)
    for a, b in zip(out[0][0], out[G][0]):
        assert a.dtype == np.float64 and np.array_equal(a, b)
    if ladder:
        r0, rG = out[0][1], out[G][1]
        print("   nit %s nfev %s" % (rG["nit"].tolist(), rG["nfev"].tolist()))
        for k in ("nit", "nfev", "status", "A"):
            assert np.array_equal(r0[k], rG[k]), k


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N,ntiles", [(30, 1), (253, 4), (505, 7)])
@pytest.mark.parametrize("G", [2, 3])
def test_trapezoid_runs_of_seven(G, N, ntiles, B):
    Y, Lidx, XP, P = inputs(N, B)
    with _capi.Problem(B, 20, N, Y, Lidx, twin.DT, 4.0, 4e-6, P, [0], disc="trapezoid", eval_kernel=4, tile_rows=84, max_beta=3) as pb:
        info = pb.info()
        assert (info["eval_kernel"], info["run_rows"], info["tile_rows"], info["ntiles"]) == (4, 7, 84, ntiles), info
        assert_bits(pb, XP, G, (ntiles + G - 1) // G)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("N,tile_rows,run_rows,ntiles", [(31, 0, 4, 1), (253, 0, 4, 6), (31, 144, 12, 1), (253, 144, 12, 2)])
def test_simpson_hermite_two_row_groups(N, tile_rows, run_rows, ntiles, B):
    Y, Lidx, XP, P = inputs(N, B)
    with _capi.Problem(B, 20, N, Y, Lidx, twin.DT, 4.0, 4e-6, P, [0], disc="SimpsonHermite", eval_kernel=4, tile_rows=tile_rows, max_beta=3) as pb:
        info = pb.info()
        assert (info["eval_kernel"], info["run_rows"], info["ntiles"]) == (4, run_rows, ntiles), info
        assert_bits(pb, XP, 2, (ntiles + 1) // 2)


@pytest.mark.parametrize("G", [2, 3])
def test_column_parameter_vectors(G):
    """Lorenz-96 with a forcing per site as a generated column-parameter module: every row group also owns a row of the
    vector table (evv), written by the publishing wave from the [NCV][D] partials its four waves left in LDS"""
    D, N, B, disc = 20, 253, 3, "trapezoid"

    def l96(t, x, k):
        return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - x + k
    Y, Lidx, XP0, _ = inputs(N, B)
    rng = np.random.RandomState(7)
    P = np.tile(8.0 + rng.rand(D), (B, 1))
    Pidx = [i for i in range(D) if i % 7 != 3]
    XP = np.concatenate([XP0[:, :N * D], P[:, Pidx] + 0.1 * rng.randn(B, len(Pidx))], axis=1)
    m = codegen.module_for(l96, D, D, colparams=True,
                           col_variant=lambda ne, gh, reach=None: _capi.eval_plan(B, D, N, disc, ne, gh, eval_kernel=4, reach=reach, Lidx=Lidx))
    assert m["colp"] is not None and m["col_variant"] is not None
    with _capi.Problem(B, D, N, Y, Lidx, twin.DT, 4.0, 4e-6, P, Pidx, disc=disc, eval_kernel=4, rhs=_capi.load_rhs_module(m["so"]), max_beta=3) as pb:
        info = pb.info()
        assert info["eval_kernel"] == 4 and info["ntiles"] > G, info
        assert_bits(pb, XP, G, (info["ntiles"] + G - 1) // G)


def test_planner_and_knob():
    """the planner's rule (wide=1; a handle starts on 4-wave workgroups, which measured faster: profiles/r06_groups_c3.txt) at
    the headline shape and at its Simpson-Hermite sibling (nothing is launched), and the widths a run length has no kernel for"""
    Y, Lidx, _, _ = inputs(1001, 1)
    P = np.full((64, 1), 8.0)
    with _capi.Problem(64, 20, 1000, Y[:1000], Lidx, twin.DT, 4.0, 4e-6, P, [0], disc="trapezoid") as pb:
        info = pb.info()
        assert (info["eval_kernel"], info["run_rows"], info["tile_rows"], info["ntiles"]) == (4, 7, 84, 12), info
        assert (info["row_groups"], info["eval_grid"]) == (1, 768), info           # handles start on 4-wave workgroups (measured faster)
        pb.tune(wide=1)                                                             # the planner's rule:
        info = pb.info()
        assert (info["row_groups"], info["eval_grid"]) == (3, 256), info           # three 4-wave workgroups per CU -> one of 12 waves
    with _capi.Problem(64, 20, 1001, Y, Lidx, twin.DT, 4.0, 4e-6, P, [0], disc="SimpsonHermite") as pb:
        pb.tune(wide=1)
        info = pb.info()
        assert (info["run_rows"], info["ntiles"], info["row_groups"], info["eval_grid"]) == (12, 7, 2, 256), info
        with pytest.raises(Exception):
            pb.tune(wide=3)                      # (runs of 12 rows: two row groups' registers per CU)
        assert pb.info()["row_groups"] == 2
    # a grid that does not fill the device stays on 4-wave workgroups: width would only empty compute units
    with _capi.Problem(3, 20, 505, Y[:505], Lidx, twin.DT, 4.0, 4e-6, P[:3], [0], disc="trapezoid", tile_rows=84) as pb:
        pb.tune(wide=1)
        assert pb.info()["row_groups"] == 1, pb.info()
    # more than one resident round: today's plan
    with _capi.Problem(64, 20, 5000, np.tile(Y, (5, 1))[:5000], Lidx, twin.DT, 4.0, 4e-6, P, [0], disc="trapezoid") as pb:
        pb.tune(wide=1)
        assert pb.info()["eval_kernel"] == 4 and pb.info()["row_groups"] == 1, pb.info()
