"""GPU: the forecast kernels k_predict, k_predict_tlm, k_predict_adj and k_shoot at the wide lane geometries of
tests/_forecast_shapes.py -- E = 2 .. 4 of the predictor and the shooting kernel, the barrier form at E = 1 .. 8 of the
tangent and the adjoint, lanes that own elements past D and lanes that do not, chunks with an idle last slot -- against the
NumPy references of _predict_ref.py, _tlm_ref.py and _adj_ref.py (where the bounds are derived for these widths); generated
modules whose constant D compiles an E > 1 instantiation; the adjoint planner's chunk shrink on the device; and the
refusals that bound the table.  tests/test_forecast_geometry_cpu.py holds the planners and the host emulations to the same
table.  T = 3 trajectories, 40 steps."""
import numpy as np
import pytest

import _adj_ref
import _forecast_shapes as fs
import _shoot_cases as sc
from _adj_ref import TOL_ADJ, TOL_ADJ_MISFIT_WIDE, adj_rk4, l96_adj_reference, l96_pgrad, l96_vjp
from _predict_ref import DT, K_TRUE, STEPS, TOL, TOL_WIDE, attractor_starts, l96, l96_reference, rk4
from _tlm_ref import TOL as TOL_TLM
from _tlm_ref import l96_jvp, l96_tlm_reference, ordered_sums, row_error, tlm_rk4
from varanneal_amd import _capi, codegen

pytestmark = pytest.mark.gpu

T = fs.T
SLOTS = [s for s, _, _ in fs.SLOTS_WIDE]
P = np.full((T, 1), K_TRUE)


def _l96_user(t, x, k):
    return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - x + k


def _handle(D, N=5, Lidx=None, **kw):
    Lidx = list(range(0, D, 2)) if Lidx is None else Lidx
    return _capi.Problem(1, D, N, np.zeros((N, len(Lidx))), Lidx, DT, 4.0, 1e-2, kw.pop("P", np.array([[K_TRUE]])), kw.pop("Pidx", [0]), **kw)


def _same(a, b):
    return sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)


# ----------------------------------------------------------------------------------------------- predictor
@pytest.mark.parametrize("D", [s for s, _, _ in fs.PREDICT_WIDE])
@pytest.mark.parametrize("substeps,every", [(1, 1), (2, 3)])
def test_predict_at_wide_states(D, substeps, every):
    """E = 2 (D = 257), 3 (513) and 4 (769: one live lane in the last pass; 1024: every lane full)"""
    x0, ref = l96_reference(D, T, substeps, every)
    with _handle(D) as pb:
        got = pb.predict(x0, P, STEPS, substeps=substeps, every=every)
        again = pb.predict(x0, P, STEPS, substeps=substeps, every=every)
    assert got.shape == ref.shape
    assert np.array_equal(got[:, 0], x0)
    err = np.abs(got - ref).max()
    print("D=%d substeps=%d every=%d  max |device - NumPy| = %.3e (bound %.1e)" % (D, substeps, every, err, TOL_WIDE))
    assert err <= TOL_WIDE
    assert np.array_equal(got, again)


# ----------------------------------------------------------------------------------------------- tangent
WANT = ("dx", "var", "cov")
PAIR = dict(substeps=2, every=3)


@pytest.mark.parametrize("D,nvec", SLOTS)
def test_tangent_at_wide_shapes(D, nvec):
    """the barrier form at E = 1 .. 8, mixed directions, (substeps, every) = (2, 3): tangents against tlm_rk4, the nominal
    against NumPy and against predict(), var and cov bit-equal to the ordered sums of dx"""
    x0, V0, ref_x, ref_dx = l96_tlm_reference(D, T, V=fs.directions(D, nvec), **PAIR)
    with _handle(D) as pb:
        r = pb.predict_tangent(x0, P, V0, STEPS, want=WANT, **PAIR)
        plain = pb.predict(x0, P, STEPS, **PAIR)
    assert r["dx"].shape == ref_dx.shape and r["cov"].shape == ref_x.shape + (D,)
    assert np.array_equal(r["out"][:, 0], x0) and np.array_equal(r["dx"][:, :, 0], V0[:, :, :D])
    ex, ed, epl = np.abs(r["out"] - ref_x).max(), row_error(r["dx"], ref_dx), np.abs(r["out"] - plain).max()
    print("D=%d nvec=%d E=%d  nominal |device - NumPy| = %.3e, |device - predict()| = %.3e (bound %.1e), tangents relative per row = %.3e (bound %.1e)"
          % (D, nvec, fs.expected("k_predict_tlm", (D, nvec))[2], ex, epl, TOL_WIDE, ed, TOL_TLM))
    assert ex <= TOL_WIDE and epl <= TOL_WIDE
    assert ed <= TOL_TLM
    var, cov = ordered_sums(r["dx"])
    assert np.array_equal(r["var"], var) and np.array_equal(r["cov"], cov)


@pytest.mark.parametrize("D,nvec", SLOTS)
def test_tangent_second_call_gives_the_same_bits(D, nvec):
    x0, V0, _, _ = l96_tlm_reference(D, T, V=fs.directions(D, nvec), **PAIR)
    with _handle(D) as pb:
        r = pb.predict_tangent(x0, P, V0, STEPS, want=WANT, **PAIR)
        again = pb.predict_tangent(x0, P, V0, STEPS, want=WANT, **PAIR)
    assert _same(r, again)


# ----------------------------------------------------------------------------------------------- adjoint
@pytest.mark.parametrize("D,ncot", SLOTS)
def test_adjoint_at_wide_shapes(D, ncot):
    """the barrier form at E = 1 .. 8, cotangent mode, both (substeps, every) pairs: gx0 and gp against adj_rk4"""
    with _handle(D) as pb:
        for substeps, every in ((1, 1), (2, 3)):
            x0, G, ref_x, ref_gx, ref_gp = l96_adj_reference(D, T, ncot, substeps, every)
            r = pb.predict_adjoint(x0, P, STEPS, G=G, substeps=substeps, every=every)
            ex, eg, ep = np.abs(r["out"] - ref_x).max(), row_error(r["gx0"], ref_gx), row_error(r["gp"], ref_gp)
            print("D=%d ncot=%d substeps=%d every=%d E=%d  nominal |device - NumPy| = %.3e (bound %.1e), gx0 relative per row = %.3e, gp = %.3e "
                  "(bound %.1e)" % (D, ncot, substeps, every, fs.expected("k_predict_adj", (D, ncot))[2], ex, TOL_WIDE, eg, ep, TOL_ADJ))
            assert np.array_equal(r["out"][:, 0], x0)
            assert ex <= TOL_WIDE and eg <= TOL_ADJ and ep <= TOL_ADJ


@pytest.mark.parametrize("D,n", SLOTS)
def test_adjoint_transposes_the_tangent_kernel(D, n):
    """dX from predict_tangent along the entry's n mixed directions, the entry's n cotangent sets: <G_g, dX_c> =
    <gx0_g, v_x> + gp_g v_p for every pair, within (TOL + TOL_ADJ) |G_g| |dX_c| -- the bound of
    test_gpu_predict_adj.py::test_transpose_of_the_tangent_kernel, which _adj_ref.derive_transpose() finds to hold the
    references themselves with room at these widths"""
    V = fs.directions(D, n)
    x0, G, _, _, _ = l96_adj_reference(D, T, n, **PAIR)
    V0 = np.ascontiguousarray(np.broadcast_to(V, (T,) + V.shape))
    with _handle(D) as pb:
        dX = pb.predict_tangent(x0, P, V0, STEPS, want=("dx",), **PAIR)["dx"]
        r = pb.predict_adjoint(x0, P, STEPS, G=G, **PAIR)
    worst = 0.0
    for j in range(T):
        for g in range(n):
            for c in range(n):
                lhs = (G[j, g] * dX[j, c]).sum()
                rhs = np.dot(r["gx0"][j, g], V[c, :D]) + r["gp"][j, g, 0] * V[c, D]
                worst = max(worst, abs(lhs - rhs) / (np.linalg.norm(G[j, g]) * np.linalg.norm(dX[j, c])))
    print("D=%d n=%d: <G, dX_c> against <gx0, v_x> + gp v_p, largest defect relative to |G| |dX_c| = %.3e (bound %.1e)" % (D, n, worst, TOL_TLM + TOL_ADJ))
    assert worst <= TOL_TLM + TOL_ADJ


@pytest.mark.parametrize("D", [300, 1024])
def test_adjoint_misfit_mode_at_wide_states(D):
    """misfit mode with one set beside the nominal, E = 3 and E = 8: cost, gx0 and gp against misfit_rk4, relative within
    _adj_ref.TOL_ADJ_MISFIT_WIDE"""
    x0, Lidx, w, Y = _adj_ref.misfit_inputs(D, T)
    with _handle(D, Lidx=Lidx) as pb:
        r = pb.predict_adjoint(x0, P, STEPS, Y=Y, weights=w, **PAIR)
    worst = 0.0
    for i in range(T):
        c, g, q, _ = _adj_ref.misfit_rk4(l96, l96_vjp, l96_pgrad, x0[i], K_TRUE, Y[i], Lidx, w, STEPS, DT, **PAIR)
        worst = max(worst, abs(r["cost"][i] - c) / c, row_error(r["gx0"][i, 0], g), row_error(r["gp"][i, 0], q))
    print("D=%d misfit mode: cost, gx0, gp relative, largest = %.3e (bound %.1e)" % (D, worst, TOL_ADJ_MISFIT_WIDE))
    assert worst <= TOL_ADJ_MISFIT_WIDE


def test_every_trajectory_reads_its_own_parameters():
    """(300, 3): a forcing of its own per trajectory through all three kernels (E = 2 of the predictor, E = 4 of the others,
    two workgroups per trajectory): trajectory j's answer is the reference's for ITS forcing"""
    D, n = 300, 3
    ks = [8.17, 7.5, 9.0]
    p = np.array(ks)[:, None]
    x0, V0, ref_x, ref_dx = l96_tlm_reference(D, T, ks=ks, V=fs.directions(D, n))
    _, G, _, ref_gx, ref_gp = l96_adj_reference(D, T, n, ks=ks)
    with _handle(D) as pb:
        plain = pb.predict(x0, p, STEPS)
        t = pb.predict_tangent(x0, p, V0, STEPS, want=("dx",))
        a = pb.predict_adjoint(x0, p, STEPS, G=G)
    for j in range(T):
        assert max(np.abs(o[j] - ref_x[j]).max() for o in (plain, t["out"], a["out"])) <= TOL_WIDE, j
        assert row_error(t["dx"][j], ref_dx[j]) <= TOL_TLM, j
        assert row_error(a["gx0"][j], ref_gx[j]) <= TOL_ADJ and row_error(a["gp"][j], ref_gp[j]) <= TOL_ADJ, j
    assert np.abs(ref_x[1] - ref_x[0]).max() > 1e-2 and np.abs(ref_x[2] - ref_x[0]).max() > 1e-2     # (the forcings matter)


# ----------------------------------------------------------------------------------------------- generated modules
def test_generated_module_compiles_and_runs_e_above_one():
    """the generated Lorenz-96 at D = 300: its module compiles k_predict<..., 2> and, of the tangent and adjoint forms, the
    E its width can run; with 2 directions / 2 cotangent sets both plan 900 elements, E = 4.  Bounds: the predictor's and the
    adjoint's are those of the tests that hold a generated model to the same references at D <= 20 (TOL of
    test_gpu_predict.py::test_generated_lorenz96_with_a_forcing_per_site, widened to TOL_WIDE as derived for this width;
    TOL_ADJ = NAKL_ADJ_TOL of test_gpu_predict_adj.py); the tangent's is _tlm_ref.TOL"""
    D, n = 300, 2
    m = codegen.module_for(_l96_user, D, 1)
    x0, V0, ref_x, ref_dx = l96_tlm_reference(D, T, V=fs.directions(D, n), **PAIR)
    _, G, _, ref_gx, ref_gp = l96_adj_reference(D, T, n, **PAIR)
    with _handle(D, rhs=_capi.load_rhs_module(m["so"])) as pb:
        plain = pb.predict(x0, P, STEPS, **PAIR)
        t = pb.predict_tangent(x0, P, V0, STEPS, want=("dx",), **PAIR)
        a = pb.predict_adjoint(x0, P, STEPS, G=G, **PAIR)
    ex = max(np.abs(o - ref_x).max() for o in (plain, t["out"], a["out"]))
    ed, eg, ep = row_error(t["dx"], ref_dx), row_error(a["gx0"], ref_gx), row_error(a["gp"], ref_gp)
    print("generated D=300: nominal |device - NumPy| = %.3e (bound %.1e), tangents %.3e (bound %.1e), gx0 %.3e, gp %.3e (bound %.1e)"
          % (ex, TOL_WIDE, ed, TOL_TLM, eg, ep, TOL_ADJ))
    assert np.array_equal(plain[:, 0], x0)
    assert ex <= TOL_WIDE and ed <= TOL_TLM and eg <= TOL_ADJ and ep <= TOL_ADJ


def _persite():
    """the generated Lorenz-96 with a forcing per site at D = NP = 40, all estimated: (module, x0, P (T, 40))"""
    D = fs.ADJ_SHRINK["D"]
    m = codegen.module_for(_l96_user, D, D, colparams=True)
    return m, attractor_starts(D, T), K_TRUE + 0.5 * np.random.RandomState(13).randn(T, D)


def _persite_pgrad(t, x, p, st, s):
    """(df/dp)^T s with a forcing per site: df_i / dp_j = delta_ij, so the cotangent itself, (ncot, D)"""
    return s


def test_adjoint_chunk_shrink_on_the_device():
    """_forecast_shapes.ADJ_SHRINK: 6 cotangent sets at D = NP = 40 run as chunks of 3 and 3 because 64 KiB hold the parameter
    partials of 4 sets, not of 6 (the CPU plan test has the figures); gp has 40 entries per set"""
    c = fs.ADJ_SHRINK
    D, ncot = c["D"], c["ncot"]
    m, x0, Pp = _persite()
    G = _adj_ref.cotangents(D, T, ncot, STEPS + 1)
    ref = [adj_rk4(l96, l96_vjp, _persite_pgrad, x0[j], Pp[j], G[j], STEPS, DT, npe=D) for j in range(T)]
    with _handle(D, P=Pp[:1], Pidx=list(range(D)), rhs=_capi.load_rhs_module(m["so"])) as pb:
        r = pb.predict_adjoint(x0, Pp, STEPS, G=G)
    assert r["gp"].shape == (T, ncot, D)
    ex = max(np.abs(r["out"][j] - ref[j][0]).max() for j in range(T))
    eg = max(row_error(r["gx0"][j], ref[j][1]) for j in range(T))
    ep = max(row_error(r["gp"][j], ref[j][2]) for j in range(T))
    print("per-site forcing D=40, 6 sets: nominal %.3e (bound %.1e), gx0 %.3e, gp %.3e relative per row (bound %.1e)" % (ex, TOL, eg, ep, TOL_ADJ))
    assert ex <= TOL and eg <= TOL_ADJ and ep <= TOL_ADJ


def test_tangent_with_parameter_parts_per_site():
    """the same model through predict_tangent: 6 directions [state part | 40 forcing parts]"""
    D, nvec = fs.ADJ_SHRINK["D"], 6
    m, x0, Pp = _persite()
    V = np.random.RandomState(14).randn(nvec, 2 * D)
    ref = [tlm_rk4(l96, l96_jvp, x0[j], Pp[j], V, STEPS, DT) for j in range(T)]
    V0 = np.ascontiguousarray(np.broadcast_to(V, (T,) + V.shape))
    with _handle(D, P=Pp[:1], Pidx=list(range(D)), rhs=_capi.load_rhs_module(m["so"])) as pb:
        r = pb.predict_tangent(x0, Pp, V0, STEPS, want=("dx",))
    ex = max(np.abs(r["out"][j] - ref[j][0]).max() for j in range(T))
    ed = max(row_error(r["dx"][j], ref[j][1]) for j in range(T))
    print("per-site forcing D=40, 6 directions: nominal %.3e (bound %.1e), tangents relative per row %.3e (bound %.1e)" % (ex, TOL, ed, TOL_TLM))
    assert ex <= TOL and ed <= TOL_TLM


# ----------------------------------------------------------------------------------------------- shooting
KEYS = ("x0", "p", "cost", "cost_start", "grad_max", "nit", "nfev", "status")
MAXFUN = 8
_shots = {}


def _shoot_wide(D, x0, k, Y):
    N = sc.N_ROWS
    with _capi.Problem(1, D, N, np.zeros((N, D)), list(range(D)), DT, 4.0, 1e-2, np.array([[K_TRUE]]), [0]) as pb:
        return pb.shoot(x0, np.asarray(k, dtype=np.float64).reshape(-1, 1), N - 1, Y, np.full(D, 1.0 / (D * N)), maxfun=MAXFUN,
                        **sc.SHOOT_OPT_ARGS)


def _both(D, points):
    if D not in _shots:
        c = sc.wide_case(D, points)
        _shots[D] = _shoot_wide(D, c["x0"], c["k"], c["Y"])
    return _shots[D]


@pytest.mark.parametrize("D,points", [s for s, _, _ in fs.SHOOT_WIDE])
def test_shoot_under_a_budget_at_wide_states(D, points):
    """E = 3 (D = 300) and E = 4 (D = 512) with maxfun = 8, the criteria of test_gpu_shoot_device.py::test_budget: status 1, at
    most 9 evaluations, cost < cost_start, cost is the NumPy misfit at the returned point within TOL_ADJ relative; and the
    same bits on a second call"""
    c, r = sc.wide_case(D, points), _both(D, points)
    for j in range(points):
        cost = sc.misfit(D, np.append(r["x0"][j], r["p"][j, 0]), c["Y"][j])[0]
        print("D=%d point %d: status %d nfev %d nit %d cost %.17g (NumPy at the returned point %.17g) from %.6g"
              % (D, j, r["status"][j], r["nfev"][j], r["nit"][j], r["cost"][j], cost, r["cost_start"][j]))
        assert r["status"][j] == 1 and r["nfev"][j] <= MAXFUN + 1 and r["cost"][j] < r["cost_start"][j]
        assert abs(r["cost"][j] - cost) <= TOL_ADJ * cost
    again = _shoot_wide(D, c["x0"], c["k"], c["Y"])
    for k in KEYS:
        assert np.array_equal(r[k], again[k]), k


@pytest.mark.parametrize("D,points", [s for s, _, _ in fs.SHOOT_WIDE])
def test_shoot_points_are_independent_at_wide_states(D, points):
    """point 0 shot alone gets the bits it gets beside point 1"""
    c, r = sc.wide_case(D, points), _both(D, points)
    one = _shoot_wide(D, c["x0"][:1], c["k"][:1], c["Y"][:1])
    for k in KEYS:
        assert np.array_equal(one[k][0], r[k][0]), k


# ----------------------------------------------------------------------------------------------- refusals
def test_refusals_that_bound_the_table():
    """past the widest geometry each planner has, the call raises NotImplementedError with the planner's reason and the
    handle goes on working: predict at D = 1025, shoot at D = 513"""
    D = 1025
    x0 = attractor_starts(D, 1)
    with _handle(D) as pb:
        XP = np.append(np.tile(x0[0], 5), K_TRUE)[None, :]
        A0 = pb.action_grad(XP, 2.0)[0]
        with pytest.raises(NotImplementedError, match="at most 1024 columns"):
            pb.predict(x0, P[:1], STEPS)
        with pytest.raises(NotImplementedError, match="at most 1024 columns"):
            pb.predict_tangent(x0, P[:1], np.ones((1, 1, D + 1)), STEPS)
        with pytest.raises(NotImplementedError, match="at most 1024 columns"):
            pb.predict_adjoint(x0, P[:1], STEPS, G=np.ones((1, 1, STEPS + 1, D)))
        A1 = pb.action_grad(XP, 2.0)[0]
    assert np.isfinite(A0[0]) and A1[0] == A0[0]
    D = 513
    N = sc.N_ROWS
    x0, ref = l96_reference(D, 1)
    with _capi.Problem(1, D, N, np.zeros((N, D)), list(range(D)), DT, 4.0, 1e-2, np.array([[K_TRUE]]), [0]) as pb:
        with pytest.raises(NotImplementedError, match="at most 512 columns"):
            pb.shoot(x0, P[:1], N - 1, np.zeros((1, N, D)), np.full(D, 1.0 / (D * N)), maxfun=MAXFUN, **sc.SHOOT_OPT_ARGS)
        got = pb.predict(x0, P[:1], STEPS)
    assert np.abs(got - ref).max() <= TOL_WIDE


def _l96_two(t, x, k):
    return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - k[1] * x + k[0]


def test_adjoint_refuses_the_widest_state_with_two_parameters():
    """D = 1024 with two parameters: one cotangent set's images and partials take 4 D + 2 D + 3 D doubles, 72 KiB, and no
    smaller chunk exists; the predictor of the same handle still runs (Lorenz-96 with damping k[1] = 1: the reference's)"""
    D = 1024
    m = codegen.module_for(_l96_two, D, 2)
    x0, ref = l96_reference(D, T)
    p = np.tile([K_TRUE, 1.0], (T, 1))
    with _handle(D, P=p[:1], Pidx=[0, 1], rhs=_capi.load_rhs_module(m["so"])) as pb:
        with pytest.raises(NotImplementedError, match="do not fit 64 KiB of LDS"):
            pb.predict_adjoint(x0, p, STEPS, G=np.ones((T, 1, STEPS + 1, D)))
        got = pb.predict(x0, p, STEPS)
    assert np.abs(got - ref).max() <= TOL_WIDE
