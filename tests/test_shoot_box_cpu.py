"""CPU: the boxed shooting kernel (csrc/va_shoot_box.h) without a GPU -- k_shoot's evaluation phases with the one-lane
L-BFGS-B step between them, run lane by lane on the host by a g++ build of tests/cpu_emul/shoot_box_check.cpp (the same
headers the kernel includes), against SciPy's L-BFGS-B with the same bounds around the NumPy adjoint
(tests/_shoot_box_cases.py, where the family, the boxes, the reference and the caps are written down); plan_shoot_box's
workspace (csrc/va_shoot_geo.h) and the refusals' texts."""
import os
import subprocess

import numpy as np
import pytest

import _shoot_box_cases as bc
import _shoot_cases as sc
from _adj_ref import TOL_ADJ
from _predict_ref import DT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("x0", "k", "cost", "cost_start", "grad_max", "nit", "nfev", "status")
SRC = os.path.join(ROOT, "tests", "cpu_emul", "shoot_box_check.cpp")
INC = os.path.join(ROOT, "varanneal_amd", "csrc")


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("shoot_box") / "shoot_box_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", INC, "-o", exe, SRC])
    return exe


def _fmt(v):
    return "%.17g" % v if np.isfinite(v) else ("inf" if v > 0 else ("-inf" if v < 0 else "nan"))


def _host_run(exe, tmp_path, x0, ks, Y, w, lo, hi, m=10, maxiter=15000, maxfun=15000, maxls=20, expect=0):
    T, D = x0.shape
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    vals = ["%.17g" % v for v in list(x0.ravel()) + list(ks)]
    vals += [str(D)] + [str(i) for i in range(D)] + ["%.17g" % v for v in list(w) + list(Y.ravel())]
    vals += ["1" if lo.ndim == 1 else "0"] + [_fmt(v) for v in list(lo.ravel()) + list(hi.ravel())]
    f, o = tmp_path / "in.txt", tmp_path / "out.bin"
    f.write_text("\n".join(vals) + "\n")
    run = subprocess.run([exe, "run", str(D), str(T), str(sc.N_ROWS - 1), repr(DT), str(m), str(maxiter), str(maxfun), str(maxls),
                          repr(sc.SHOOT_OPT_ARGS["ftol"]), repr(sc.SHOOT_OPT_ARGS["gtol"]), str(f), str(o)], capture_output=True, text=True)
    assert run.returncode == expect, (run.returncode, run.stderr)
    if expect:
        return run.stderr
    raw = np.fromfile(str(o))
    assert raw.size == T * D + 7 * T
    r = dict(zip(KEYS, np.split(raw, np.cumsum([T * D] + [T] * 6))))
    r["x0"] = r["x0"].reshape(T, D)
    for k in ("nit", "nfev", "status"):
        r[k] = r[k].astype(np.int64)
    r["geo"] = [int(v) for v in run.stdout.split()]
    return r


def _point(r, j):
    return {k: r[k][j] for k in KEYS}


def _feasible(r, j, lo, hi):
    z = np.append(r["x0"][j], r["k"][j])
    return bool(np.all(z >= lo) and np.all(z <= hi))


_runs = {}


@pytest.fixture
def together(check_exe, tmp_path):
    """the whole case of a width in one call, computed once"""
    def get(D):
        if D not in _runs:
            c = sc.case(D)
            lo, hi = bc.box(D)
            _runs[D] = _host_run(check_exe, tmp_path, c["x0"], c["k"], c["Y"], c["w"], lo, hi)
        return _runs[D]
    return get


@pytest.mark.parametrize("D", [5, 20, 33])
def test_convergence(together, D):
    """D = 5: a wave of six points, the second group with idle slots; D = 20: one wave, one point; D = 33: 128 threads with
    barriers.  Every point under _shoot_box_cases.check_point: status 0, inside its closed box exactly, k == 8.05,
    cost <= cost_start, cost no larger than the reference's plus 4e-15 per iteration, cost = the NumPy misfit at the returned
    point within TOL_ADJ, the largest projected-gradient entry there (NumPy adjoint) within 10 times the largest the
    reference leaves on the case, at most twice the reference's evaluations; and grad_max is the projected-gradient norm
    at the returned point."""
    r = together(D)
    assert r["geo"][:4] == {5: [6, 64, 1, 1], 20: [1, 64, 1, 1], 33: [1, 128, 1, 0]}[D]
    lo, hi = bc.box(D)
    for j in range(bc.WIDTHS[D]):
        bc.check_point(D, j, _point(r, j), "host emulation ")
        z = np.append(r["x0"][j], r["k"][j])
        pg = np.abs(bc.projected_gradient(z, sc.misfit(D, z, sc.case(D)["Y"][j])[1], lo[j], hi[j])).max()
        assert abs(r["grad_max"][j] - pg) <= 1e-6 * pg + 1e-12


def test_points_are_independent(check_exe, tmp_path, together):
    """the 7 points at D = 5 run together (six to a wave, one beside five idle slots) give each point the bits it gets when
    run alone, in every output"""
    c, r = sc.case(5), together(5)
    lo, hi = bc.box(5)
    for j in range(7):
        one = _host_run(check_exe, tmp_path, c["x0"][j:j + 1], c["k"][j:j + 1], c["Y"][j:j + 1], c["w"], lo[j:j + 1], hi[j:j + 1])
        for k in KEYS:
            assert np.array_equal(one[k][0], r[k][j]), (j, k)


def test_all_infinite_box(check_exe, tmp_path):
    """a shared all-infinite box at D = 5 meets _shoot_cases.check_point, the unbounded criteria (bit equality with k_shoot
    is not asked: the direction is formed through the compact form and the subspace step)"""
    c = sc.case(5)
    r = _host_run(check_exe, tmp_path, c["x0"], c["k"], c["Y"], c["w"], np.full(6, -np.inf), np.full(6, np.inf))
    for j in range(7):
        sc.check_point(5, j, _point(r, j), "all-infinite box ")


def test_start_outside_its_box(check_exe, tmp_path, together):
    """starts pushed 0.5 below a lower bound (entry 0) and k = 9 above its upper bound: the start is projected (the same
    point as a start ON those bounds: the same bits in every output), status 0, the result feasible"""
    c = sc.case(5)
    lo, hi = bc.box(5)
    x0, k = c["x0"].copy(), np.full(7, 9.0)
    x0[:, 0] = lo[:, 0] - 0.5
    r = _host_run(check_exe, tmp_path, x0, k, c["Y"], c["w"], lo, hi)
    x0p, kp = x0.copy(), np.full(7, bc.K_HI)
    x0p[:, 0] = lo[:, 0]
    rp = _host_run(check_exe, tmp_path, x0p, kp, c["Y"], c["w"], lo, hi)
    for j in range(7):
        assert r["status"][j] == 0 and _feasible(r, j, lo[j], hi[j]) and r["cost"][j] <= r["cost_start"][j]
        assert abs(r["cost_start"][j] - sc.misfit(5, np.append(x0p[j], kp[j]), c["Y"][j])[0]) <= TOL_ADJ * r["cost_start"][j]
        for key in KEYS:
            assert np.array_equal(r[key][j], rp[key][j]), (j, key)


def test_nothing_free_at_the_cauchy_point(check_exe, tmp_path):
    """lower = upper = start on all entries but entry 1.  Width inf: entry 1 is unbounded, the free set is {1} throughout, a
    one-variable fit.  Width 1e-4 (start +- 1e-4, less than the fit wants to move): the first Cauchy point lands on entry 1's
    bound, nothing is free, the subspace step is skipped, and the run still ends with status 0 at a feasible point, the
    fixed entries untouched to the bit, whose cost is the misfit there"""
    c = sc.case(5)
    z0 = np.hstack([c["x0"], c["k"][:, None]])
    for width in (np.inf, 1e-4):
        lo, hi = z0.copy(), z0.copy()
        lo[:, 1], hi[:, 1] = z0[:, 1] - width, z0[:, 1] + width
        r = _host_run(check_exe, tmp_path, c["x0"], c["k"], c["Y"], c["w"], lo, hi)
        for j in range(7):
            z = np.append(r["x0"][j], r["k"][j])
            cost, g = sc.misfit(5, z, c["Y"][j])
            pg = np.abs(bc.projected_gradient(z, g, lo[j], hi[j])).max()
            print("width %g point %d: status %d nit %d nfev %d cost %.17g from %.6g, projected gradient %.3e, entry 1 moved %.3e"
                  % (width, j, r["status"][j], r["nit"][j], r["nfev"][j], r["cost"][j], r["cost_start"][j], pg, z[1] - z0[j, 1]))
            assert r["status"][j] == 0 and _feasible(r, j, lo[j], hi[j])
            assert np.array_equal(np.delete(z, 1), np.delete(z0[j], 1))
            assert r["cost"][j] <= r["cost_start"][j] and abs(r["cost"][j] - cost) <= TOL_ADJ * cost
            # a one-variable problem: at the returned point the projected gradient is gone (gtol), or the last step's
            # decrease was below ftol max(|f|, 1) = 1e-15, which a gradient above 1e-6 would not allow on this scale
            assert pg <= 1e-6
            if width < np.inf:
                assert abs(z[1] - z0[j, 1]) == width or pg <= 1e-6


def test_budget(check_exe, tmp_path):
    """maxfun = 5: status 1, at most 6 evaluations, a feasible returned iterate, cost <= cost_start, and cost is the misfit AT
    the returned point (NumPy, TOL_ADJ relative): a trial that the budget cut off is not what comes back"""
    c = sc.case(5)
    lo, hi = bc.box(5)
    r = _host_run(check_exe, tmp_path, c["x0"], c["k"], c["Y"], c["w"], lo, hi, maxfun=5)
    for j in range(7):
        cost = sc.misfit(5, np.append(r["x0"][j], r["k"][j]), c["Y"][j])[0]
        print("point %d: status %d nfev %d nit %d cost %.17g (NumPy at the returned point %.17g) from %.6g"
              % (j, r["status"][j], r["nfev"][j], r["nit"][j], r["cost"][j], cost, r["cost_start"][j]))
        assert r["status"][j] == 1 and r["nfev"][j] <= 6 and r["cost"][j] <= r["cost_start"][j]
        assert _feasible(r, j, lo[j], hi[j])
        assert abs(r["cost"][j] - cost) <= TOL_ADJ * cost


def test_non_finite_start(check_exe, tmp_path, together):
    """x0[3] = 1e200 at point 1 (entry 3 has no bound at D = 5, so the projection leaves it): status 3, the point comes back
    unchanged, nothing raises; its wave neighbours (and point 6 in the other workgroup) have the bits of the clean run"""
    c, clean = sc.case(5), together(5)
    lo, hi = bc.box(5)
    assert lo[1, 3] == -np.inf and hi[1, 3] == np.inf
    x0 = c["x0"].copy()
    x0[1, 3] = 1e200
    r = _host_run(check_exe, tmp_path, x0, c["k"], c["Y"], c["w"], lo, hi)
    assert r["status"][1] == 3 and r["nit"][1] == 0 and r["nfev"][1] == 1 and not np.isfinite(r["cost"][1])
    assert np.array_equal(r["x0"][1], x0[1]) and r["k"][1] == c["k"][1]
    for j in (0, 2, 3, 4, 5, 6):
        for k in KEYS:
            assert np.array_equal(r[k][j], clean[k][j]), (j, k)


def test_refusals(check_exe, tmp_path):
    """lower > upper and NaN bounds are refused with the entry named; the options as in shoot_check"""
    c = sc.case(5)
    lo, hi = (v.copy() for v in bc.box(5))
    lo[2, 4] = hi[2, 4] = 1.0
    lo[2, 4] = 2.0
    msg = _host_run(check_exe, tmp_path, c["x0"], c["k"], c["Y"], c["w"], lo, hi, expect=3)
    assert "entry 4 of table 2" in msg and "lower" in msg and "upper" in msg
    lo, hi = (v.copy() for v in bc.box(5))
    hi[3, 5] = np.nan
    msg = _host_run(check_exe, tmp_path, c["x0"], c["k"], c["Y"], c["w"], lo, hi, expect=3)
    assert "entry 5 of table 3" in msg and "NaN" in msg
    lo, hi = bc.box(5)
    assert "maxfun" in _host_run(check_exe, tmp_path, c["x0"], c["k"], c["Y"], c["w"], lo, hi, maxfun=0, expect=3)
    assert "MAX_M" in _host_run(check_exe, tmp_path, c["x0"], c["k"], c["Y"], c["w"], lo, hi, m=33, expect=3)


@pytest.mark.parametrize("NP,NPest,m", [(1, 1, 10), (18, 4, 32)])
def test_workspace(check_exe, NP, NPest, m):
    """plan_shoot_box over D = 1 .. 513, planned for 7 points: plan_shoot's geometry, LDS and refusals; the per-point
    workspace is 7 n + 2 m n + 11 m^2 + 8 m doubles and 3 n ints packed two to a double behind them"""
    out = subprocess.run([check_exe, "geo", str(NP), str(NPest), str(m), "1", "513"], capture_output=True, text=True)
    assert out.returncode == 0
    lines = out.stdout.strip().splitlines()
    assert len(lines) == 513
    for D, ln in zip(range(1, 514), lines):
        w = ln.split()
        assert int(w[1]) == D
        if D == 513:
            assert w[0] == "NO" and "at most 512 columns" in ln
            continue
        if 8 * (6 * D + NP + D * (NP | 1)) + 8 > 64 * 1024:
            assert w[0] == "NO" and "do not fit 64 KiB of LDS" in ln
            continue
        assert w[0] == "OK", ln
        RW, threads, E, wave, lds, grid, n, pt, sRW, sthreads, sE, swave, slds, sgrid = (int(v) for v in w[2:16])
        assert (RW, threads, E, wave, lds, grid) == (sRW, sthreads, sE, swave, slds, sgrid)
        assert n == D + NPest
        assert pt == 7 * n + 2 * m * n + 11 * m * m + 8 * m + (3 * n + 1) // 2
        assert 8 * pt >= 8 * (7 * n + 2 * m * n + 11 * m * m + 8 * m) + 4 * 3 * n


def test_sanitizers(tmp_path):
    """the same stand-alone checker built with -fsanitize=address,undefined runs the D = 5 case (seven points together, then
    point 0 alone, whose workspace ends where the allocation ends) and the nothing-free case clean"""
    exe = str(tmp_path / "shoot_box_check_san")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", INC, "-o", exe, SRC])
    c = sc.case(5)
    lo, hi = bc.box(5)
    r = _host_run(exe, tmp_path, c["x0"], c["k"], c["Y"], c["w"], lo, hi)
    assert np.all(r["status"] == 0)
    one = _host_run(exe, tmp_path, c["x0"][:1], c["k"][:1], c["Y"][:1], c["w"], lo[:1], hi[:1], m=3)
    assert one["status"][0] == 0
    z0 = np.hstack([c["x0"], c["k"][:, None]])
    l2, h2 = z0.copy(), z0.copy()
    l2[:, 1], h2[:, 1] = z0[:, 1] - 1e-4, z0[:, 1] + 1e-4
    assert np.all(_host_run(exe, tmp_path, c["x0"], c["k"], c["Y"], c["w"], l2, h2)["status"] == 0)
