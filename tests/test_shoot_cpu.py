"""CPU: the shooting kernel (csrc/va_shoot.h) without a GPU -- the evaluation's phases re-armed trip after trip, the L-BFGS
step of one lane per point, freezing and the trip bound, run lane by lane on the host by a g++ build of
tests/cpu_emul/shoot_check.cpp (the same headers the kernel includes), against SciPy's L-BFGS-B around the NumPy adjoint
(tests/_shoot_cases.py, where the family, the reference and the bounds are written down); and plan_shoot's geometry
(csrc/va_shoot_geo.h) with the refusals' texts."""
import os
import subprocess

import numpy as np
import pytest

import _shoot_cases as sc
from _adj_ref import TOL_ADJ
from _predict_ref import DT, K_TRUE, l96, rk4

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("x0", "k", "cost", "cost_start", "grad_max", "nit", "nfev", "status")


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("shoot") / "shoot_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "varanneal_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpu_emul", "shoot_check.cpp")])
    return exe


def _host_run(exe, tmp_path, x0, ks, Y, w, m=10, maxiter=15000, maxfun=15000, maxls=20, expect=0):
    T, D = x0.shape
    vals = ["%.17g" % v for v in list(x0.ravel()) + list(ks)]
    vals += [str(D)] + [str(i) for i in range(D)] + ["%.17g" % v for v in list(w) + list(Y.ravel())]
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


_runs = {}


@pytest.fixture
def together(check_exe, tmp_path):
    """the whole case of a width in one call, computed once"""
    def get(D):
        if D not in _runs:
            c = sc.case(D)
            _runs[D] = _host_run(check_exe, tmp_path, c["x0"], c["k"], c["Y"], c["w"])
        return _runs[D]
    return get


@pytest.mark.parametrize("D", [5, 20, 33, 130])
def test_convergence(together, D):
    """(1) D = 5: a wave of six points, the second group with idle slots; D = 20: one wave, one point; D = 33: 128 threads
    with barriers; D = 130, two points: 256 threads, E = 2.  Every point: status 0, cost <= cost_start, cost no larger than
    the reference's plus 4e-15 per iteration, cost = the NumPy misfit at the returned point within TOL_ADJ, the largest
    gradient entry there (NumPy adjoint) within 10 times the largest the reference leaves on the case, at most twice the
    reference's evaluations.  The reference on these inputs (SciPy L-BFGS-B, SHOOT_OPT_ARGS, measured on the CPU):
        D = 5    nfev 19 .. 31,   nit 16 .. 27,  largest gradient entry 9.74e-9, cost 1.74e-3 .. 3.22e-3 from 3.58e-3 .. 1.04e-2
        D = 20   nfev 47 .. 57,   nit 42 .. 50,  9.56e-9, cost 2.18e-3 .. 2.65e-3 from 5.42e-3 .. 8.37e-3
        D = 33   nfev 66 .. 111,  nit 60 .. 99,  3.33e-8, cost 2.24e-3 .. 2.71e-3 from 5.37e-3 .. 7.23e-3
        D = 130  nfev 107, 110,   nit 99, 100,   5.71e-9, cost 2.44e-3, 2.54e-3 from 5.47e-3, 6.12e-3
    all with status 0."""
    r = together(D)
    assert r["geo"][:4] == {5: [6, 64, 1, 1], 20: [1, 64, 1, 1], 33: [1, 128, 1, 0], 130: [1, 256, 2, 0]}[D]
    assert r["geo"][5] == {5: 2, 20: 7, 33: 7, 130: 2}[D]
    for j in range(sc.WIDTHS[D]):
        sc.check_point(D, j, _point(r, j), "host emulation ")
        assert r["grad_max"][j] <= sc.SHOOT_OPT_ARGS["gtol"] or r["nit"][j] > 0


def test_points_are_independent(check_exe, tmp_path, together):
    """(2) the 7 points at D = 5 run together (six to a wave, one beside five idle slots) give each point the bits it gets
    when run alone, in every output"""
    c, r = sc.case(5), together(5)
    for j in range(7):
        one = _host_run(check_exe, tmp_path, c["x0"][j:j + 1], c["k"][j:j + 1], c["Y"][j:j + 1], c["w"])
        for k in KEYS:
            assert np.array_equal(one[k][0], r[k][j]), (j, k)


def test_a_finished_point_is_frozen(check_exe, tmp_path):
    """(3) D = 5, point 2 with noise-free data, started at the truth with k = K_TRUE: its gradient is zero to rounding, so it
    stops at the first evaluation (nit 0, nfev 1) and comes back bit for bit while its wave goes on for dozens of trips;
    the other five points of the wave (and the seventh) still meet (1)"""
    c = sc.case(5)
    x0, k, Y = c["x0"].copy(), c["k"].copy(), c["Y"].copy()
    x0[2], k[2] = c["truth"][2], K_TRUE
    Y[2] = rk4(l96, c["truth"][2], K_TRUE, sc.N_ROWS - 1, DT)
    r = _host_run(check_exe, tmp_path, x0, k, Y, c["w"])
    print("point 2: status %d nit %d nfev %d cost %.3e grad_max %.3e" % (r["status"][2], r["nit"][2], r["nfev"][2], r["cost"][2], r["grad_max"][2]))
    assert (r["status"][2], r["nit"][2], r["nfev"][2]) == (0, 0, 1)
    assert np.array_equal(r["x0"][2], x0[2]) and r["k"][2] == k[2] and r["cost"][2] == r["cost_start"][2]
    for j in (0, 1, 3, 4, 5, 6):
        sc.check_point(5, j, _point(r, j), "beside a frozen point ")


def test_budget(check_exe, tmp_path):
    """(4) maxfun = 5: status 1, at most 6 evaluations, cost <= cost_start, and cost is the misfit AT the returned point
    (NumPy, TOL_ADJ relative): a trial that the budget cut off is not what comes back"""
    c = sc.case(5)
    r = _host_run(check_exe, tmp_path, c["x0"], c["k"], c["Y"], c["w"], maxfun=5)
    for j in range(7):
        cost = sc.misfit(5, np.append(r["x0"][j], r["k"][j]), c["Y"][j])[0]
        print("point %d: status %d nfev %d nit %d cost %.17g (NumPy at the returned point %.17g) from %.6g"
              % (j, r["status"][j], r["nfev"][j], r["nit"][j], r["cost"][j], cost, r["cost_start"][j]))
        assert r["status"][j] == 1 and r["nfev"][j] <= 6 and r["cost"][j] <= r["cost_start"][j]
        assert abs(r["cost"][j] - cost) <= TOL_ADJ * cost


def test_non_finite_start(check_exe, tmp_path, together):
    """(5) x0[0] = 1e200 at point 1: status 3, the point comes back unchanged, nothing raises; its wave neighbours (and
    point 6 in the other workgroup) have the bits of the clean run"""
    c, clean = sc.case(5), together(5)
    x0 = c["x0"].copy()
    x0[1, 0] = 1e200
    r = _host_run(check_exe, tmp_path, x0, c["k"], c["Y"], c["w"])
    assert r["status"][1] == 3 and r["nit"][1] == 0 and r["nfev"][1] == 1 and not np.isfinite(r["cost"][1])
    assert np.array_equal(r["x0"][1], x0[1]) and r["k"][1] == c["k"][1]
    for j in (0, 2, 3, 4, 5, 6):
        for k in KEYS:
            assert np.array_equal(r[k][j], clean[k][j]), (j, k)


def _geo(exe, NP, NPest, m, D0, D1):
    out = subprocess.run([exe, "geo", str(NP), str(NPest), str(m), str(D0), str(D1)], capture_output=True, text=True)
    assert out.returncode == 0
    return out.stdout.strip().splitlines()


@pytest.mark.parametrize("NP,NPest,m", [(1, 1, 10), (18, 4, 32)])
def test_geometry(check_exe, NP, NPest, m):
    """(6) plan_shoot over D = 1 .. 513, planned for 7 points: RW, threads, E, wave and the grid are plan_predict_adj(D, 7, 1,
    NP, 0)'s; LDS is that plan's plus one flag per point slot; the per-point workspace is 3 n + 2 m + 2 m n doubles;
    refused at 513 with the limit in the text.  With 18 parameters the adjoint plan's own LDS refusal (D >= 327) passes through."""
    lines = _geo(check_exe, NP, NPest, m, 1, 513)
    assert len(lines) == 513
    for D, ln in zip(range(1, 514), lines):
        w = ln.split()
        assert int(w[1]) == D
        if D == 513:
            assert w[0] == "NO" and "at most 512 columns" in ln
            continue
        if 8 * (6 * D + NP + D * (NP | 1)) + 8 > 64 * 1024:               # (one point's images and partials, va_predict_adj_geo.h)
            assert w[0] == "NO" and "do not fit 64 KiB of LDS" in ln
            continue
        assert w[0] == "OK", ln
        RW, threads, E, wave, lds, grid, n, pt, aRW, athreads, aE, awave, alds, agrid = (int(v) for v in w[2:16])
        assert (RW, threads, E, wave, grid) == (aRW, athreads, aE, awave, agrid)
        assert lds == alds + 8 * RW <= 64 * 1024
        assert n == D + NPest and pt == 3 * n + 2 * m + 2 * m * n
        assert grid == -(-7 // RW) and E <= 4
        if D <= 16:
            assert (wave, threads, E) == (1, 64, 1) and RW >= 1 and RW <= 64 // (2 * D)
            if NP == 1:
                assert RW == 64 // (2 * D)
        elif D <= 32:
            assert (wave, threads, E, RW) == (1, 64, 1, 1)
        else:
            assert wave == 0 and RW == 1 and threads == min(256, -(-2 * D // 64) * 64) and E == -(-2 * D // threads)


def test_refusals(check_exe, tmp_path):
    assert "bad sizes" in _geo(check_exe, 1, 2, 10, 5, 5)[0]
    assert "1 to 32 pairs" in _geo(check_exe, 1, 1, 33, 5, 5)[0]

    def args(m, maxiter, maxfun, maxls):
        out = subprocess.run([check_exe, "args", str(m), str(maxiter), str(maxfun), str(maxls)], capture_output=True, text=True)
        assert out.returncode == 0
        return out.stdout.strip()
    assert args(10, 15000, 15000, 20) == "OK" and args(32, 1, 1, 1) == "OK" and args(10, 1, 100000, 20) == "OK"
    assert args(10, 15000, 0, 20).startswith("NO maxfun must be 1 .. 100000")
    assert args(10, 15000, 100001, 20).startswith("NO maxfun")
    assert args(33, 15000, 15000, 20).startswith("NO m must be 1 .. 32")
    assert args(0, 15000, 15000, 20).startswith("NO m ")
    assert args(10, 0, 15000, 20).startswith("NO maxiter")
    assert args(10, 15000, 15000, 0).startswith("NO maxls")
    c = sc.case(5)
    assert "maxfun" in _host_run(check_exe, tmp_path, c["x0"], c["k"], c["Y"], c["w"], maxfun=0, expect=3)
    assert "MAX_M" in _host_run(check_exe, tmp_path, c["x0"], c["k"], c["Y"], c["w"], m=33, expect=3)
