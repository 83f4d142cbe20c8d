"""CPU: the forecast kernels (csrc/va_predict.h, va_predict_tlm.h, va_predict_adj.h, va_shoot.h) at every lane geometry
their planners emit, without a GPU.  tests/_forecast_shapes.py lists the shapes and the plan each must get; here the
planners are held to that table through the check programs of tests/cpu_emul/ (the headers the kernels include), the table
is held to the launchers' instantiations (every (kernel, wave / barrier, E) is reached by some entry), and the host
emulations -- the kernels' own phases, lane by lane -- run at every wide entry against the NumPy references of
_predict_ref.py, _tlm_ref.py and _adj_ref.py, where the bounds are derived for these widths.  The device runs of the same
entries are in tests/test_gpu_forecast_geometry.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import _adj_ref
import _forecast_shapes as fs
import _shoot_cases as sc
import _tlm_ref
from _adj_ref import TOL_ADJ, TOL_ADJ_MISFIT_WIDE
from _predict_ref import DT, K_TRUE, STEPS, TOL_WIDE, l96_reference
from _tlm_ref import TOL, ordered_sums, row_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "varanneal_amd", "csrc")
PAIRS = [(1, 1), (2, 3)]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("forecast_geometry")
    built = {}
    for name in ("predict", "predict_tlm", "predict_adj", "shoot"):
        built[name] = str(d / (name + "_check"))
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", CSRC, "-o", built[name],
                               os.path.join(ROOT, "tests", "cpu_emul", name + "_check.cpp")])
    return built


def _lines(cmd):
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return out.stdout.strip().splitlines()


def _plan(exe, kernel, shape, NP=1):
    """(wave, threads, E, chunk, nchunks, RW), the LDS bytes and the rest of the check program's line"""
    if kernel == "k_predict":
        w = _lines([exe["predict"], "geo", str(shape)])[0].split()
        assert w[0] == "OK", w
        RW, threads, E, wave, lds = (int(v) for v in w[2:7])
        return (wave, threads, E, None, None, RW), lds, []
    if kernel == "k_shoot":
        w = _lines([exe["shoot"], "geo", str(NP), "1", "10", str(shape[0]), str(shape[0])])[0].split()
        assert w[0] == "OK", w
        RW, threads, E, wave, lds = (int(v) for v in w[2:7])
        # (plan_shoot takes plan_predict_adj's plan for one cotangent set: the launcher refuses any other chunk)
        assert [int(v) for v in w[10:14]] == [RW, threads, E, wave]
        return (wave, threads, E, 1, 1, RW), lds, []
    D, n = shape
    cmd = [exe["predict_tlm"], "geo", str(n), str(D), str(D)] if kernel == "k_predict_tlm" else \
        [exe["predict_adj"], "geo", str(n), str(NP), str(D), str(D)]
    w = _lines(cmd)[0].split()
    assert w[0] == "OK", w
    RW, chunk, nchunks, threads, E, wave, lds = (int(v) for v in w[2:9])
    return (wave, threads, E, chunk, nchunks, RW), lds, w[10:15]


ENTRIES = [(k, s) for k in sorted(fs.TABLE) for s, _, _ in fs.TABLE[k]]


@pytest.mark.parametrize("kernel,shape", ENTRIES, ids=["%s-%s" % (k, s) for k, s in ENTRIES])
def test_plan_is_the_tables(exe, kernel, shape):
    """the planner gives every entry the plan the table states; for the tangent and the adjoint the check program also runs
    the kernel's load phase on every lane of every workgroup (T = 3) and finds every (trajectory, direction, column) and
    every nominal output column with exactly one lane, every workgroup's nominal carried once"""
    plan, _, cover = _plan(exe, kernel, shape)
    assert plan == fs.expected(kernel, shape)
    assert cover in ([], ["1"] * 5)
    wave, threads, E = plan[:3]
    D = shape if kernel == "k_predict" else shape[0]
    elems = D if kernel == "k_predict" else (plan[3] + 1) * D
    if not wave:
        assert threads == min(256, -(-elems // 64) * 64) and E == -(-elems // threads)


def test_adjoint_chunk_shrinks_to_fit_the_lds(exe):
    """D = NP = 40, 6 cotangent sets (_forecast_shapes.ADJ_SHRINK, with the arithmetic): 24 sets would fit the lanes, 4 fit
    64 KiB, and the 6 go evenly over the 2 workgroups that 4 need: chunks of 3 and 3.  The same shape with one parameter
    keeps all 6 in one workgroup: it is the parameter partials that shrink the chunk."""
    c = fs.ADJ_SHRINK
    plan, lds, cover = _plan(exe, "k_predict_adj", (c["D"], c["ncot"]), NP=c["NP"])
    assert plan == c["plan"] and lds == c["lds_bytes"] and cover == ["1"] * 5
    one = lambda chunk: 8 * (4 * 40 + 40 + chunk * (2 * 40 + 40 * 41))
    assert one(3) == lds and one(4) <= 65536 < one(5)
    assert _plan(exe, "k_predict_adj", (40, 6), NP=1)[0] == (0, 256, 2, 6, 1, 1)


def test_adjoint_fewer_trajectories_side_by_side(exe):
    """The adjoint planner's `--g.RW` loop (fewer trajectories side by side before fewer sets) IS reachable without
    stimulus columns, though only just.  RW > 1 needs RW (ncot + 1) D <= 64, and the LDS takes, in doubles,
        RW (4 D + 2 ncot D + NP + ncot D (NP | 1)).
    With a = RW D <= 32 and b = RW ncot D <= 64 - a this is 4 a + 2 b + RW NP + b (NP | 1) <= 132 a + 131 b at NP = 128
    (RW <= a), largest at a = b = 32, i.e. D = 1, ncot = 1, RW = 32:
        32 (4 + 2 + NP + (NP | 1)) doubles > 8192  <=>  NP + (NP | 1) > 250  <=>  NP >= 126.
    So a one-column model with 126 to 128 parameters (128 is the most a flat form carries) plans RW = 31, and D = 1 with
    two sets at NP = 128 plans 20 for 21; D = 2 already fits (16 (8 + 4 + 128 + 2 * 129) = 6368 doubles).  The check program
    runs the load phase under these plans too: one lane per output, the nominal once per live trajectory."""
    def at(ncot, NP, D=1):
        plan, lds, cover = _plan(exe, "k_predict_adj", (D, ncot), NP=NP)
        assert cover == ["1"] * 5 and lds <= 65536
        assert lds == 8 * plan[5] * (4 * D + 2 * plan[3] * D + NP + plan[3] * D * (NP | 1))
        return plan
    assert at(1, 125) == (1, 64, 1, 1, 1, 32)                       # 32 * 256 doubles: exactly 64 KiB
    for NP in (126, 127, 128):
        assert at(1, NP) == (1, 64, 1, 1, 1, 31)
        assert 8 * 32 * (6 + NP + (NP | 1)) > 65536
    assert at(2, 128) == (1, 64, 1, 2, 1, 20)
    assert at(1, 128, D=2) == (1, 64, 1, 1, 1, 16)


def _max_e():
    """E of the widest instantiation per kernel, read from the headers that the launchers' switch statements end at"""
    src = "".join(open(os.path.join(CSRC, f)).read() for f in ("va_predict_geo.h", "va_predict_tlm_geo.h", "va_predict_adj_geo.h", "va_shoot.h"))
    const = {k: int(v) for k, v in re.findall(r"constexpr int (PREDICT(?:_TLM|_ADJ)?_MAX_E) = (\d+);", src)}
    assert sorted(const) == ["PREDICT_ADJ_MAX_E", "PREDICT_MAX_E", "PREDICT_TLM_MAX_E"]
    assert "g.E > PREDICT_MAX_E" in src                                # (k_shoot's launcher: the predictor's four)
    return {"k_predict": const["PREDICT_MAX_E"], "k_predict_tlm": const["PREDICT_TLM_MAX_E"],
            "k_predict_adj": const["PREDICT_ADJ_MAX_E"], "k_shoot": const["PREDICT_MAX_E"]}


def test_table_reaches_every_instantiation(exe):
    """every launcher names one wave instantiation (E = 1) and the barrier instantiations E = 1 .. its largest E (4 for
    k_predict and k_shoot, 8 for k_predict_tlm and k_predict_adj): the table's entries, under the plans the planners really
    give them, reach all 28, and every wide entry reaches one that no narrow entry does"""
    max_e = _max_e()
    assert max_e == {"k_predict": 4, "k_predict_tlm": 8, "k_predict_adj": 8, "k_shoot": 4}
    narrow = {"k_predict": fs.PREDICT_NARROW, "k_predict_tlm": fs.TLM_NARROW, "k_predict_adj": fs.ADJ_NARROW, "k_shoot": fs.SHOOT_NARROW}
    missing = []
    for kernel in sorted(fs.TABLE):
        want = {("wave", 1)} | {("barrier", e) for e in range(1, max_e[kernel] + 1)}
        reached, old = {}, set()
        for shape, _, _ in fs.TABLE[kernel]:
            wave, _, E = _plan(exe, kernel, shape)[0][:3]
            inst = ("wave" if wave else "barrier", E)
            reached.setdefault(inst, []).append(shape)
            if shape in [s for s, _, _ in narrow[kernel]]:
                old.add(inst)
        for inst in sorted(want):
            print("%-14s %-7s E = %d  reached by %s" % (kernel, inst[0], inst[1], reached.get(inst, "NOTHING")))
        missing += [(kernel,) + inst for inst in sorted(want - set(reached))]
        assert set(reached) <= want
        new = {inst for inst, shapes in reached.items() if inst not in old}
        assert new == want - old                                       # (the wide entries are there for what was never run)
    assert not missing, missing


# ----------------------------------------------------------------------------------------------- arithmetic, host emulation
def _write(path, *arrays):
    path.write_text("\n".join("%.17g" % v for a in arrays for v in np.ravel(a)) + "\n")


@pytest.mark.parametrize("D", [s for s, _, _ in fs.PREDICT_WIDE])
@pytest.mark.parametrize("substeps,every", PAIRS)
def test_predict_host_at_wide_states(exe, tmp_path, D, substeps, every):
    """E = 2, 3, 4: lanes that own a column in the last pass and lanes that do not (D = 257, 513, 769: one lane does), and
    every lane full (D = 1024); absolute on the states within _predict_ref.TOL_WIDE"""
    x0, ref = l96_reference(D, fs.T, substeps, every)
    f = tmp_path / "in.txt"
    _write(f, x0, [K_TRUE] * fs.T)
    out = _lines([exe["predict"], "traj", str(D), str(fs.T), str(STEPS), str(substeps), str(every), repr(DT), str(f)])
    got = np.array([float(v) for v in out]).reshape(ref.shape)
    assert np.array_equal(got[:, 0], x0)
    err = np.abs(got - ref).max()
    print("D=%d substeps=%d every=%d  max |host C++ - NumPy| = %.3e (bound %.1e)" % (D, substeps, every, err, TOL_WIDE))
    assert err <= TOL_WIDE


SLOTS = [s for s, _, _ in fs.SLOTS_WIDE]


@pytest.mark.parametrize("D,nvec", SLOTS)
@pytest.mark.parametrize("substeps,every", PAIRS)
def test_tangent_host_at_wide_shapes(exe, tmp_path, D, nvec, substeps, every):
    """the barrier form at E = 1 .. 8 with mixed directions: nominal absolute within TOL_WIDE, tangents relative per row
    within _tlm_ref.TOL, var (and cov, up to D = 200) bit-equal to the ordered sums of dX"""
    V = fs.directions(D, nvec)
    x0, V0, ref_x, ref_dx = _tlm_ref.l96_tlm_reference(D, fs.T, substeps, every, V=V)
    f, o = tmp_path / "in.txt", tmp_path / "out.bin"
    _write(f, x0, [K_TRUE] * fs.T, V0)
    cov = D <= 200
    geo = _lines([exe["predict_tlm"], "traj", str(D), str(fs.T), str(nvec), str(STEPS), str(substeps), str(every), repr(DT), str(f), str(o)]
                 + ([] if cov else ["nocov"]))[0].split()
    n_out = STEPS // every + 1
    sizes = [fs.T * n_out * D, fs.T * nvec * n_out * D, fs.T * n_out * D, fs.T * n_out * D * D if cov else 0]
    raw = np.fromfile(str(o))
    assert raw.size == sum(sizes)
    out, dX, var, cv = np.split(raw, np.cumsum(sizes)[:-1])
    out, dX, var = out.reshape(ref_x.shape), dX.reshape(ref_dx.shape), var.reshape(ref_x.shape)
    wave, threads, E, chunk, nchunks, RW = fs.expected("k_predict_tlm", (D, nvec))
    assert [int(v) for v in geo[:6]] == [RW, chunk, nchunks, threads, E, wave]
    assert np.array_equal(out[:, 0], x0) and np.array_equal(dX[:, :, 0], V0[:, :, :D])
    ex, ed = np.abs(out - ref_x).max(), row_error(dX, ref_dx)
    print("D=%d nvec=%d substeps=%d every=%d E=%d: nominal |host C++ - NumPy| = %.3e (bound %.1e), tangents relative per row = %.3e (bound %.1e)"
          % (D, nvec, substeps, every, E, ex, TOL_WIDE, ed, TOL))
    assert ex <= TOL_WIDE and ed <= TOL
    if cov:
        v, c = ordered_sums(dX)
        assert np.array_equal(var, v) and np.array_equal(cv.reshape(c.shape), c)
    else:
        v = np.zeros(var.shape)
        for k in range(nvec):                                          # (ordered_sums' var, without its cov)
            v = v + dX[:, k] * dX[:, k]
        assert np.array_equal(var, v)


def _adj_run(exe, tmp_path, x0, substeps, every, G=None, misfit=None):
    T, D = x0.shape
    n_out = STEPS // every + 1
    f, o = tmp_path / "in.txt", tmp_path / "out.bin"
    if G is not None:
        ncot, mode = G.shape[1], 0
        _write(f, x0, [K_TRUE] * T, G)
    else:
        Lidx, w, Y = misfit
        ncot, mode = 1, 1
        f.write_text("\n".join(["%.17g" % v for v in list(x0.ravel()) + [K_TRUE] * T] + [str(len(Lidx))] + [str(i) for i in Lidx]
                               + ["%.17g" % v for v in list(w) + list(Y.ravel())]) + "\n")
    geo = _lines([exe["predict_adj"], "traj", str(D), str(T), str(ncot), str(STEPS), str(substeps), str(every), repr(DT), str(mode), str(f), str(o)])
    raw = np.fromfile(str(o))
    sizes = [T * n_out * D, T * ncot * D, T * ncot, T]
    assert raw.size == sum(sizes)
    out, gx0, gp, cost = np.split(raw, np.cumsum(sizes)[:-1])
    return out.reshape(T, n_out, D), gx0.reshape(T, ncot, D), gp.reshape(T, ncot, 1), cost, [int(v) for v in geo[0].split()]


@pytest.mark.parametrize("D,ncot", SLOTS)
@pytest.mark.parametrize("substeps,every", PAIRS)
def test_adjoint_host_at_wide_shapes(exe, tmp_path, D, ncot, substeps, every):
    """the barrier form at E = 1 .. 8, cotangent mode: nominal absolute within TOL_WIDE, gx0 and gp relative per row within
    _adj_ref.TOL_ADJ"""
    x0, G, ref_x, ref_gx, ref_gp = _adj_ref.l96_adj_reference(D, fs.T, ncot, substeps, every)
    out, gx0, gp, _, geo = _adj_run(exe, tmp_path, x0, substeps, every, G=G)
    wave, threads, E, chunk, nchunks, RW = fs.expected("k_predict_adj", (D, ncot))
    assert geo[:6] == [RW, chunk, nchunks, threads, E, wave]
    assert np.array_equal(out[:, 0], x0)
    ex, eg, ep = np.abs(out - ref_x).max(), row_error(gx0, ref_gx), row_error(gp, ref_gp)
    print("D=%d ncot=%d substeps=%d every=%d E=%d: nominal |host C++ - NumPy| = %.3e (bound %.1e), gx0 relative per row = %.3e, gp = %.3e (bound %.1e)"
          % (D, ncot, substeps, every, E, ex, TOL_WIDE, eg, ep, TOL_ADJ))
    assert ex <= TOL_WIDE and eg <= TOL_ADJ and ep <= TOL_ADJ


@pytest.mark.parametrize("D", [300, 1024])
def test_adjoint_host_misfit_mode_at_wide_states(exe, tmp_path, D):
    """misfit mode at E = 3 and E = 8 (one set beside the nominal) against _adj_ref.misfit_rk4: cost, gx0 and gp within
    _adj_ref.TOL_ADJ_MISFIT_WIDE relative"""
    x0, Lidx, w, Y = _adj_ref.misfit_inputs(D, fs.T)
    _, gx0, gp, cost, geo = _adj_run(exe, tmp_path, x0, 2, 3, misfit=(Lidx, w, Y))
    assert geo[4] == {300: 3, 1024: 8}[D]
    worst = 0.0
    for i in range(fs.T):
        c, g, q, _ = _adj_ref.misfit_rk4(_adj_ref.l96, _adj_ref.l96_vjp, _adj_ref.l96_pgrad, x0[i], K_TRUE, Y[i], Lidx, w, STEPS, DT,
                                         substeps=2, every=3)
        worst = max(worst, abs(cost[i] - c) / c, row_error(gx0[i, 0], g), row_error(gp[i, 0], q))
    print("D=%d misfit mode: cost, gx0, gp relative, largest = %.3e (bound %.1e)" % (D, worst, TOL_ADJ_MISFIT_WIDE))
    assert worst <= TOL_ADJ_MISFIT_WIDE


# ----------------------------------------------------------------------------------------------- shooting
KEYS = ("x0", "k", "cost", "cost_start", "grad_max", "nit", "nfev", "status")
MAXFUN = 8


def _shoot_run(exe, tmp_path, D, x0, ks, Y, w):
    T = len(x0)
    f, o = tmp_path / "in.txt", tmp_path / "out.bin"
    f.write_text("\n".join(["%.17g" % v for v in list(x0.ravel()) + list(ks)] + [str(D)] + [str(i) for i in range(D)]
                           + ["%.17g" % v for v in list(w) + list(Y.ravel())]) + "\n")
    geo = _lines([exe["shoot"], "run", str(D), str(T), str(sc.N_ROWS - 1), repr(DT), "10", "15000", str(MAXFUN), "20",
                  repr(sc.SHOOT_OPT_ARGS["ftol"]), repr(sc.SHOOT_OPT_ARGS["gtol"]), str(f), str(o)])
    raw = np.fromfile(str(o))
    assert raw.size == T * D + 7 * T
    r = dict(zip(KEYS, np.split(raw, np.cumsum([T * D] + [T] * 6))))
    r["x0"] = r["x0"].reshape(T, D)
    r["geo"] = [int(v) for v in geo[0].split()]
    return r


@pytest.mark.parametrize("D,points", [s for s, _, _ in fs.SHOOT_WIDE])
def test_shoot_host_at_wide_states(exe, tmp_path, D, points):
    """E = 3 and E = 4 under a budget of 8 evaluations (test_shoot_cpu.py::test_budget's criteria: no convergence case at
    these widths, the deciding lane is serial): status 1, at most 9 evaluations, cost < cost_start, cost is the NumPy misfit
    at the returned point within TOL_ADJ relative; and point 0 alone gets the bits it gets beside point 1"""
    c = sc.wide_case(D, points)
    r = _shoot_run(exe, tmp_path, D, c["x0"], c["k"], c["Y"], c["w"])
    wave, threads, E, _, _, RW = fs.expected("k_shoot", (D, points))
    assert r["geo"][:4] == [RW, threads, E, wave]
    for j in range(points):
        cost = sc.misfit(D, np.append(r["x0"][j], r["k"][j]), c["Y"][j])[0]
        print("D=%d point %d: status %d nfev %d nit %d cost %.17g (NumPy at the returned point %.17g) from %.6g"
              % (D, j, r["status"][j], r["nfev"][j], r["nit"][j], r["cost"][j], cost, r["cost_start"][j]))
        assert r["status"][j] == 1 and r["nfev"][j] <= MAXFUN + 1 and r["cost"][j] < r["cost_start"][j]
        assert abs(r["cost"][j] - cost) <= TOL_ADJ * cost
    one = _shoot_run(exe, tmp_path, D, c["x0"][:1], c["k"][:1], c["Y"][:1], c["w"])
    for k in KEYS:
        assert np.array_equal(one[k][0], r[k][0]), k
