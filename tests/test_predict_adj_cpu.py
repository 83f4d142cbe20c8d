"""CPU: the adjoint predictor (csrc/va_predict_adj.h) without a GPU -- the transposed RK4 rule, the kernel's element / LDS
mapping, its checkpoints and the ordered sums of the parameter partials and the cost, run lane by lane on the host by a g++
build of tests/cpu_emul/predict_adj_check.cpp (the same header the kernel includes), against the adjoint written in NumPy
(tests/_adj_ref.py, where the tolerance is derived); and the launch geometry of csrc/va_predict_adj_geo.h at its boundaries,
with the refusals' texts."""
import os
import subprocess

import numpy as np
import pytest

import _adj_ref
from _adj_ref import TOL_ADJ, l96_adj_reference, row_error
from _predict_ref import DT, K_TRUE, STEPS
from _predict_ref import TOL as TOL_X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("predict_adj") / "predict_adj_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "varanneal_amd", "csrc"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpu_emul", "predict_adj_check.cpp")])
    return exe


def _host_run(exe, tmp_path, x0, ks, substeps, every, G=None, misfit=None):
    """misfit: (Lidx, w, Y) with Y (T, n_out, L) or (n_out, L)"""
    T, D = x0.shape
    n_out = STEPS // every + 1
    vals = ["%.17g" % v for v in list(x0.ravel()) + list(ks)]
    if G is not None:
        ncot, mode = G.shape[1], 0
        vals += ["%.17g" % v for v in G.ravel()]
    else:
        Lidx, w, Y = misfit
        ncot, mode = 1, 1 if Y.ndim == 3 else 2
        vals += [str(len(Lidx))] + [str(int(v)) for v in Lidx] + ["%.17g" % v for v in list(w) + list(Y.ravel())]
    f, o = tmp_path / "in.txt", tmp_path / "out.bin"
    f.write_text("\n".join(vals) + "\n")
    run = subprocess.run([exe, "traj", str(D), str(T), str(ncot), str(STEPS), str(substeps), str(every), repr(DT), str(mode), str(f), str(o)],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    raw = np.fromfile(str(o))
    sizes = [T * n_out * D, T * ncot * D, T * ncot, T]
    assert raw.size == sum(sizes)
    out, gx0, gp, cost = np.split(raw, np.cumsum(sizes)[:-1])
    return out.reshape(T, n_out, D), gx0.reshape(T, ncot, D), gp.reshape(T, ncot, 1), cost, [int(v) for v in run.stdout.split()]


def test_reference_is_the_transpose_of_the_tangent_reference():
    worst = _adj_ref.self_check()
    print("adjoint NumPy reference against the tangent-linear one in longdouble: %.3e relative to |G| |dX|" % worst)
    assert worst <= 1e-16


@pytest.mark.parametrize("D,ncot", [(5, 1), (20, 5), (64, 3), (67, 3)])
@pytest.mark.parametrize("substeps,every", [(1, 1), (2, 3)])
def test_host_path_matches_numpy_adjoint(check_exe, tmp_path, D, ncot, substeps, every):
    """7 trajectories.  D = 5, one set: a wave of six trajectories side by side, the second group with idle slots; D = 20,
    five sets: chunks of 2, 2 and 1; D = 64 and 67, three sets: workgroups of 256 lanes, idle lanes at D = 67"""
    T = 7
    x0, G, ref_x, ref_gx, ref_gp = l96_adj_reference(D, T, ncot, substeps, every)
    out, gx0, gp, _, geo = _host_run(check_exe, tmp_path, x0, [K_TRUE] * T, substeps, every, G=G)
    ex, eg, ep = np.abs(out - ref_x).max(), row_error(gx0, ref_gx), row_error(gp, ref_gp)
    print("D=%d ncot=%d substeps=%d every=%d geometry %s: nominal |host C++ - NumPy| = %.3e, gx0 relative per row = %.3e, gp = %.3e"
          % (D, ncot, substeps, every, geo, ex, eg, ep))
    assert np.array_equal(out[:, 0], x0)
    assert ex <= TOL_X and eg <= TOL_ADJ and ep <= TOL_ADJ
    assert np.abs(ref_gx).max() > 2.0 * np.abs(G[:, :, 0]).max()                            # (the cotangents do grow backward)
    if D == 5:
        assert geo[:6] == [6, 1, 1, 64, 1, 1] and geo[7] == 2
    if D == 20:
        assert geo[:6] == [1, 2, 3, 64, 1, 1] and geo[7] == 21
    if D == 67:
        assert geo[:6] == [1, 3, 1, 256, 2, 0]


def test_row_zero_cotangent_reaches_gx0_unchanged(check_exe, tmp_path):
    x0, G, _, _, _ = l96_adj_reference(20, 7, 5)
    G0 = np.zeros_like(G)
    G0[:, :, 0] = G[:, :, 0]
    _, gx0, gp, _, _ = _host_run(check_exe, tmp_path, x0, [K_TRUE] * 7, 1, 1, G=G0)
    assert np.array_equal(gx0, G[:, :, 0]) and np.array_equal(gp, np.zeros_like(gp))


@pytest.mark.parametrize("shared", [False, True])
def test_host_misfit_mode(check_exe, tmp_path, shared):
    """misfit mode against cotangent mode fed 2 w (out - Y), and against the NumPy cost: D = 20, columns 0, 3, ... observed
    in an order that is not ascending, (substeps, every) = (2, 3)"""
    D, T, substeps, every = 20, 7, 2, 3
    x0, _, ref_x, _, _ = l96_adj_reference(D, T, 1, substeps, every)
    Lidx = [3, 0, 6, 9, 18, 12, 15]
    rng = np.random.RandomState(4)
    w = 0.5 + rng.rand(len(Lidx))
    Y = ref_x[:, :, Lidx] + 0.3 * rng.randn(T, ref_x.shape[1], len(Lidx))
    if shared:
        Y = Y[2]
    out, gx0, gp, cost, _ = _host_run(check_exe, tmp_path, x0, [K_TRUE] * T, substeps, every, misfit=(Lidx, w, Y))
    G = np.zeros((T, 1) + ref_x.shape[1:])
    G[:, 0][:, :, Lidx] = 2.0 * w * (out[:, :, Lidx] - Y)
    _, gx0_c, gp_c, _, _ = _host_run(check_exe, tmp_path, x0, [K_TRUE] * T, substeps, every, G=G)
    assert row_error(gx0, gx0_c) <= TOL_ADJ and row_error(gp, gp_c) <= TOL_ADJ
    for i in (0, 5):
        c, g, q, _ = _adj_ref.misfit_rk4(_adj_ref.l96, _adj_ref.l96_vjp, _adj_ref.l96_pgrad, x0[i], K_TRUE, Y if shared else Y[i], Lidx, w,
                                         STEPS, DT, substeps=substeps, every=every)
        assert abs(cost[i] - c) <= TOL_ADJ * c
        assert row_error(gx0[i, 0], g) <= TOL_ADJ and row_error(gp[i, 0], q) <= TOL_ADJ


def _geo(exe, ncot, NP, D0, D1):
    out = subprocess.run([exe, "geo", str(ncot), str(NP), str(D0), str(D1)], capture_output=True, text=True)
    assert out.returncode == 0
    return out.stdout.strip().splitlines()


def _lds(RW, chunk, D, NP, nstim=0):
    return 8 * (RW * (4 * D + 2 * chunk * D + NP + chunk * D * (NP | 1)) + 6 * nstim)


@pytest.mark.parametrize("ncot", [1, 2, 5, 21, 65])
def test_geometry(check_exe, ncot):
    """widths 1 .. 1025, planned for T = 3 and one parameter: the check program runs the kernel's own load phase on every lane
    of every workgroup and counts; the plan's figures against the rules of va_predict_adj_geo.h"""
    lines = _geo(check_exe, ncot, 1, 1, 1025)
    assert len(lines) == 1025
    for D, ln in zip(range(1, 1026), lines):
        w = ln.split()
        assert int(w[1]) == D
        if D == 1025:
            assert w[0] == "NO" and "1024" in ln
            continue
        assert w[0] == "OK", ln
        RW, chunk, nchunks, threads, E, wave, lds, grid = (int(v) for v in w[2:10])
        assert w[10:15] == ["1"] * 5, ln
        assert chunk >= 1 and chunk * nchunks >= ncot > chunk * (nchunks - 1)
        assert grid == -(-3 // RW) * nchunks
        assert lds == _lds(RW, chunk, D, 1) and lds <= 64 * 1024
        assert E * threads >= RW * (chunk + 1) * D
        if 2 * D <= 64:
            assert wave == 1 and threads == 64 and E == 1 and RW * (chunk + 1) * D <= 64
            assert (RW == 64 // ((ncot + 1) * D) and chunk == ncot) if (ncot + 1) * D <= 64 else (RW == 1 and chunk <= 64 // D - 1)
        else:
            assert wave == 0 and RW == 1 and threads % 64 == 0 and threads == min(256, -(-(chunk + 1) * D // 64) * 64)
            assert E == -(-(chunk + 1) * D // threads)
            assert E <= 4 if D <= 512 else (chunk == 1 and 5 <= E <= 8)


def test_geometry_boundaries(check_exe):
    """the figures (RW, chunk, nchunks, threads, E, wave, LDS bytes) on both sides of every boundary"""
    def at(ncot, D, NP=1):
        w = _geo(check_exe, ncot, NP, D, D)[0].split()
        assert w[0] == "OK", w
        return [int(v) for v in w[2:9]]
    # (ncot + 1) D = 64 and 65: all sets of a trajectory in one wave / chunks of a lone trajectory
    assert at(3, 16) == [1, 3, 1, 64, 1, 1, _lds(1, 3, 16, 1)]
    assert at(7, 8) == [1, 7, 1, 64, 1, 1, _lds(1, 7, 8, 1)]
    assert at(4, 13) == [1, 2, 2, 64, 1, 1, _lds(1, 2, 13, 1)]           # 65: 4 slots to the wave, even chunks of 2
    assert at(1, 16) == [2, 1, 1, 64, 1, 1, _lds(2, 1, 16, 1)]           # two trajectories side by side
    # 2 D = 64 and 66: the last single wave / the first workgroup with barriers
    assert at(1, 32) == [1, 1, 1, 64, 1, 1, _lds(1, 1, 32, 1)]
    assert at(3, 32) == [1, 1, 3, 64, 1, 1, _lds(1, 1, 32, 1)]
    assert at(1, 33) == [1, 1, 1, 128, 1, 0, _lds(1, 1, 33, 1)]
    assert at(3, 33) == [1, 3, 1, 192, 1, 0, _lds(1, 3, 33, 1)]
    # D = 512 and 513: the last E <= 4 / one set beside the nominal with E = 5
    assert at(3, 512) == [1, 1, 3, 256, 4, 0, _lds(1, 1, 512, 1)]
    assert at(3, 513) == [1, 1, 3, 256, 5, 0, _lds(1, 1, 513, 1)]
    assert at(1, 1024) == [1, 1, 1, 256, 8, 0, 57352]
    # many parameters: fewer sets per workgroup before refusing (D = 20, 24 parameters: a set takes 20 * 25 + 40 doubles)
    RW, chunk, nchunks, threads, E, wave, lds = at(21, 20, NP=24)
    assert (RW, wave, threads, E) == (1, 1, 64, 1) and chunk == 2 and nchunks == 11 and lds == _lds(1, 2, 20, 24)
    RW, chunk, nchunks, threads, E, wave, lds = at(8, 100, NP=24)
    assert (RW, wave) == (1, 0) and chunk == 2 and nchunks == 4 and lds == _lds(1, 2, 100, 24) <= 65536 < _lds(1, 3, 100, 24)
    assert (threads, E) == (256, 2)


def test_refusals(check_exe):
    def no(ncot, D, NP):
        ln = _geo(check_exe, ncot, NP, D, D)[0]
        assert ln.startswith("NO %d " % D), ln
        return ln
    assert "at most 1024 columns" in no(1, 1025, 1)
    assert "do not fit 64 KiB of LDS" in no(1, 1024, 2)                  # 4 D + 2 D + 3 D doubles: 72 KiB
    assert "do not fit 64 KiB of LDS" in no(1, 100, 128)
    assert "bad sizes" in no(0, 20, 1)
