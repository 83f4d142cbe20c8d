"""Evaluation kernels that need more than 64 KiB of LDS: the instantiation va_problem_create opts in (eval_op with
op.prepare, csrc/va_device.h) must be the one a launch runs -- a mismatch shows only above 64 KiB, as a refused launch.

The case table was made on the CPU with tests/cpu_emul/lds_check.cpp (the planner of va_eval_geo.h put through the
launchers' own size functions): per family the smallest (D, tile_rows) whose LDS exceeds 64 KiB, N a few tiles.
test_table_is_what_the_size_functions_give re-derives every row without a GPU.

    family   cells here                       LDS bytes   note
    flat     D=516 tile_rows=4, euler /        75232      every discretisation: the launcher picks the instantiation by it
             trapezoid / forwardmap
             D=412 tile_rows=3, Simpson-H.     70144
    eval3    D=66 tile_rows=50 (K=8)           68704
    eval4    D=6 tile_rows=244 (K=7)           72192
    eval5    none                              <= 62464   the planner offers no such shape: four ring slots are kept under
                                                          40 KiB, else three; the largest over D = 66..1024, every
                                                          discretisation, weight arrays and merr_nskip is 62464 B (D=200,
                                                          RM array, every column observed, line-search launch).  Neither launch kind can exceed
                                                          64 KiB, so no shape separates them either.
    k_seed   not repeated                      ~160 KiB   persist_geometry takes the longest slice that fits 160 KiB and
                                                          every instantiation is opted in (161304 B at D = 20, N = 41):
                                                          tests/test_gpu_persist.py runs it for the built-in and for a
                                                          module (test_generated_model_runs_the_persistent_kernel).
Each cell runs the built-in Lorenz-96 and a generated module of the same model.  The predictor through a module's table and
its refusal for a column-only module of more than 128 parameters (VA_EUNSUPPORTED) are tests/test_gpu_predict.py's
test_generated_module_with_stimulus / test_model_past_128_parameters_is_refused."""
import os
import subprocess

import numpy as np
import pytest

import va_oracle
from varanneal_amd import _capi, codegen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT, B = 0.025, 2

# (family's eval kernel, D, tile_rows, N, disc, LDS bytes)
CASES = [
    (1, 516, 4, 13, "euler", 75232),
    (1, 516, 4, 13, "trapezoid", 75232),
    (1, 412, 3, 13, "SimpsonHermite", 70144),
    (1, 516, 4, 13, "forwardmap", 75232),
    (3, 66, 50, 121, "trapezoid", 68704),
    (4, 6, 244, 600, "trapezoid", 72192),
]
IDS = ["k%d-D%d-%s" % (c[0], c[1], c[4]) for c in CASES]


def _l96_user(t, x, p):
    """Lorenz-96 as a user would write it (not the registry's callable)"""
    return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - x + p[0]


def _lidx(D):
    L = max(1, D // 5)
    return [l * D // L for l in range(L)]                  # as lds_check.cpp spreads them


def test_table_is_what_the_size_functions_give(tmp_path):
    """every row: the planner picks the family, and the family's size function gives the bytes (> 64 KiB), for the built-in
    and for a generated model alike; k_eval5 stays under 64 KiB at the shape where it is largest"""
    exe = str(tmp_path / "lds_check")
    subprocess.check_call([codegen.HIPCC, "-x", "hip", "--cuda-host-only", "-O1", "-std=c++17", "-Wno-unused-function",
                           "-I", os.path.join(ROOT, "varanneal_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpu_emul", "lds_check.cpp")])
    lines, want = [], []
    for rhs in (0, 1000):
        for ek, D, tr, N, disc, lds in CASES:
            lines.append("%d %d %d %d 0 0 1 %d %d %d 0 0 %d 0 2 2 2 1 1 2 1 1 10"
                         % (D, N, B, _capi.DISC[disc], len(_lidx(D)), tr, ek, rhs))
            want.append((ek, lds))
    lines.append("200 201 1 0 1 0 1 200 0 5 0 0 0 0 2 2 2 1 1 2 1 1 10")      # (every column observed: the largest)
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    for (ek, lds), o in zip(want, out):
        emode = int(o.split()[0])
        l0, l1 = (int(v) for v in o.split("|")[1].split()[1:])
        assert (emode, l0, l1) == (ek, lds, lds) and lds > 64 * 1024, o
    e5 = out[len(want)]
    assert int(e5.split()[0]) == 5 and max(int(v) for v in e5.split("|")[1].split()[1:]) == 62464


_modules = {}


def _module(ek, D, tr, N, disc):
    """the generated module of the cell: its flat kernel, or the column-run instantiation the cell's plan calls for"""
    key = (D,) if ek == 1 else (ek, D, tr, N, disc)
    if key not in _modules:
        cv = None if ek == 1 else (lambda ne, gh: _capi.eval_plan(B, D, N, disc, ne, gh, tile_rows=tr, eval_kernel=ek))
        m = codegen.module_for(_l96_user, D, 1, col_variant=cv)
        assert ek == 1 or m["col_variant"][0] == ek, m["col_variant"]
        _modules[key] = _capi.load_rhs_module(m["so"])
    return _modules[key]


_refs = {}


def _reference(case):
    """the cell's problem data and the oracle's answers, computed once and shared by the two right-hand sides"""
    if case not in _refs:
        ek, D, tr, N, disc, lds = case
        rng = np.random.RandomState(D + N)
        Lidx = _lidx(D)
        Y = rng.randn(N, len(Lidx))
        P = np.array([[8.17], [7.9]])
        XP = np.concatenate([2.0 * rng.randn(B, N * D), P], axis=1)
        opts = {"maxiter": 3, "gtol": 1e-12, "ftol": 1e-14}
        ref = []
        for b in range(B):
            ob = va_oracle.Problem(D, N, Y, Lidx, DT, 4.0, 0.05, P[b], [0], disc=disc)
            Ao, _, _, go = ob.action_grad(XP[b], 3.0)
            _, _, st, nit, nfev = ob.minimize_lbfgs(XP[b], 3.0, opts)
            ref.append((Ao, go, (nit, nfev, st)))
        _refs[case] = (Lidx, Y, P, XP, opts, ref)
    return _refs[case]


@pytest.mark.gpu
@pytest.mark.parametrize("generated", [False, True], ids=["builtin", "module"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_kernel_above_64k_is_prepared_and_launched(case, generated):
    ek, D, tr, N, disc, lds = case
    Lidx, Y, P, XP, opts, ref = _reference(case)
    rhs = _module(ek, D, tr, N, disc) if generated else "lorenz96"
    with _capi.Problem(B, D, N, Y, Lidx, DT, 4.0, 0.05, P, [0], disc=disc, rhs=rhs, tile_rows=tr, eval_kernel=ek) as pb:
        assert pb.info()["eval_kernel"] == ek, pb.info()
        A, me, fe, g = pb.action_grad(XP, 3.0)
        pb.tune(persist=0)                   # (the three-launch cycle: line-search launches of the evaluation kernel, not k_seed)
        r = pb.minimize_lbfgs(XP, 3.0, opts)
    for b in range(B):
        Ao, go, counts = ref[b]
        ea, eg = abs(A[b] - Ao) / abs(Ao), np.abs(g[b] - go).max() / np.abs(go).max()
        print("%s seed %d: |dA|/|A| %.2e  |dg|/|g| %.2e  (nit, nfev, status) %s vs %s"
              % (IDS[CASES.index(case)], b, ea, eg, (r["nit"][b], r["nfev"][b], r["status"][b]), counts))
        assert ea <= 1e-12 and eg <= 1e-10
        assert (r["nit"][b], r["nfev"][b], r["status"][b]) == counts
