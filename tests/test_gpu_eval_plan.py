"""GPU: a handle's evaluation kernel and tile are the ones the chooser's CPU check records (csrc/va_eval_geo.h through
tests/cpu_emul/plan_check.cpp, tests/golden/eval_plans.txt): va_problem_create copies the plan the header makes.  Built-in
Lorenz-96 problems of a few seeds; each case is a create and a destroy."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DISC = {0: "euler", 1: "trapezoid", 2: "SimpsonHermite", 3: "forwardmap"}
L96 = (0, 0, 2, 2, 2, 1, 1, 2)       # rhs, lin, then the built-in's forms: ne, ghost, reaches

# (D, N, B, disc, merr_nskip, L, tile_rows, eval_kernel asked for) -> the kernel the golden row names
CASES = [
    ((8, 161, 8, 1, 1, 4, 0, 4), 4), ((8, 161, 8, 1, 1, 4, 0, 3), 3), ((8, 161, 8, 1, 1, 4, 0, 1), 1),
    ((20, 161, 8, 1, 1, 10, 0, 0), 4), ((20, 161, 8, 1, 1, 10, 0, 3), 3),
    ((200, 161, 8, 1, 1, 100, 0, 0), 5), ((200, 161, 8, 1, 1, 100, 0, 3), 3), ((200, 161, 8, 1, 1, 100, 0, 1), 1),
    ((101, 161, 8, 1, 1, 50, 0, 0), 3),                  # odd D > 64: neither k_eval4 nor k_eval5
    ((20, 161, 8, 1, 2, 10, 200, 0), 4),                 # a run length asked for: runs of 12 rows, data every 2nd row
    ((200, 161, 8, 2, 1, 100, 40, 3), 3),                # Simpson-Hermite, a tile asked for
    ((20, 161, 64, 2, 1, 10, 0, 0), 4),                  # Simpson-Hermite
]


@pytest.fixture(scope="module")
def recorded():
    import importlib.util
    spec = importlib.util.spec_from_file_location("dump_eval_plans", os.path.join(ROOT, "tools", "dump_eval_plans.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    with open(os.path.join(ROOT, "tests", "golden", "eval_plans.txt")) as fh:
        return {row: [int(v) for v in line.split("|")[0].split()] for row, line in zip(tool.grid(), fh)}


@pytest.mark.parametrize("case,kernel", CASES)
def test_handle_runs_the_recorded_plan(recorded, case, kernel):
    from varanneal_amd import _capi
    D, N, B, disc, nskip, L, tile_rows, ek = case
    emode, RY, NT, maxr, T, ntiles, ghost = recorded[(D, N, B, disc, 0, 0, nskip, L, tile_rows, ek, 0, 0) + L96]
    assert emode == kernel
    rng = np.random.default_rng(D + N)
    Y = rng.standard_normal(((N - 1) // nskip + 1, L))
    Lidx = [l * D // L for l in range(L)]                # as plan_check.cpp spreads them
    with _capi.Problem(B, D, N, Y, Lidx, 0.025, 4.0, 4e-6, np.full((B, 1), 8.17), [0], disc=DISC[disc], merr_nskip=nskip,
                       tile_rows=tile_rows, eval_kernel=ek) as pb:
        info = pb.info()
    assert (info["eval_kernel"], info["run_rows"], info["tile_rows"], info["ntiles"]) == (emode, maxr, T, ntiles)
