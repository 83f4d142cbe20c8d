"""CPU: the case table of the persistent ladder kernel's GPU tests (tests/_persist_cases.py, run on the device by
tests/test_gpu_persist_geometry.py).  For every case: the planner (csrc/va_persist_geo.h, through the persist_check
build of tests/test_persist_geometry.py) accepts the slicing and gives the geometry the case names; the reference
minimiser alone returns the same (nit, nfev, status) from the start point and from three copies of it perturbed by a
relative 1e-13 -- the device adds its partial sums in another order than the oracle, and a step-for-step comparison
means something only where such noise cannot change a line-search decision; and the case reaches the branch of
csrc/va_persist.h it is there for."""
import numpy as np
import pytest

import _persist_cases as pc
from test_persist_geometry import exe, geo  # noqa: F401  (exe: the fixture that builds persist_check)

NAMES = [c.name for c in pc.CASES]


def test_every_group_has_cases():
    count = {g: sum(c.group == g for c in pc.CASES) for g in pc.GROUPS}
    print("cases per group:", count, "total", len(pc.CASES))
    assert all(n > 0 for n in count.values()) and sum(count.values()) == len(pc.CASES)
    for br in pc.BRANCHES:
        names = [c.name for c in pc.CASES if br in c.reach]
        print("%-16s %d cases, e.g. %s" % (br, len(names), names[:3]))
        assert names, br


@pytest.mark.parametrize("name", NAMES)
def test_planner_accepts_the_slicing(exe, name):
    c = pc.BY_NAME[name]
    L = len(pc.problem(c)["Lidx"])
    g = geo(exe, c.N, c.D, L=L, NP=pc.n_params(c), NPest=len(c.Pidx), m=c.lbfgs_m, disc=c.disc, maxG=256 // c.B, wantT=c.persist_rows)
    assert g is not None, "the planner refuses the slicing"
    assert g[:2] == (c.G, c.T)
    assert c.persist_rows in (0, c.T)
    assert c.B * c.G <= 64                        # no test asks for more than 64 co-resident workgroups
    assert c.N - (c.G - 1) * c.T >= 2


@pytest.mark.parametrize("name", NAMES)
def test_oracle_is_stable_and_the_case_reaches_its_branch(name):
    c = pc.BY_NAME[name]
    p = pc.problem(c)
    ref = pc.oracle(c)
    rng = np.random.RandomState(4242)
    for b in range(c.B):
        x, A, st, nit, nfev = ref[b]
        print(name, "seed", b, "(nit, nfev, status) =", (nit, nfev, st), "A = %.6e" % A, "(G, T, m) =", (c.G, c.T, c.lbfgs_m))
        # converged, or stopped by maxiter as in tests/test_gpu_persist.py (the abnormal and maxfun exits are not this table's subject)
        assert (st == 0 or (st == 1 and nit == c.maxiter)) and np.isfinite(A)
        for k in range(3):
            x0 = p["XP"][b] * (1.0 + 1e-13 * rng.randn(p["XP"].shape[1]))
            xk, Ak, stk, nitk, nfevk = pc.oracle_minimize(c, b, x0)
            assert (nitk, nfevk, stk) == (nit, nfev, st), (b, k)
        if c.group == "history":                                    # the history fills and wraps / the solve passes 20 columns
            assert nit >= (c.lbfgs_m + 5 if c.lbfgs_m <= 17 else 20)
        if pc.COL_GT_MREG in c.reach:
            assert c.lbfgs_m > pc.PZ_MREG and nit > pc.PZ_MREG + 1      # more than PZ_MREG pairs were in the history
    if pc.HALO_HL2 in c.reach:
        assert c.disc == "SimpsonHermite" and c.G > 1
    if pc.NDN0 in c.reach:
        assert c.nskip > c.T and any(pc.data_rows(c.N, c.T, c.nskip, w) == 0 for w in range(c.G))
        assert sum(pc.data_rows(c.N, c.T, c.nskip, w) for w in range(c.G)) == p["Y"].shape[0]
    if pc.RF0_FULL in c.reach:
        assert p["RF0"].shape == (c.N - 1, c.D, c.D) and p["RM"].ndim == 3
    if pc.NPE0 in c.reach:
        assert p["XP"].shape[1] == c.N * c.D
    if pc.IDLE_WAVES in c.reach:
        assert (pc.PZ_WAVES - 1) * 64 >= (c.T + (2 if c.disc == "SimpsonHermite" else 1) + 1) * c.D
