"""GPU: the persistent per-seed ladder kernel (k_seed, csrc/va_persist.h) at every slice geometry its planner accepts,
and its three-launch twin on the same handle, against the oracle step for step: identical (nit, nfev, status), action
and iterates to 1e-6, A = me + fe to 1e-12 -- the tolerances tests/test_gpu_persist.py holds this kernel to.  The
cases are tests/_persist_cases.py; tests/test_persist_cases.py confirms on the CPU that the planner accepts each
slicing with the (G, T) asserted here, that the oracle's decisions do not depend on rounding noise there, and that each
case reaches its branch.  What each group is there for in va_persist.h:

  width      wave*64 >= RD (D = 4, 5, 7 at G = 1: most of the 16 waves hold no element of the staged rows and publish
             zeros); G = 1 (no exchange: totals straight from `part`); at D = 36, 64 the planner's own G > 1
  forced     the halo polls at G > 1 -- with HL = 2 (Simpson-Hermite: two rows from the left neighbour, one row past
             the slice from the right) and HL = 1; T = 2 (the left halo and both edge rows are the neighbour's whole
             slice); G = 9 .. 20 (pz_col_sum past one chunk of 8 rows, past two); a last slice of two / three rows
             (`rows` < T, lr = HL + rows - 2 of the published edge rows); a full last slice; G = 2; seeds b > 0 (D = 5)
  history    col > PZ_MREG (pz_coeffs' LDS path: m = 11, 17, 32; coeffs_wave's on the three-launch cycle), the register
             path at its limit (m = 10), wrapping histories (m = 3, 10, 11, 17: joff = 1, `order` rotates), m = 32 =
             MAX_M (pz_sum_cols, the LDS plan, njobs = 67 speculation jobs over 15 waves)
  sparse     ndn = 0 (nskip > T: slices without a data row), nd_lo / nd_hi at slice edges off the data grid, the
             biased base pointers of ylds / rmlds / rflds (r_lo, r_hi under HL = 2)
  obs        the column map (unsorted Lidx, L = 1, L = D), NPe = 0 (no parameter block: nvh = RD), several seeds
  full       rf0_full (tile_qfull, the qs / fs swap) and rm_full, sliced and not
  generated  a generated module's k_seed with RHS::NP = 3 and NPe = 2 (pidx_l, the fixed parameter from pfix)
"""
import numpy as np
import pytest

import _persist_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from varanneal_amd import _capi
    _capi.lib()
    return _capi


@pytest.fixture(scope="module")
def damped3_rhs(capi):
    from varanneal_amd import codegen
    return capi.load_rhs_module(codegen.module_for(pc.damped3, 6, 3)["so"])


def device_problem(capi, c, rhs=None, seeds=None):
    p = pc.problem(c)
    P = p["P"] if seeds is None else p["P"][seeds]
    kw = dict(disc=c.disc, merr_nskip=c.nskip, lbfgs_m=c.lbfgs_m)
    if rhs is not None:
        kw["rhs"] = rhs
    return capi.Problem(len(P), c.D, c.N, p["Y"], p["Lidx"], p["dt"], p["RM"], p["RF0"], P, p["Pidx"], **kw)


def run_both_paths(pb, c, XP):
    """the minimisation on the persistent kernel at the case's slicing, then on the three-launch cycle of the same handle"""
    if c.persist_rows:
        pb.tune(persist_rows=c.persist_rows)
    assert pb.persistent() == (c.G, c.T)
    cyc0 = pb.counters()["cycles"]
    r = pb.minimize_lbfgs(XP, c.rf, pc.opts(c))
    assert pb.persistent() == (c.G, c.T)                    # (a launch that was abandoned turns the path off for good)
    assert pb.counters()["cycles"] > cyc0
    pb.tune(persist=0)
    assert pb.persistent() is None
    r3 = pb.minimize_lbfgs(XP, c.rf, pc.opts(c))
    return r, r3


@pytest.mark.parametrize("name", [c.name for c in pc.CASES])
def test_both_device_paths_match_the_oracle(capi, request, name):
    c = pc.BY_NAME[name]
    XP = pc.problem(c)["XP"]
    rhs = request.getfixturevalue("damped3_rhs") if c.model == "damped3" else None
    with device_problem(capi, c, rhs) as pb:
        r, r3 = run_both_paths(pb, c, XP)
    for b, (x, A, st, nit, nfev) in enumerate(pc.oracle(c)):
        for path, rr in (("k_seed", r), ("three-launch", r3)):
            tag = (name, path, b)
            dA = abs(rr["A"][b] - A) / abs(A)
            dx = np.abs(rr["x"][b] - x).max() / max(1.0, np.abs(x).max())
            dsum = abs(rr["A"][b] - (rr["me"][b] + rr["fe"][b])) / abs(A)
            print(tag, "(nit, nfev, status) =", (rr["nit"][b], rr["nfev"][b], rr["status"][b]), "oracle", (nit, nfev, st),
                  "dA = %.2e  dx = %.2e  |A - me - fe| = %.2e" % (dA, dx, dsum))
            assert (rr["nit"][b], rr["nfev"][b], rr["status"][b]) == (nit, nfev, st), tag
            assert abs(rr["A"][b] - A) <= 1e-6 * abs(A), tag
            assert np.abs(rr["x"][b] - x).max() <= 1e-6 * max(1.0, np.abs(x).max()), tag
            assert abs(rr["A"][b] - (rr["me"][b] + rr["fe"][b])) <= 1e-12 * abs(A), tag


def test_a_seed_does_not_depend_on_its_companions_at_forced_slices(capi):
    """seed 1 alone gives bit for bit what it gives in a batch of three, five workgroups each"""
    c = pc.BY_NAME["obs_B3"]
    XP = pc.problem(c)["XP"]
    with device_problem(capi, c) as pb:
        r, _ = run_both_paths(pb, c, XP)
    with device_problem(capi, c, seeds=slice(1, 2)) as pb1:
        r1, _ = run_both_paths(pb1, c, XP[1:2])
    assert np.array_equal(r1["x"][0], r["x"][1]) and r1["A"][0] == r["A"][1]
    assert (r1["me"][0], r1["fe"][0], r1["nit"][0], r1["nfev"][0]) == (r["me"][1], r["fe"][1], r["nit"][1], r["nfev"][1])
