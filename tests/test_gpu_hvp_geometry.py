"""GPU: va_hess_vec (csrc/va_hvp.h k_hvp, k_hvp_finish) at the shapes it really runs, held to the derivative bound
_hess_ref.REL = 1e-10 against the reference of tests/_hess_torch_ref.py (the oracle's action differentiated twice by
autograd, itself within 2.6e-15 of the SymPy Hessians where SymPy reaches): tiles of several hundred elements, so that the
strided loops of tile_fdot and tile_hv take up to four steps per thread; several tiles, partial last tiles, Simpson-Hermite
odd tiles that start on odd rows; widths that do not divide a workgroup, exceed it, or force the tile down to 2 or 3 rows;
the weight images of k_eval4 and k_eval5 handles (unsorted observed columns of odd count, RM and RF arrays, merr_nskip = 2);
generated models whose parameter rows run over several tiles, every point with fixed parameters of its own.  The same
cases pass the host run of the phases in tests/test_hess_torch_ref_cpu.py.

Per point: two random directions, the unit vectors of the last owned row of tile 0 and of the first row of tile 1 (column
D - 1) for every tiling of the case, and the unit vector of each estimated parameter -- a seam or weight error is O(1) in
one Hessian column."""
import numpy as np
import pytest

import _hess_ref as hr
import _hess_torch_ref as tr
from varanneal_amd import _capi, codegen

pytestmark = pytest.mark.gpu


def _check(c, rhs="lorenz96"):
    """every tiling of the case, full and Gauss-Newton; returns the largest rel_err"""
    N, D = c["N"], c["D"]
    kw = {} if c["stim"] is None else dict(stim=c["stim"])
    worst = 0.0
    with _capi.Problem(tr.NPTS, D, N, c["Y"], c["Lidx"], c["dt"], c["RM"], c["RF0"], np.array(c["P"]), c["Pidx"], disc=c["disc"],
                       rhs=rhs, merr_nskip=c["nskip"], **kw) as pb:
        if c["kernel"] is not None:
            assert pb.info()["eval_kernel"] == c["kernel"], pb.info()
        before = pb.action_grad(c["X"], c["rf_scale"])
        for gn, want in ((False, c["want"]), (True, c["want_gn"])):
            for tile_rows in c["plan"]:
                got = pb.hess_vec(c["X"], c["V"], c["rf_scale"], P=c["P"], gauss_newton=gn, tile_rows=tile_rows)
                err = hr.rel_err(got, want)
                print("%s gn=%d tile_rows=%d  max |Hv - H_ref v| / max |H_ref v| = %.2e" % (c["name"], gn, tile_rows, err))
                assert err <= hr.REL
                worst = max(worst, err)
                again = pb.hess_vec(c["X"], c["V"], c["rf_scale"], P=c["P"], gauss_newton=gn, tile_rows=tile_rows)
                assert np.array_equal(again[:, :, N * D:], got[:, :, N * D:])
                if c["forced_T"] and tile_rows == 0:
                    # the plan is not reported: the library's choice is the same launch as asking for T rows (the same
                    # bits, parameter rows summed over the same tiles), and one row more does not fit
                    T = c["forced_T"]
                    assert c["plan"][0] == (T, -(-N // T))
                    assert np.array_equal(pb.hess_vec(c["X"], c["V"], c["rf_scale"], P=c["P"], gauss_newton=gn, tile_rows=T), got)
                    with pytest.raises(_capi.VaError, match="do not fit"):
                        pb.hess_vec(c["X"], c["V"], c["rf_scale"], P=c["P"], gauss_newton=gn, tile_rows=T + 1)
        for a, b in zip(before, pb.action_grad(c["X"], c["rf_scale"])):
            assert np.array_equal(a, b)
    return worst


@pytest.mark.parametrize("disc", ["trapezoid", "SimpsonHermite", "euler", "forwardmap"])
def test_d20_on_a_column_kernel_handle(disc):
    """k_eval4 handle, D = 20, N = 41 / 40, scalar weights, 3 points x 8 directions: one tile of 820 / 800 elements (four
    strided steps per thread), tiles of 16 rows (three, the last partial) and of 13 rows (260 elements; Simpson-Hermite: odd
    tiles that start on odd rows).  Measured on an MI355X: 1.3e-16 .. 2.4e-16."""
    _check(tr.geometry_case("d20-%s" % disc))


@pytest.mark.parametrize("disc", ["trapezoid", "SimpsonHermite"])
def test_d20_weight_arrays_on_a_column_kernel_handle(disc):
    """k_eval4 handle with weight arrays: merr_nskip = 2, RM a random (21, 3) array, Lidx = [12, 0, 7] (sorted at create,
    the RM columns permuted with it), RF a random (40, 20) array; one tile and tiles of 13 rows.
    Measured on an MI355X: 1.8e-16 .. 4.0e-16."""
    _check(tr.geometry_case("d20-weights-%s" % disc))


@pytest.mark.parametrize("weights", ["weights", "rfarray"])
@pytest.mark.parametrize("disc", ["trapezoid", "SimpsonHermite"])
def test_d200_on_a_streaming_kernel_handle(disc, weights):
    """k_eval5 handle, D = 200, N = 21: observation rows padded to the handle's pitch (odd L), scalars spread into arrays.
    weights: the set above (RM (11, 3), RF (20, 200), nskip 2); rfarray: scalar RM, RF array.  The library's tiles (15 / 14
    rows, two tiles) and tiles of 5 rows.  Measured on an MI355X: 1.7e-16 .. 2.4e-16."""
    _check(tr.geometry_case("d200-%s-%s" % (weights, disc)))


@pytest.mark.parametrize("D,disc", [(D, d) for D in (67, 300, 600) for d in ("trapezoid", "SimpsonHermite")])
def test_widths(D, disc):
    """D = 67, N = 9 (odd, no divisor of 256: the carried (row, column) pair wraps at a different place every step); D = 300,
    N = 7 (wider than a workgroup: no whole row per step); D = 600, N = 5 (160 KiB of LDS hold 3 + 2 rows of six images,
    Simpson-Hermite 2 + 3: two and three tiles, and asking for one row more is refused).
    Measured on an MI355X: 1.2e-16 .. 4.6e-16."""
    _check(tr.geometry_case("d%d-%s" % (D, disc)))


def test_generated_stencil_parameter_rows_over_several_tiles():
    """hr.two_param_stencil, D = 20, N = 21, Simpson-Hermite, both parameters estimated: one tile of 420 elements and five
    tiles of 5 rows (pgrad2 and the (x, p) cross terms in every tile, summed by k_hvp_finish).
    Measured on an MI355X: 2.7e-16."""
    c = tr.geometry_case("stencil-d20")
    m = codegen.module_for(hr.two_param_stencil, c["D"], 2)
    _check(c, rhs=_capi.load_rhs_module(m["so"]))


def test_nakl_points_with_their_own_fixed_parameters():
    """NaKL, D = 4, N = 161, trapezoid, a stimulus, 3 of 18 parameters estimated; the 15 fixed ones differ from point to
    point; one tile of 644 elements and four tiles of 50 rows.
    Measured on an MI355X: 4.2e-15 (full), 1.5e-15 (Gauss-Newton)."""
    from models.nakl import nakl
    c = tr.geometry_case("nakl-n161")
    m = codegen.module_for(nakl, c["D"], 18, nstim=1)
    _check(c, rhs=_capi.load_rhs_module(m["so"]))
