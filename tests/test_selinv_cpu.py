"""CPU: the block-tridiagonal selected inverse (csrc/va_selinv.h) without a GPU -- the kernel's phases run thread by thread on
the host by a g++ build of tests/cpu_emul/selinv_check.cpp (the same header the kernel includes) against numpy's dense
inverse; the failure handling; the geometry of csrc/va_selinv_geo.h; k_hblocks's index map against Python's banded assembly.

The bound throughout: max |Sigma - Sigma_ref| <= kappa_2(H_ref) 2.2e-16 max |Sigma_ref| with Sigma_ref = numpy.linalg.inv(H_ref),
kappa from the reference matrix; logdet against numpy.linalg.slogdet within n kappa 2.2e-16 (tests/_selinv_ref.py)."""
import subprocess

import numpy as np
import pytest

import _hess_ref as hr
import _selinv_ref as sr

L96_CASES = ([(d, "plain") for d in ("euler", "forwardmap", "trapezoid", "SimpsonHermite")]
             + [("trapezoid", "nskip"), ("SimpsonHermite", "rfarr")])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return sr.build_exe(str(tmp_path_factory.mktemp("selinv") / "selinv_check"))


@pytest.mark.parametrize("W,K,NPe", sr.SHAPES)
def test_host_phases_match_the_dense_inverse(exe, tmp_path, W, K, NPe):
    """random positive definite arrow matrices, three per shape: every output block, logdet, status.
    Measured ratios err / bound: at most 0.60 (W = 17, kappa = 5: the bound is a few units in the last place there)."""
    Dk, Bk, Pk, Hpp, H = sr.arrow_batch(W, K, NPe)
    r = sr.host_selinv(exe, tmp_path, Dk, Bk, Pk, Hpp)
    assert list(r["status"]) == [0, 0, 0]
    for p in range(3):
        sr.check_blocks("W=%d K=%d NPe=%d pt %d" % (W, K, NPe, p), H[p], W, K, NPe, r["Skk"][p], r["Snk"][p], r["Spk"][p], r["Spp"][p],
                        r["logdet"][p])
    # NULL outputs change nothing in the others
    r2 = sr.host_selinv(exe, tmp_path, Dk, Bk, Pk, Hpp, want=(1, 0, 0, 1))
    assert np.array_equal(r2["Skk"], r["Skk"]) and np.array_equal(r2["Spp"], r["Spp"]) and np.array_equal(r2["logdet"], r["logdet"])


def test_not_positive_definite_points_end_with_a_status(exe, tmp_path):
    W, K, NPe = 5, 4, 1
    Dk, Bk, Pk, Hpp, H = (np.array(a) for a in sr.arrow_batch(W, K, NPe))
    good = sr.host_selinv(exe, tmp_path, Dk[[0, 2]], Bk[[0, 2]], Pk[[0, 2]], Hpp[[0, 2]])
    Dk[1, 1] = -Dk[1, 1]
    r = sr.host_selinv(exe, tmp_path, Dk, Bk, Pk, Hpp)
    assert list(r["status"]) == [0, 2, 0]
    for name in ("Skk", "Snk", "Spk", "Spp"):
        assert np.all(np.isnan(r[name][1])), name
        assert np.array_equal(r[name][[0, 2]], good[name]), name              # bit for bit
    assert np.isnan(r["logdet"][1]) and np.array_equal(r["logdet"][[0, 2]], good["logdet"])
    # a parameter block the path cannot carry: the Schur complement fails, status -1
    Dk, Bk, Pk, Hpp, H = (np.array(a) for a in sr.arrow_batch(W, K, NPe))
    Hpp[2] = -Hpp[2]
    r = sr.host_selinv(exe, tmp_path, Dk, Bk, Pk, Hpp)
    assert list(r["status"]) == [0, 0, -1]
    assert np.all(np.isnan(r["Skk"][2])) and np.all(np.isnan(r["Spp"][2])) and np.isnan(r["logdet"][2])
    assert np.all(np.isfinite(r["Skk"][:2]))
    # NaN in a pivot is a failure too, in the first block
    Dk[0, 0, 0, 0] = np.nan
    r = sr.host_selinv(exe, tmp_path, Dk, Bk, Pk, Hpp)
    assert list(r["status"]) == [1, 0, -1]


def test_geometry(exe):
    shapes = [(W, K, NPe) for W in (1, 2, 5, 16, 17, 20, 40, 56, 57, 63, 64) for K in (1, 81) for NPe in (0, 1, 31, 32)]
    args = [str(v) for s in shapes for v in s]
    out = subprocess.run([exe, "geo"] + args, capture_output=True, text=True)
    assert out.returncode == 0
    lines = out.stdout.strip().splitlines()
    assert len(lines) == len(shapes)
    spilled = 0
    for (W, K, NPe), ln in zip(shapes, lines):
        w = ln.split()
        assert w[0] == "OK", ln
        Wp, NPp, snk_global, lds, ws = (int(v) for v in w[4:9])
        assert Wp % 2 == 1 and Wp >= W and NPp % 2 == 1 and NPp >= NPe                  # odd pitches: 8-byte column walks without conflicts
        big, piv = max(W * Wp, NPe * NPp), (max(W, NPe) + 1) // 2 * 2
        assert lds == 8 * (2 + piv + (3 if snk_global else 4) * big + 3 * NPe * Wp + NPe * NPp)
        assert lds <= 160 * 1024
        assert snk_global == int(8 * (2 + piv + 4 * big + 3 * NPe * Wp + NPe * NPp) > 160 * 1024)
        assert ws == (2 * K - 1 + snk_global) * W * W + K * NPe * W + K * W
        spilled += snk_global
    assert spilled > 0                                                                   # (W = 64 with 32 parameters)
    out = subprocess.run([exe, "geo", "65", "2", "0", "64", "2", "33", "0", "2", "0"], capture_output=True, text=True)
    a, b, c = out.stdout.strip().splitlines()
    assert a.startswith("NO 65 2 0") and "64" in a
    assert b.startswith("NO 64 2 33") and "32" in b
    assert c.startswith("NO 0 2 0")


@pytest.mark.parametrize("disc,hb", [("trapezoid", 1), ("SimpsonHermite", 2)])
def test_block_index_map_matches_the_banded_assembly(exe, tmp_path, disc, hb):
    """coloured products of the reference Gauss-Newton Hessians: k_hblocks's map gives exactly the blocks cut from the
    banded form va_ode.Annealer._hessian_blocks assembles, padding included (N = 7, hb = 2: K = 4, one real row at the end)"""
    c = hr.l96_case(disc)
    N, D, NPe = c["N"], c["D"], 1
    V = sr.coloured_directions(N, D, hb, NPe)
    HV = np.einsum("pij,vj->pvi", c["Hgn"], V)
    got = sr.host_blocks(exe, tmp_path, HV, N, D, hb, NPe)
    K, W = -(-N // hb), hb * D
    assert got[0].shape == (3, K, W, W)
    if hb == 2:
        assert K == 4 and np.array_equal(got[0][:, 3, D:, D:], np.broadcast_to(np.eye(D), (3, D, D)))
        assert not got[0][:, 3, :D, D:].any() and not got[1][:, 2, D:, :].any() and not got[2][:, 3, :, D:].any()
    for p in range(3):
        want = sr.blocks_from_banded(*sr.banded_from_products(HV[p], N, D, hb, NPe), N=N, D=D, hb=hb)
        for g, w_ in zip(got, want):
            assert np.array_equal(g[p], w_)
        # and the banded form holds the matrix it came from: the blocks are the reference Hessian's
        Hd = sr.dense_from_blocks(*[g[p] for g in got])
        ND = N * D
        keep = np.r_[np.arange(ND), K * W + np.arange(NPe)]
        assert np.array_equal(np.triu(Hd[np.ix_(keep, keep)]), np.triu(c["Hgn"][p]))      # (upper triangle, mirrored)


@pytest.mark.parametrize("disc,variant", L96_CASES)
def test_l96_gauss_newton_matrices_through_the_host_phases(exe, tmp_path, disc, variant):
    """coloured products -> blocks -> factor -> selected inverse -> time rows, against inv(Hgn) of the unpadded matrix"""
    c = hr.l96_case(disc, variant)
    N, D, NPe = c["N"], c["D"], 1
    hb = 2 if disc == "SimpsonHermite" else 1
    HV = np.einsum("pij,vj->pvi", c["Hgn"], sr.coloured_directions(N, D, hb, NPe))
    r = sr.host_laplace(exe, tmp_path, HV, N, D, hb, NPe)
    assert list(r["status"]) == [0, 0, 0]
    for p in range(3):
        sr.check_time_rows("%s %s pt %d" % (disc, variant, p), c["Hgn"][p], N, D, NPe, r["var_x"][p], r["cov_xx"][p], r["cov_px"][p],
                           r["cov_pp"][p], r["logdet"][p])
