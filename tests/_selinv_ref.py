"""Helpers of the selected-inverse tests (TEST INFRASTRUCTURE): random block-tridiagonal arrow matrices, the dense reference
and its error bound, the coloured products a Hessian gives, Python's own cut of the blocks, and the runner of
tests/cpu_emul/selinv_check.cpp (the phases of csrc/va_selinv.h thread by thread on the host).  Shared by
tests/test_selinv_cpu.py and tests/test_gpu_selinv.py; nothing here is modified by a test."""
import functools
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.2e-16
SHAPES = [(1, 1, 0), (1, 3, 1), (5, 4, 1), (16, 3, 2), (17, 2, 0), (40, 3, 3), (64, 2, 32)]      # (W, K, NPe)


def build_exe(path):
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I",
                           os.path.join(ROOT, "varanneal_amd", "csrc"), "-o", path,
                           os.path.join(ROOT, "tests", "cpu_emul", "selinv_check.cpp")])
    return path


# ------------------------------------------------------------------------------------------------ matrices
def dense_from_blocks(Dk, Bk, Pk, Hpp):
    """one point's blocks -> the (K W + NPe)^2 matrix"""
    K, W = Dk.shape[0], Dk.shape[1]
    NPe = Hpp.shape[0]
    n = K * W
    H = np.zeros((n + NPe, n + NPe))
    for k in range(K):
        H[k * W:(k + 1) * W, k * W:(k + 1) * W] = Dk[k]
        H[n:, k * W:(k + 1) * W] = Pk[k]
        H[k * W:(k + 1) * W, n:] = Pk[k].T
        if k < K - 1:
            H[(k + 1) * W:(k + 2) * W, k * W:(k + 1) * W] = Bk[k]
            H[k * W:(k + 1) * W, (k + 1) * W:(k + 2) * W] = Bk[k].T
    H[n:, n:] = Hpp
    return H


@functools.lru_cache(maxsize=None)
def random_arrow(W, K, NPe, seed=0):
    """D_k = G G^T + W I, B_k and P_k of unit scale times 0.3, H_pp = G G^T + (NPe + K) I; the diagonal shift is raised
    until the matrix is positive definite.  Returns (Dk, Bk, Pk, Hpp, H)."""
    rng = np.random.RandomState(1000 * W + 10 * K + NPe + seed)
    G = rng.randn(K, W, W)
    GG = np.einsum("kij,klj->kil", G, G)
    Bk = 0.3 * rng.randn(max(K - 1, 0), W, W)
    Pk = 0.3 * rng.randn(K, NPe, W)
    Gp = rng.randn(NPe, NPe)
    shift = 0.0
    while True:
        Dk = GG + (W + shift) * np.eye(W)
        Hpp = np.dot(Gp, Gp.T) + (NPe + K + shift) * np.eye(NPe)
        H = dense_from_blocks(Dk, Bk, Pk, Hpp)
        if np.linalg.eigvalsh(H).min() > 0:
            break
        shift = 2.0 * shift + 1.0
    for a in (Dk, Bk, Pk, Hpp, H):
        a.setflags(write=False)
    return Dk, Bk, Pk, Hpp, H


def arrow_batch(W, K, NPe, npts=3):
    """npts different matrices of one shape, stacked"""
    pts = [random_arrow(W, K, NPe, seed=100 * p) for p in range(npts)]
    return tuple(np.array([pt[i] for pt in pts]) for i in range(5))


# ------------------------------------------------------------------------------------------------ the reference and the bound
def reference(H):
    """(Sigma_ref, kappa_2, log det) of the reference matrix alone"""
    Sig = np.linalg.inv(H)
    w = np.linalg.eigvalsh(H)
    sign, ld = np.linalg.slogdet(H)
    assert sign > 0 and w[0] > 0
    return Sig, w[-1] / w[0], ld


def check_blocks(label, H, W, K, NPe, Skk=None, Snk=None, Spk=None, Spp=None, logdet=None):
    """every given output block of one point against inv(H): max |S - S_ref| <= kappa 2.2e-16 max |S_ref|; logdet against
    slogdet: |d| <= n kappa 2.2e-16.  Prints the measured ratios."""
    Sig, kappa, ld = reference(H)
    n = K * W
    bound = kappa * EPS * np.abs(Sig).max()
    err = 0.0
    for k in range(K):
        lo, hi = k * W, (k + 1) * W
        if Skk is not None:
            err = max(err, np.abs(Skk[k] - Sig[lo:hi, lo:hi]).max())
        if Spk is not None and NPe:
            err = max(err, np.abs(Spk[k] - Sig[n:, lo:hi]).max())
        if Snk is not None and k < K - 1:
            err = max(err, np.abs(Snk[k] - Sig[hi:hi + W, lo:hi]).max())
    if Spp is not None and NPe:
        err = max(err, np.abs(Spp - Sig[n:, n:]).max())
    msg = "%s: kappa %.2e  max|S - S_ref| %.2e  bound %.2e  ratio %.3f" % (label, kappa, err, bound, err / bound)
    if logdet is not None:
        dl, bl = abs(logdet - ld), H.shape[0] * kappa * EPS
        msg += "  |dlogdet| %.2e  bound %.2e  ratio %.3f" % (dl, bl, dl / bl)
    print(msg)
    assert np.isfinite(err) and err <= bound, msg
    if logdet is not None:
        assert dl <= bl, msg


def check_time_rows(label, H, N, D, NPe, var_x, cov_xx=None, cov_px=None, cov_pp=None, logdet=None):
    """results unpacked to time rows (one point) against inv(H) of the UNPADDED Hessian, the same bound"""
    Sig, kappa, ld = reference(H)
    ND = N * D
    bound = kappa * EPS * np.abs(Sig).max()
    err = np.abs(var_x.reshape(ND) - np.diag(Sig)[:ND]).max()
    if cov_xx is not None:
        for n in range(N):
            err = max(err, np.abs(cov_xx.reshape(N, D, D)[n] - Sig[n * D:(n + 1) * D, n * D:(n + 1) * D]).max())
    if cov_px is not None and NPe:
        err = max(err, np.abs(cov_px.reshape(NPe, ND) - Sig[ND:, :ND]).max())
    if cov_pp is not None and NPe:
        err = max(err, np.abs(cov_pp.reshape(NPe, NPe) - Sig[ND:, ND:]).max())
    msg = "%s: kappa %.2e  max|S - S_ref| %.2e  bound %.2e  ratio %.3f" % (label, kappa, err, bound, err / bound)
    if logdet is not None:
        dl, bl = abs(logdet - ld), H.shape[0] * kappa * EPS
        msg += "  |dlogdet| %.2e  bound %.2e  ratio %.3f" % (dl, bl, dl / bl)
    print(msg)
    assert np.isfinite(err) and err <= bound, msg
    if logdet is not None:
        assert dl <= bl, msg


# ------------------------------------------------------------------------------------------------ colouring, Python's cut
def coloured_directions(N, D, hb, NPe):
    """the directions of va_ode.Annealer._hessian_blocks"""
    nc, ND = 2 * hb + 1, N * D
    V = np.zeros((nc * D + NPe, ND + NPe))
    rows = np.arange(N)
    for c in range(nc * D):
        V[c, (rows[rows % nc == c // D]) * D + c % D] = 1.0
    V[nc * D + np.arange(NPe), ND + np.arange(NPe)] = 1.0
    return V


def banded_from_products(HV, N, D, hb, NPe):
    """(ab, H_xp, H_pp) exactly as va_ode.Annealer._hessian_blocks fills them from the coloured products"""
    nc, ND = 2 * hb + 1, N * D
    u = (hb + 1) * D - 1
    ab = np.zeros((u + 1, ND))
    for n in range(N):
        for j in range(D):
            col = HV[(n % nc) * D + j]
            lo = max(0, n - hb) * D
            i = np.arange(lo, n * D + j + 1)
            ab[u + i - (n * D + j), n * D + j] = col[i]
    H_xp = HV[nc * D:, :ND].T.copy()
    H_pp = HV[nc * D:, ND:].copy()
    return ab, H_xp, 0.5 * (H_pp + H_pp.T)


def blocks_from_banded(ab, H_xp, H_pp, N, D, hb):
    """the padded blocks cut from the banded form: (Dk [K, W, W], Bk [K-1, W, W], Pk [K, NPe, W], Hpp)"""
    ND, u = N * D, ab.shape[0] - 1
    W, K = hb * D, -(-N // hb)
    NPe = H_pp.shape[0]
    n = K * W
    Hx = np.eye(n)
    Hx[:ND, :ND] = 0.0
    for k in range(u + 1):                                # superdiagonal k
        d = ab[u - k, k:]
        Hx[np.arange(ND - k), np.arange(k, ND)] = d
        Hx[np.arange(k, ND), np.arange(ND - k)] = d
    Px = np.zeros((NPe, n))
    Px[:, :ND] = H_xp.T
    Dk = np.array([Hx[k * W:(k + 1) * W, k * W:(k + 1) * W] for k in range(K)])
    Bk = np.array([Hx[(k + 1) * W:(k + 2) * W, k * W:(k + 1) * W] for k in range(K - 1)]).reshape(K - 1, W, W)
    Pk = np.array([Px[:, k * W:(k + 1) * W] for k in range(K)]).reshape(K, NPe, W)
    return Dk, Bk, Pk, H_pp


# ------------------------------------------------------------------------------------------------ the host run
def _nums(*arrays):
    return "\n".join(" ".join(repr(float(v)) for v in np.asarray(a, dtype=float).ravel()) for a in arrays if np.size(a)) + "\n"


def _run(exe, mode, tmpdir, txt):
    f = os.path.join(str(tmpdir), "selinv_%s.txt" % mode)
    with open(f, "w") as fh:
        fh.write(txt)
    out = subprocess.run([exe, mode, f], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr)
    return np.array([float(v) for v in out.stdout.split()])


def host_selinv(exe, tmpdir, Dk, Bk, Pk, Hpp, want=(1, 1, 1, 1)):
    """stacked blocks [npts, ...] through selinv_host; dict of status, logdet and the requested outputs"""
    npts, K, W = Dk.shape[:3]
    NPe = Hpp.shape[-1]
    w = _run(exe, "run", tmpdir, "%d %d %d %d %d %d %d %d\n" % ((npts, K, W, NPe) + tuple(want)) + _nums(Dk, Bk, Pk, Hpp))
    r = dict(status=w[:npts].astype(int), logdet=w[npts:2 * npts])
    o = 2 * npts
    for name, on, shape in (("Skk", want[0], (npts, K, W, W)), ("Snk", want[1], (npts, K - 1, W, W)),
                            ("Spk", want[2], (npts, K, NPe, W)), ("Spp", want[3], (npts, NPe, NPe))):
        if on:
            cnt = int(np.prod(shape))
            r[name] = w[o:o + cnt].reshape(shape)
            o += cnt
    assert o == w.size
    return r


def host_blocks(exe, tmpdir, HV, N, D, hb, NPe):
    """coloured products [npts, nvec, n_var] through hblocks_host: (Dk, Bk, Pk, Hpp), stacked"""
    npts = HV.shape[0]
    W, K = hb * D, -(-N // hb)
    w = _run(exe, "blocks", tmpdir, "%d %d %d %d %d\n" % (N, D, hb, NPe, npts) + _nums(HV))
    sizes = [(npts, K, W, W), (npts, K - 1, W, W), (npts, K, NPe, W), (npts, NPe, NPe)]
    out, o = [], 0
    for s in sizes:
        cnt = int(np.prod(s))
        out.append(w[o:o + cnt].reshape(s))
        o += cnt
    assert o == w.size
    return tuple(out)


def host_laplace(exe, tmpdir, HV, N, D, hb, NPe):
    """coloured products -> blocks -> selinv_host -> time rows: dict of status, logdet, var_x, cov_xx, cov_px, cov_pp"""
    npts, ND = HV.shape[0], N * D
    w = _run(exe, "laplace", tmpdir, "%d %d %d %d %d\n" % (N, D, hb, NPe, npts) + _nums(HV))
    r = dict(status=w[:npts].astype(int), logdet=w[npts:2 * npts])
    o = 2 * npts
    for name, shape in (("var_x", (npts, N, D)), ("cov_xx", (npts, N, D, D)), ("cov_px", (npts, NPe, ND)), ("cov_pp", (npts, NPe, NPe))):
        cnt = int(np.prod(shape))
        r[name] = w[o:o + cnt].reshape(shape)
        o += cnt
    assert o == w.size
    return r
