"""CPU: the Hamiltonian Monte Carlo sampler (csrc/va_hmc.h) without a GPU -- the generator, the phases of one lane run lane by
lane on the host by a g++ build of tests/cpu_emul/hmc_check.cpp (the same headers the kernels include), against the chain
written in NumPy (tests/_hmc_ref.py, where the tolerances are derived); the launch geometry of csrc/va_hmc_geo.h and the
argument checks va_hmc makes before it touches a device; the warm-up rule of va_ode.Annealer.sample."""
import os
import subprocess

import numpy as np
import pytest

import _hmc_ref as R
from varanneal_amd import va_ode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x1234567890ABCDEF


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("hmc") / "hmc_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-I",
                           os.path.join(ROOT, "varanneal_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "cpu_emul", "hmc_check.cpp")])
    return out


def _out(exe, *args):
    run = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stderr)
    return run.stdout


def _host_words(exe, seed, chain, it, n):
    return np.array([[int(w, 16) for w in line.split()] for line in _out(exe, "words", seed, chain, it, n).splitlines()], dtype=np.uint32)


# ---------------------------------------------------------------- generator
def test_known_answer_of_philox4x32_10(exe):
    """Random123's known-answer vector for philox4x32-10 at an all-zero counter and key, by both implementations"""
    kat = np.array([0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8], dtype=np.uint32)
    ref = R.philox4x32_10((0, 0), (0, 0, 0, 0))
    host = _host_words(exe, 0, 0, 0, 1)[0]
    assert np.array_equal(ref, host)
    assert np.array_equal(ref, kat), ["%08x" % w for w in ref]
    # all-ones counter and key (the same publication)
    kat1 = np.array([0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd], dtype=np.uint32)
    assert np.array_equal(R.philox4x32_10((0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF,) * 4), kat1)


@pytest.mark.parametrize("chain,it,n", [(0, 0, 7), (2, 5, 300), (65535, 123456, 33)])
def test_host_words_equal_the_numpy_generator(exe, chain, it, n):
    assert np.array_equal(_host_words(exe, SEED, chain, it, n), R.words(SEED, chain, it, n))


def test_draws_do_not_depend_on_the_split_over_workgroups(exe):
    """n_var = 2500: three workgroups per chain, a ragged last one; every (chain, element) draws the words of its own counter
    whichever lane of whichever workgroup holds it, and chain b of three draws what chain b alone would"""
    n, B, it = 2500, 3, 4
    rows = [line.split() for line in _out(exe, "draws", SEED, it, n, B).splitlines()]
    assert len(rows) == n * B
    ref = [R.words(SEED, b, it, n) for b in range(B)]
    seen = set()
    for b, i, w0, w1 in rows:
        b, i = int(b), int(i)
        seen.add((b, i))
        assert int(w0, 16) == ref[b][i, 0] and int(w1, 16) == ref[b][i, 1]
    assert len(seen) == n * B


def test_host_uniforms_lie_in_the_half_open_interval(exe):
    """the host phases' hmc_u01 / hmc_box_muller at the extreme words: (0, 1], a finite normal, and the reference's values"""
    for w0, w1 in ((0, 0xFFFFFFFF), (0xFFFFFFFF, 0), (0, 0), (0x80000000, 0x3FFFFFFF)):
        u0, u1, z = (float(v) for v in _out(exe, "bm", w0, w1).split())
        assert u0 == R.u01(w0) and u1 == R.u01(w1) and 0.0 < u0 <= 1.0 and 0.0 < u1 <= 1.0
        assert np.isfinite(z) and abs(z - R.box_muller(w0, w1)) <= R.normal_bound(w0)
    assert float(_out(exe, "bm", 0, 0).split()[0]) == 2.0 ** -32 and float(_out(exe, "bm", 0xFFFFFFFF, 0).split()[0]) == 1.0
    assert float(_out(exe, "bm", 0xFFFFFFFF, 0).split()[2]) == 0.0                # log 1 = 0: r = 0


@pytest.mark.parametrize("chain,it,n", [(0, 0, 5), (3, 9, 1500)])
def test_host_normals_and_uniforms_equal_the_reference(exe, chain, it, n):
    """what the phases draw without explicit noise: the uniforms bit for bit, the normals within the bound _hmc_ref derives"""
    got = np.array([float(v) for v in _out(exe, "normals", SEED, chain, it, n).split()])
    ref = R.noise_row(SEED, chain, it, n)
    assert got.shape == ref.shape and np.array_equal(got[n:], ref[n:])
    err, bound = np.abs(got[:n] - ref[:n]), R.normal_bound(R.words(SEED, chain, it, n)[:n, 0])
    print("host normals: worst |host - NumPy| / bound = %.3f" % (err / bound).max())
    assert np.all(err <= bound)


# ---------------------------------------------------------------- geometry, argument checks
@pytest.mark.parametrize("n_var,B,nwg", [(1, 1, 1), (46, 3, 1), (1024, 2, 1), (1025, 2, 2), (1201, 3, 2), (3221, 64, 4)])
def test_geometry_visits_every_element_once(exe, n_var, B, nwg):
    f = _out(exe, "geo", n_var, B).split()
    assert f[0] == "OK" and [int(v) for v in f[1:]] == [nwg, nwg * B, 256, 1, 1]


def test_geometry_refusals(exe):
    assert _out(exe, "geo", 0, 1).startswith("NO")
    assert _out(exe, "geo", 1 << 40, 1 << 20).startswith("NO")


@pytest.mark.parametrize("case,word", [("n_iter", "n_iter"), ("n_leap", "n_leap"), ("thin", "thin"), ("eps_zero", "eps[1]"), ("eps_neg", "eps[0]"),
                                       ("eps_nan", "eps[0]"), ("eps_inf", "eps[1]"), ("minv_zero", "minv[3]"), ("minv_nan", "minv[5]"),
                                       ("minv_inf", "minv[0]"), ("minv_size", "minv holds"), ("jitter_one", "jitter"), ("jitter_neg", "jitter"),
                                       ("jitter_nan", "jitter"), ("keep_high", "keep_idx[1]"), ("keep_neg", "keep_idx[0]")])
def test_invalid_arguments_are_named(exe, case, word):
    rc, why = _out(exe, "args", case).split(" ", 1)
    assert rc == "1" and word in why


@pytest.mark.parametrize("case", ["good", "good_per_chain", "good_no_minv"])
def test_valid_arguments_pass(exe, case):
    assert _out(exe, "args", case).split()[0] == "0"


# ---------------------------------------------------------------- the chain on the 6-variable quadratic
H = R.tridiag_hessian()


def _host_chain(exe, tmp_path, x0, eps, n_iter, n_leap, noise=None, jitter=0.0, minv=None, thin=1, keep=(), nan_it=-1, seed=SEED):
    B, n = x0.shape
    kind = 0 if minv is None else (2 if np.ndim(minv) == 2 else 1)
    eps = np.broadcast_to(np.asarray(eps, dtype=np.float64).reshape(-1), (B,))
    nums = list(eps) + ([] if minv is None else list(np.ravel(minv)))
    tail = list(np.diag(H)) + list(np.diag(H, 1)) + list(x0.ravel()) + ([] if noise is None else list(noise.ravel()))
    f, o = tmp_path / "in.txt", tmp_path / "out.bin"
    f.write_text("%d %d %d %d %.17g %d %d %d %d %d\n" % (B, n_iter, n_leap, thin, jitter, nan_it, 0 if noise is None else 1, seed, kind, len(keep))
                 + "\n".join("%.17g" % v for v in nums) + "\n" + " ".join(str(int(k)) for k in keep) + "\n"
                 + "\n".join("%.17g" % v if np.isfinite(v) else "nan" for v in tail) + "\n")
    _out(exe, "chain", f, o)
    raw = np.fromfile(str(o))
    nt, nk = n_iter * B * n, B * (n_iter // thin) * len(keep)
    sizes = [nt, nt, B * n, B * n, B * n_iter, B * n_iter, B * n_iter, nk]
    assert raw.size == sum(sizes)
    xt, pt, mean, var, A, dH, acc, kept = np.split(raw, np.cumsum(sizes)[:-1])
    return dict(x_trace=xt.reshape(n_iter, B, n), p_trace=pt.reshape(n_iter, B, n), mean=mean.reshape(B, n), var=var.reshape(B, n),
                A=A.reshape(B, n_iter), dH=dH.reshape(B, n_iter), accepted=acc.reshape(B, n_iter).astype(np.int32),
                kept=kept.reshape(B, n_iter // thin, len(keep)))


def _noise(n_iter, B, n, seed=3):
    rs = np.random.RandomState(seed)
    z = rs.randn(n_iter, B, n + 2)
    z[:, :, n:] = rs.uniform(0.05, 1.0, (n_iter, B, 2))
    return z


@pytest.mark.parametrize("minv_kind", [0, 1, 2])
def test_host_chain_equals_the_numpy_chain(exe, tmp_path, minv_kind):
    """B = 3 chains, per-chain step sizes, jitter, thin = 2 and scattered kept columns, each shape of minv: positions,
    momenta, running statistics bit for bit; dH within the summation-order bound; every decision equal"""
    B, n, n_iter, n_leap = 3, 6, 12, 5
    rs = np.random.RandomState(11)
    x0 = rs.randn(B, n)
    minv = [None, rs.uniform(0.5, 2.0, n), rs.uniform(0.5, 2.0, (B, n))][minv_kind]
    eps, noise, keep = np.array([0.9, 0.45, 0.2]), _noise(n_iter, B, n), [5, 0, 3]
    ref = R.chain(x0, R.quadratic_action_grad(H), eps, n_iter, n_leap, noise, jitter=0.3, minv=minv, thin=2, keep_idx=keep)
    assert R.decisions_are_safe(ref)
    assert 0 < ref["accepted"].sum() < ref["accepted"].size                    # (both outcomes occur)
    got = _host_chain(exe, tmp_path, x0, eps, n_iter, n_leap, noise, jitter=0.3, minv=minv, thin=2, keep=keep)
    assert np.array_equal(got["accepted"], ref["accepted"])
    for k in ("x_trace", "p_trace", "mean", "var", "A", "kept"):
        assert np.array_equal(got[k], ref[k]), k
    err = np.abs(got["dH"] - ref["dH"])
    print("|dH host - dH numpy| / bound: at most %.3f" % (err / ref["dh_bound"]).max())
    assert np.all(err <= ref["dh_bound"])


def test_reversing_the_momentum_returns_to_the_start(exe, tmp_path):
    B, n, L, eps = 1, 6, 7, 0.3
    x0 = np.random.RandomState(5).randn(B, n)
    noise = _noise(2, B, n)
    noise[:, :, n] = 1e-300                                                     # log u = -690: both iterations are accepted
    first = _host_chain(exe, tmp_path, x0, eps, 1, L, noise[:1])
    noise[1, :, :n] = -first["p_trace"][0]                                      # (identity mass: p = z)
    both = _host_chain(exe, tmp_path, x0, eps, 2, L, noise)
    assert both["accepted"].all() and np.array_equal(both["x_trace"][0], first["x_trace"][0])
    S = max(np.abs(both["x_trace"]).max(), np.abs(both["p_trace"]).max(), np.abs(x0).max())
    bound = R.reverse_bound(L, eps, np.abs(H).sum(axis=1).max(), S)
    err = np.abs(both["x_trace"][1] - x0).max()
    print("|x back - x start| = %.3e, bound %.3e" % (err, bound))
    assert err <= bound
    assert np.abs(both["p_trace"][1] + noise[0, :, :n]).max() <= bound          # ... and the momentum to minus the first draw


def test_energy_error_is_second_order_in_the_step(exe, tmp_path):
    """the same trajectory length with eps and eps / 2: max |dH| falls by a factor between 3 and 5"""
    B, n = 4, 6
    x0 = np.random.RandomState(8).randn(B, n)
    noise = _noise(8, B, n)
    noise[:, :, n] = 1e-300
    a = _host_chain(exe, tmp_path, x0, 0.1, 8, 4, noise)
    b = _host_chain(exe, tmp_path, x0, 0.05, 8, 8, noise)
    ratio = np.abs(a["dH"]).max() / np.abs(b["dH"]).max()
    print("max|dH|(eps) / max|dH|(eps/2) = %.3f" % ratio)
    assert 3.0 <= ratio <= 5.0


def test_nan_gradient_rejects_counts_and_restores(exe, tmp_path):
    B, n, n_iter, L = 2, 6, 4, 3
    x0 = np.random.RandomState(9).randn(B, n)
    noise = _noise(n_iter, B, n)
    noise[:, :, n] = 1e-300
    calls = [0]
    f = R.quadratic_action_grad(H)

    def with_nan(X):
        A, G = f(X)
        if 1 + 2 * L <= calls[0] < 1 + 3 * L:                                  # the evaluations of iteration 2
            G[:, 2] = np.nan
        calls[0] += 1
        return A, G
    ref = R.chain(x0, with_nan, 0.2, n_iter, L, noise)
    got = _host_chain(exe, tmp_path, x0, 0.2, n_iter, L, noise, nan_it=2)
    assert list(got["accepted"][0]) == [1, 1, 0, 1] and np.array_equal(got["accepted"], ref["accepted"])
    assert np.isnan(got["dH"][:, 2]).all() and np.isfinite(np.delete(got["dH"], 2, axis=1)).all()
    assert np.array_equal(got["x_trace"][2], got["x_trace"][1]) and got["A"][0, 2] == got["A"][0, 1]      # restored
    for k in ("x_trace", "mean", "var", "A"):
        assert np.all(np.isfinite(got[k])) and np.array_equal(got[k], ref[k]), k


def _batch_check(x, exact_mean, exact_var, nb=50):
    """each sample mean and variance within 5 standard errors, the standard error from the chain's own nb batch means"""
    n = (x.shape[0] // nb) * nb
    xb = x[:n].reshape(nb, -1, x.shape[1])
    m, se_m = xb.mean(axis=1).mean(axis=0), xb.mean(axis=1).std(axis=0, ddof=1) / np.sqrt(nb)
    sq = (x[:n] - exact_mean) ** 2
    sb = sq.reshape(nb, -1, x.shape[1]).mean(axis=1)
    v, se_v = sb.mean(axis=0), sb.std(axis=0, ddof=1) / np.sqrt(nb)
    return np.abs(m - exact_mean) / se_m, np.abs(v - exact_var) / se_v


def test_stationary_distribution_of_the_quadratic(exe, tmp_path):
    """one chain of 20 000 iterations with the generator's own draws (seed fixed): exp(-1/2 x^T H x) has mean 0 and
    covariance H^-1.  The host phases (the libm of this machine) and the NumPy chain fed the NumPy generator's noise."""
    n, n_iter, L, eps, seed = 6, 20000, 5, 0.35, 2024
    x0 = np.zeros((1, n))
    var = np.diag(np.linalg.inv(H))
    w = R.philox4x32_10((seed & 0xFFFFFFFF, seed >> 32), (0, np.arange(n_iter)[:, None], np.arange(n)[None, :], 0))
    ex = R.philox4x32_10((seed & 0xFFFFFFFF, seed >> 32), (0, np.arange(n_iter), 0, 1))
    noise = np.concatenate([R.box_muller(w[..., 0], w[..., 1]), R.u01(ex[:, :2])], axis=1)[:, None, :]
    ref = R.chain(x0, R.quadratic_action_grad(H), eps, n_iter, L, noise, jitter=0.2)
    zm, zv = _batch_check(ref["x_trace"][:, 0], 0.0, var)
    print("NumPy chain: acceptance %.3f, worst mean %.2f se, worst variance %.2f se" % (ref["accepted"].mean(), zm.max(), zv.max()))
    assert zm.max() <= 5.0 and zv.max() <= 5.0
    got = _host_chain(exe, tmp_path, x0, eps, n_iter, L, None, jitter=0.2, seed=seed)
    zm, zv = _batch_check(got["x_trace"][:, 0], 0.0, var)
    print("host phases: acceptance %.3f, worst mean %.2f se, worst variance %.2f se" % (got["accepted"].mean(), zm.max(), zv.max()))
    assert zm.max() <= 5.0 and zv.max() <= 5.0
    assert 0.6 < got["accepted"].mean() < 1.0
    # Welford's running statistics are the trace's own
    assert np.allclose(got["mean"][0], got["x_trace"][:, 0].mean(axis=0), rtol=0, atol=1e-12)
    assert np.allclose(got["var"][0], got["x_trace"][:, 0].var(axis=0, ddof=1), rtol=1e-10)


# ---------------------------------------------------------------- warm-up rule
def test_warmup_rescaling_rule():
    f = va_ode.hmc_rescale_step
    eps = np.array([0.1, 0.1, 0.1, 0.1, 0.1])
    out = f(eps, np.array([0.0, 0.4, 0.8, 0.95, 1.0]))
    assert out[0] == 0.05 and out[4] == 0.2                                    # clipped to a factor 2 either way
    assert out[2] == 0.1                                                       # the target rate leaves the step alone
    assert out[1] < 0.1 < out[3] and np.all(np.diff(out) >= 0)                 # monotone in the acceptance rate
    assert np.array_equal(f(eps, np.full(5, 0.8), target=0.8), eps)
    assert np.array_equal(eps, np.full(5, 0.1))                                # pure: the input is not touched
    with pytest.raises(ValueError):
        f(eps, np.array([0.5, 0.5, 1.2, 0.5, 0.5]))
