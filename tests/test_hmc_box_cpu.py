"""CPU: the box sampler (csrc/va_hmc_box.h) without a GPU -- the map of one entry, the phases of one lane run lane by lane on
the host by a g++ build of tests/cpu_emul/hmc_box_check.cpp (the same headers the kernels include), against the chain
written in NumPy (tests/_hmc_box_ref.py, where the energy bound is derived); the argument checks va_hmc_box makes before it
touches a device."""
import os
import subprocess

import numpy as np
import pytest

import _hmc_box_ref as BR
import _hmc_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = np.inf
LD = np.longdouble


def _build(tmp, name):
    out = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-I",
                           os.path.join(ROOT, "varanneal_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "cpu_emul", name + ".cpp")])
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("hmc_box"), "hmc_box_check")


@pytest.fixture(scope="module")
def exe_plain(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("hmc_plain"), "hmc_check")


def _out(exe, *args):
    run = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stderr)
    return run.stdout


def _fmt(v):
    return "%.17g" % v if np.isfinite(v) else ("nan" if np.isnan(v) else ("inf" if v > 0 else "-inf"))


# ---------------------------------------------------------------- the map
BOXES, map_table = BR.BOXES, BR.map_table


def _host_table(exe, tmp_path, mode, lo, hi, v):
    f, o = tmp_path / (mode + ".txt"), tmp_path / (mode + ".bin")
    f.write_text("%d\n" % v.size + "\n".join("%s %s %s" % (_fmt(a), _fmt(b), _fmt(c)) for a, b, c in zip(lo, hi, v)) + "\n")
    _out(exe, mode, f, o)
    return np.fromfile(str(o)).reshape(-1, v.size)


def test_map_stays_inside_its_box():
    lo, hi, z = map_table()
    x, dx, dlj, lj = BR.box_map(BR.box_kinds(lo, hi), lo, hi, z)
    assert np.all(x >= lo) and np.all(x <= hi) and np.all(np.isfinite(x))
    assert np.all(np.isfinite(dx)) and np.all(np.isfinite(dlj)) and np.all(np.isfinite(lj))
    kind = BR.box_kinds(lo, hi)
    assert np.all(dx[kind != 2] > 0) and np.all(dx[kind == 2] < 0)
    assert sorted(set(kind)) == [0, 1, 2, 3]


def test_slopes_match_centred_differences_in_longdouble():
    """dx against (T(z + h) - T(z - h)) / 2h and dlj against the same quotient of lj, the quotients by the NumPy map in
    longdouble, h = 2^-16 l with l = max(1, |z|) the length scale of the map at z.  The tolerance, derived:
      truncation  h^2/6 |f'''|.  For x: f''' = dx (dlj^2 + dlj') with |dlj| <= 2/r, |dlj'| <= 4/r^2 (one-sided, r^2 = z^2 + 4
                  >= l^2), and f''' = dx (-3/q^2 + 15 z^2/q^4) (two-sided, q^2 = 1 + z^2 >= l^2): |f'''| <= 15 |dx| / l^2 in
                  every kind, so the truncation is at most (15/6) 2^-32 |dx|.  For lj: dlj'' is a sum of at most four
                  terms each below 6/l^3: |lj'''| <= 24/l^3, truncation at most 4 2^-32 / l.
      rounding    the longdouble map takes fewer than 16 operations: each of the two values is off by at most 16 u_L F, F
                  the largest magnitude in play (|lo|, |hi|, |f|); the quotient by at most 16 u_L F / h = 16 u_L 2^16 F / l,
                  u_L the unit roundoff of longdouble.
      the float64 value under test adds 16 2^-53 of itself.
    Where dx itself falls below the rounding term (two-sided bounds far out, where x has merged with its bound), the
    quotient cannot resolve it and the bound is the rounding term; that is what the formats allow."""
    lo, hi, z = map_table()
    kind = BR.box_kinds(lo, hi)
    uL = LD(np.finfo(LD).eps) / 2
    ell = np.maximum(1.0, np.abs(z)).astype(LD)
    h = ell * LD(2.0) ** -16
    zp, zm = z.astype(LD) + h, z.astype(LD) - h
    fp, fm = BR.box_map(kind, lo, hi, zp, dtype=LD), BR.box_map(kind, lo, hi, zm, dtype=LD)
    h2 = zp - zm                                                                  # (the step really taken)
    x, dx, dlj, lj = BR.box_map(kind, lo, hi, z)
    fin = lambda a: np.where(np.isfinite(a), np.abs(a), 0.0)
    F = np.maximum.reduce([fin(lo), fin(hi), np.abs(x)]).astype(LD)
    q_x = (fp[0] - fm[0]) / h2
    tol_x = LD(15.0 / 6.0) * LD(2.0) ** -32 * np.abs(dx) + 16 * uL * F / h + 16 * 2.0 ** -53 * np.abs(dx)
    err_x = np.abs(dx.astype(LD) - q_x)
    print("dx: worst error / tolerance %.3g" % float((err_x / tol_x).max()))
    assert np.all(err_x <= tol_x)
    Fl = np.maximum(np.abs(fp[3]), np.abs(fm[3]))
    q_l = (fp[3] - fm[3]) / h2
    tol_l = 4 * LD(2.0) ** -32 / ell + 16 * uL * Fl / h + 16 * 2.0 ** -53 * np.abs(dlj)
    err_l = np.abs(dlj.astype(LD) - q_l)
    print("dlj: worst error / tolerance %.3g" % float((err_l / tol_l).max()))
    assert np.all(err_l <= tol_l)
    # ... and the tolerance still sees a wrong slope wherever the slope is resolved at all: half of it is far outside
    resolved = np.abs(dx) > 1e3 * (16 * uL * F / h)
    assert resolved.sum() > z.size // 2 and np.all((np.abs(0.5 * dx.astype(LD) - q_x) > tol_x)[resolved & (kind != 0)])


def _interior():
    """interior x of every bounded box: two-sided at fractions of the width, one-sided at distances 1e-6 .. 1e6"""
    lo, hi, x = [], [], []
    for a, b in BOXES[1:]:
        if np.isfinite(a) and np.isfinite(b):
            xs = a + (b - a) * np.array([1e-6, 1e-3, 0.1, 0.25, 0.5, 0.7, 0.9, 0.999, 1 - 1e-6])
        else:
            w = 10.0 ** np.linspace(-6, 6, 13)
            xs = a + w if np.isfinite(a) else b - w
        lo += [a] * xs.size; hi += [b] * xs.size; x += list(xs)
    return np.array(lo), np.array(hi), np.array(x)


def test_inverse_then_map_returns_x(exe, tmp_path):
    """T(T^-1(x)) within 4 ulp of x, by NumPy and by the host build.  An ulp of x itself for a one-sided box that lies on one
    side of 0 (lo >= 0 or hi <= 0: every operation of w -> z -> w -> lo + w then rounds at the magnitude of x or below).
    Elsewhere the arithmetic the issue prescribes rounds at a larger magnitude than |x| can be: a one-sided box that
    straddles 0 adds w to a bound larger than x; the two-sided inverse forms u = 2 (x - lo)/(hi - lo) - 1 by a subtraction
    that rounds at 1, which is half the width in x (measured at x = lo + 1e-6 width in (0.5, 100): 25 ulp of x, 0.4 ulp
    of 100).  There the ulp is taken at the largest of |x| and the box's finite bounds.  Measured: 1.00 ulp at most in
    either sense."""
    lo, hi, x = _interior()
    kind = BR.box_kinds(lo, hi)
    fin = lambda a: np.where(np.isfinite(a), np.abs(a), 0.0)
    one_side = (kind != 3) & ((lo >= 0.0) | (hi <= 0.0))
    assert one_side.any() and (~one_side).any()
    ulp = np.where(one_side, np.spacing(np.abs(x)), np.spacing(np.maximum.reduce([np.abs(x), fin(lo), fin(hi)])))
    z = BR.box_inverse(kind, lo, hi, x)
    assert np.all(np.isfinite(z))
    back = BR.box_map(kind, lo, hi, z)[0]
    print("T(T^-1(x)) - x: at most %.2f ulp" % (np.abs(back - x) / ulp).max())
    assert np.all(np.abs(back - x) <= 4 * ulp)
    zh = _host_table(exe, tmp_path, "inv", lo, hi, x)[0]
    assert np.array_equal(zh, z)                                                 # IEEE on both sides
    assert np.array_equal(_host_table(exe, tmp_path, "map", lo, hi, zh)[0], back)


def test_host_map_equals_numpy(exe, tmp_path):
    """hmc_box_map by g++ on the whole table: x, dx, dlj bit for bit (+ - * / sqrt, no contraction); lj = log(slope) of the
    same double by two libraries of 1 ulp each: within 2 ulp"""
    lo, hi, z = map_table()
    x, dx, dlj, lj = BR.box_map(BR.box_kinds(lo, hi), lo, hi, z)
    hx, hdx, hdlj, hlj = _host_table(exe, tmp_path, "map", lo, hi, z)
    assert np.array_equal(hx, x) and np.array_equal(hdx, dx) and np.array_equal(hdlj, dlj)
    assert np.all(np.abs(hlj - lj) <= 2 * np.spacing(np.abs(lj)))


# ---------------------------------------------------------------- the reference samples the right law
def test_reference_samples_the_truncated_normal():
    """One variable, A = x^2/2 on (0, inf), (-inf, 1), (-0.5, 1.5): 4000 iterations of 5 steps, eps 0.35, jitter 0.1, the noise
    of noise_row(2024, chain 0).  Mean and standard deviation within 0.05 of scipy.stats.truncnorm's (about 5 standard
    errors of 4000 independent draws); with the log-Jacobian switched off the mean misses by more than 0.5.
    The committed reference gives |mean error|, |std error| = (0.030, 0.014), (0.004, 0.008), (0.006, 0.016) at acceptance
    0.996, 0.995, 0.987, and mean errors 0.74, 1.16, 0.82 without the Jacobian."""
    from scipy.stats import truncnorm
    n_iter = 4000
    noise = np.stack([R.noise_row(2024, 0, it, 1) for it in range(n_iter)])[:, None, :]
    ag = lambda X: (0.5 * (X[:, 0] * X[:, 0]), X.copy())
    for lo, hi in [(0.0, INF), (-INF, 1.0), (-0.5, 1.5)]:
        lo_, hi_ = np.array([lo]), np.array([hi])
        z0 = BR.box_inverse(BR.box_kinds(lo_, hi_), lo_, hi_, np.array([[0.5]]))
        m, s = truncnorm.mean(lo, hi), truncnorm.std(lo, hi)
        r = BR.chain_box(z0, ag, lo_, hi_, 0.35, n_iter, 5, noise, jitter=0.1)
        x = r["x_trace"][:, 0, 0]
        print("(%g, %g): mean off by %.4f, std by %.4f, acceptance %.3f" % (lo, hi, abs(x.mean() - m), abs(x.std() - s), r["accepted"].mean()))
        assert np.all(x > lo) and np.all(x < hi)
        assert abs(x.mean() - m) <= 0.05 and abs(x.std() - s) <= 0.05
        w = BR.chain_box(z0, ag, lo_, hi_, 0.35, n_iter, 5, noise, jitter=0.1, jacobian=False)
        print("    without the log-Jacobian: mean off by %.3f" % abs(w["x_trace"][:, 0, 0].mean() - m))
        assert abs(w["x_trace"][:, 0, 0].mean() - m) > 0.5


# ---------------------------------------------------------------- the chain on the 6-variable quadratic
H = R.tridiag_hessian()
LO6 = np.array([-3.0, -2.5, -INF, -INF, -4.0, -3.0])
HI6 = np.array([3.0, INF, 2.5, INF, 2.0, INF])


def _host_chain(exe, tmp_path, x0, lo, hi, eps, n_iter, n_leap, noise=None, jitter=0.0, minv=None, thin=1, keep=(), nan_it=-1, seed=1, box=True):
    """the chain by hmc_box_check (box=True) or by hmc_check, the unbounded sampler's program (box=False: lo, hi unused)"""
    B, n = x0.shape
    kind = 0 if minv is None else (2 if np.ndim(minv) == 2 else 1)
    eps = np.broadcast_to(np.asarray(eps, dtype=np.float64).reshape(-1), (B,))
    nums = list(eps) + ([] if minv is None else list(np.ravel(minv)))
    tail = list(np.diag(H)) + list(np.diag(H, 1)) + list(x0.ravel()) + (list(lo) + list(hi) if box else []) + ([] if noise is None else list(noise.ravel()))
    f, o = tmp_path / "in.txt", tmp_path / "out.bin"
    f.write_text("%d %d %d %d %.17g %d %d %d %d %d\n" % (B, n_iter, n_leap, thin, jitter, nan_it, 0 if noise is None else 1, seed, kind, len(keep))
                 + "\n".join("%.17g" % v for v in nums) + "\n" + " ".join(str(int(k)) for k in keep) + "\n"
                 + "\n".join(_fmt(v) for v in tail) + "\n")
    _out(exe, "chain", f, o)
    raw = np.fromfile(str(o))
    nt, nk = n_iter * B * n, B * (n_iter // thin) * len(keep)
    names = (["z_trace"] if box else []) + ["x_trace", "p_trace", "mean", "var", "A", "dH", "accepted", "kept"]
    sizes = ([nt] if box else []) + [nt, nt, B * n, B * n, B * n_iter, B * n_iter, B * n_iter, nk]
    assert raw.size == sum(sizes)
    d = dict(zip(names, np.split(raw, np.cumsum(sizes)[:-1])))
    for k in ("z_trace", "x_trace", "p_trace"):
        if k in d:
            d[k] = d[k].reshape(n_iter, B, n)
    for k in ("mean", "var"):
        d[k] = d[k].reshape(B, n)
    for k in ("A", "dH", "accepted"):
        d[k] = d[k].reshape(B, n_iter)
    d["accepted"] = d["accepted"].astype(np.int32)
    d["kept"] = d["kept"].reshape(B, n_iter // thin, len(keep))
    return d


def _noise(n_iter, B, n, seed=3):
    rs = np.random.RandomState(seed)
    z = rs.randn(n_iter, B, n + 2)
    z[:, :, n:] = rs.uniform(0.05, 1.0, (n_iter, B, 2))
    return z


def _start(B, seed):
    x0 = 0.8 * np.random.RandomState(seed).randn(B, 6)
    assert np.all(x0 > LO6) and np.all(x0 < HI6)
    return x0


@pytest.mark.parametrize("minv_kind", [0, 1, 2])
def test_host_chain_equals_the_numpy_chain(exe, tmp_path, minv_kind):
    """B = 3, n = 6 with kinds [3, 1, 2, 0, 3, 1], 12 iterations of 5 steps, per-chain step sizes, jitter, thin = 2, scattered
    kept columns, each shape of minv: z, x, momenta, running statistics and kept columns bit for bit; every decision equal;
    dH within the bound _hmc_box_ref derives"""
    B, n, n_iter, n_leap = 3, 6, 12, 5
    assert list(BR.box_kinds(LO6, HI6)) == [3, 1, 2, 0, 3, 1]
    rs = np.random.RandomState(11)
    x0 = _start(B, 21)
    minv = [None, rs.uniform(0.5, 2.0, n), rs.uniform(0.5, 2.0, (B, n))][minv_kind]
    eps, noise, keep = np.array([0.9, 0.45, 0.2]), _noise(n_iter, B, n), [5, 0, 3]
    z0 = BR.box_inverse(BR.box_kinds(LO6, HI6), LO6, HI6, x0)
    ref = BR.chain_box(z0, R.quadratic_action_grad(H), LO6, HI6, eps, n_iter, n_leap, noise, jitter=0.3, minv=minv, thin=2, keep_idx=keep)
    assert BR.decisions_are_safe(ref)
    assert 0 < ref["accepted"].sum() < ref["accepted"].size                    # (both outcomes occur)
    got = _host_chain(exe, tmp_path, x0, LO6, HI6, eps, n_iter, n_leap, noise, jitter=0.3, minv=minv, thin=2, keep=keep)
    assert np.array_equal(got["accepted"], ref["accepted"])
    for k in ("z_trace", "x_trace", "p_trace", "mean", "var", "A", "kept"):
        assert np.array_equal(got[k], ref[k]), k
    assert np.all(got["x_trace"] >= LO6) and np.all(got["x_trace"] <= HI6)
    err = np.abs(got["dH"] - ref["dH"])
    print("|dH host - dH numpy| / bound: at most %.3f" % (err / ref["dh_bound"]).max())
    assert np.all(err <= ref["dh_bound"])


def test_all_free_bounds_give_the_unbounded_samplers_bits(exe, exe_plain, tmp_path):
    """kind 0 everywhere through hmc_host_box, against hmc_host on the same noise: every output bit for bit, dH included
    (A - 0 = A and x = z are exact)"""
    B, n, n_iter, n_leap = 3, 6, 12, 5
    x0 = _start(B, 22)
    eps, noise, keep = np.array([0.9, 0.45, 0.2]), _noise(n_iter, B, n), [5, 0, 3]
    free_lo, free_hi = np.full(n, -INF), np.full(n, INF)
    box = _host_chain(exe, tmp_path, x0, free_lo, free_hi, eps, n_iter, n_leap, noise, jitter=0.3, thin=2, keep=keep)
    plain = _host_chain(exe_plain, tmp_path, x0, None, None, eps, n_iter, n_leap, noise, jitter=0.3, thin=2, keep=keep, box=False)
    assert 0 < plain["accepted"].sum() < plain["accepted"].size
    for k in plain:
        assert np.array_equal(box[k], plain[k]), k
    assert np.array_equal(box["z_trace"], box["x_trace"])


def _hess_U_rowsum(Z, G):
    """largest absolute row sum of the Hessian of U at Z (one chain): diag(dx) H diag(dx) + diag(g d2x - d2lj), d2x = dx dlj,
    d2lj by a centred difference of dlj in longdouble"""
    kind = BR.box_kinds(LO6, HI6)
    _, dx, dlj, _ = BR.box_map(kind, LO6, HI6, Z)
    h = LD(2.0) ** -20 * np.maximum(1.0, np.abs(Z))
    d2lj = ((BR.box_map(kind, LO6, HI6, Z.astype(LD) + h, dtype=LD)[2] - BR.box_map(kind, LO6, HI6, Z.astype(LD) - h, dtype=LD)[2]) / (2 * h)).astype(np.float64)
    J = dx[:, None] * H * dx[None, :] + np.diag(G * dx * dlj - d2lj)
    return np.abs(J).sum(axis=1).max()


def test_reversing_the_momentum_returns_to_the_start(exe, tmp_path):
    """_hmc_ref's reverse_bound as it stands, with hmax the largest absolute row sum of U's Hessian in z met on the way and S
    the largest magnitude among z, p, x, g and gz.  Short steps from a start in the flat middle of every box (eps = 0.02,
    L = 4) keep the amplification (1 + eps (1 + hmax))^(2 L) near 10^2, so the bound is a statement: it lies many orders
    below the distance the trajectory covers, and a reversal with ONE momentum component left un-negated misses it by
    orders too.  Measured with the committed numbers: |z back - z start| = 1.4e-17 against a bound of 1.6e-12 (hmax 25.7,
    S 3.7; the bound is a worst case over 8 steps of 16 roundings each, the error an ulp of z), distance covered 0.146,
    the wrong reversal off by 3.7e-2."""
    B, n, L, eps = 1, 6, 4, 0.02
    x0 = 0.3 * np.random.RandomState(5).randn(B, n)
    assert np.all(x0 > LO6) and np.all(x0 < HI6)
    noise = _noise(2, B, n)
    noise[:, :, n] = 1e-300                                                     # log u = -690: both iterations are accepted
    first = _host_chain(exe, tmp_path, x0, LO6, HI6, eps, 1, L, noise[:1])
    noise[1, :, :n] = -first["p_trace"][0]                                      # (identity mass: p = z)
    both = _host_chain(exe, tmp_path, x0, LO6, HI6, eps, 2, L, noise)
    assert both["accepted"].all() and np.array_equal(both["z_trace"][0], first["z_trace"][0])
    # the trajectory once more in NumPy, for the magnitudes and the Hessian along it
    kind = BR.box_kinds(LO6, HI6)
    z0 = BR.box_inverse(kind, LO6, HI6, x0)
    f = R.quadratic_action_grad(H)
    Z, P, S, hmax = z0.copy(), noise[0, :, :n].copy(), 0.0, 0.0
    for l in range(L + 1):
        X, dx, dlj, _ = BR.box_map(kind, LO6, HI6, Z)
        G = f(X)[1]
        GZ = np.where(kind == 0, G, G * dx - dlj)
        hmax = max(hmax, _hess_U_rowsum(Z[0], G[0]))
        S = max([S] + [np.abs(v).max() for v in (Z, P, X, G, GZ)])
        P = P - (0.5 * eps if l in (0, L) else eps) * GZ
        if l < L:
            Z = Z + eps * P
    assert np.array_equal(Z, first["z_trace"][0]) and np.array_equal(P, first["p_trace"][0])
    bound = R.reverse_bound(L, eps, hmax, S)
    err = np.abs(both["z_trace"][1] - z0).max()
    moved = np.abs(first["z_trace"][0] - z0).max()
    print("|z back - z start| = %.3e, bound %.3e (hmax %.3f, S %.3f), distance covered %.3e" % (err, bound, hmax, S, moved))
    assert err <= bound
    assert np.abs(both["p_trace"][1] + noise[0, :, :n]).max() <= bound
    assert bound < 1e-8 * moved                                                 # the bound says something ...
    wrong = noise.copy()
    wrong[1, 0, 2] = -wrong[1, 0, 2]                                            # ... one component not reversed
    off = _host_chain(exe, tmp_path, x0, LO6, HI6, eps, 2, L, wrong)
    miss = np.abs(off["z_trace"][1] - z0).max()
    print("one momentum component not reversed: off by %.3e" % miss)
    assert off["accepted"].all() and miss > 1e6 * bound


# ---------------------------------------------------------------- argument checks
@pytest.mark.parametrize("case,rc,words", [("lo_eq_hi", "1", ["lower[0] = 1 >= upper[0] = 1"]), ("lo_gt_hi", "1", ["lower[2] = 3 >= upper[2] = 2"]),
                                           ("lo_nan", "1", ["lower[1]", "NaN"]), ("on_lower", "1", ["XP[1][2] = 0.5", "not strictly inside"]),
                                           ("on_upper", "1", ["XP[0][1] = 2", "not strictly inside"]), ("outside", "1", ["XP[1][0] = 1.5"]),
                                           ("start_nan", "1", ["XP[0][3]"]), ("z_inf", "1", ["Z0[1][1]", "not finite"]),
                                           ("no_bounds", "4", ["no bounds", "va_hmc samples unbounded"])])
def test_refusals_are_named(exe, case, rc, words):
    got, why = _out(exe, "args", case).split(" ", 1)
    assert got == rc
    for w in words:
        assert w in why, why


@pytest.mark.parametrize("case", ["good", "good_z"])
def test_valid_arguments_pass(exe, case):
    out = _out(exe, "args", case)
    assert out.split()[0] == "0" and out.strip().endswith("kinds 3 2 1 0")
