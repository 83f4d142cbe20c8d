"""NumPy reference of the box sampler (csrc/va_hmc_box.h), written independently of it (TEST INFRASTRUCTURE).

    box_kinds / box_map / box_inverse   the map x = T(z) of one entry, its slope, the slope's log and that log's derivative
    chain_box                           _hmc_ref.chain with the chain run in z on U(z) = A(T(z)) - sum log|dx/dz|

Positions and momenta need + - * / sqrt only, each correctly rounded in IEEE arithmetic and evaluated here in the order
the header writes them, so z, x, p, the running statistics and the kept columns must agree with the device BIT FOR BIT as
long as the accept decisions agree.  box_map takes a dtype: in np.longdouble it is the yardstick of the difference
quotients of tests/test_hmc_box_cpu.py.

dh_bound -- dH = ((A1 - L1) + K1) - ((A0 - L0) + K0), L = sum_i lj_i the log-Jacobian sums.  _hmc_ref derives
n 2^-52 sum|terms| for terms = the 2 n kinetic terms, |A0| and |A1|: (n - 1) 2^-52 sum for two orders of recursive summation,
the rest for the three additions.  The box sampler adds the 2 n terms lj_i (n at the start, n at the end of the
trajectory) to `terms`, and
  * their two sums are again added in another order here and there: covered by the same (n - 1) 2^-52 sum|terms|, now over
    all 4 n + 2 terms;
  * every lj_i is a logarithm of the SAME double on both sides (the slope is bit-equal), within 1 ulp of the true value by
    each library (ROCm "HIP math API", glibc and NumPy: 1 ulp for log in double), so the two differ by at most 2 ulp:
    2 2^-52 |lj_i| each, 2 2^-52 sum|terms| at most in all;
  * dH is now formed by five additions instead of three, each rounding at most 2^-53 of a magnitude below sum|terms|:
    2.5 2^-52 sum|terms|.
Hence |dH_dev - dH_ref| <= (n - 1 + 2 + 2.5) 2^-52 sum|terms| <= (n + 4) 2^-52 sum|terms|, what chain_box returns as
dh_bound.  _hmc_ref.decisions_are_safe() applies to it unchanged (its slack already carries the logarithm of the accept
uniform).

reverse_bound is _hmc_ref's with hmax taken for U: the Hessian of U in z is diag(dx) H_x diag(dx) + diag(g_x d2x - d2lj),
and a test passes the largest absolute row sum of that matrix along its trajectory (by differences of box_map).
"""
import numpy as np

import _hmc_ref as R


# the table the CPU and the GPU test of the map share: every box at every z of +-[1e-9, 1e9] and 0
BOXES = [(-np.inf, np.inf), (0.0, np.inf), (-12.0, np.inf), (-np.inf, 1.0), (-np.inf, 14.0), (-0.5, 1.5), (-15.0, 15.0), (0.5, 100.0)]
Z_TABLE = np.concatenate([-(10.0 ** np.linspace(-9.0, 9.0, 37))[::-1], [0.0], 10.0 ** np.linspace(-9.0, 9.0, 37)])


def map_table():
    """(lo, hi, z)"""
    lo = np.repeat([b[0] for b in BOXES], Z_TABLE.size)
    hi = np.repeat([b[1] for b in BOXES], Z_TABLE.size)
    return lo, hi, np.tile(Z_TABLE, len(BOXES))


def box_kinds(lo, hi):
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    return (np.isfinite(lo) * 1 + np.isfinite(hi) * 2).astype(np.int32)


def bounds_arrays(bounds):
    lo = np.array([-np.inf if b[0] is None else b[0] for b in bounds], dtype=np.float64)
    hi = np.array([np.inf if b[1] is None else b[1] for b in bounds], dtype=np.float64)
    return lo, hi


def box_map(kind, lo, hi, z, dtype=np.float64):
    """(x, dx/dz, d log|dx/dz| / dz, log|dx/dz|) entry by entry; kind, lo, hi broadcast against z"""
    z = np.asarray(z, dtype=dtype)
    kind = np.broadcast_to(np.asarray(kind), z.shape)
    lo = np.broadcast_to(np.asarray(lo, dtype=dtype), z.shape)
    hi = np.broadcast_to(np.asarray(hi, dtype=dtype), z.shape)
    one, two, three, four = dtype(1.0), dtype(2.0), dtype(3.0), dtype(4.0)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        zz = z * z
        # kinds 1 and 2
        r2 = zz + four
        r = np.sqrt(r2)
        w = np.where(z >= 0, (z + r) / two, two / (r - z))
        d12 = w / r
        dlj12 = one / r - z / r2
        # kind 3
        q2 = one + zz
        q = np.sqrt(q2)
        s = (one + z / q) / two
        wd = hi - lo
        x3 = np.minimum(np.maximum(lo + wd * s, lo), hi)
        d3 = wd / (two * (q * q * q))
        dlj3 = (-three * z) / q2
        x = np.where(kind == 0, z, np.where(kind == 1, lo + w, np.where(kind == 2, hi - w, x3)))
        dx = np.where(kind == 0, one, np.where(kind == 1, d12, np.where(kind == 2, -d12, d3)))
        dlj = np.where(kind == 0, dtype(0.0), np.where(kind == 3, dlj3, dlj12))
        lj = np.where(kind == 0, dtype(0.0), np.log(np.where(kind == 3, d3, d12)))
    return x, dx, dlj, lj


def box_inverse(kind, lo, hi, x):
    x = np.asarray(x, dtype=np.float64)
    kind = np.broadcast_to(np.asarray(kind), x.shape)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        w = np.where(kind == 1, x - lo, hi - x)
        z12 = w - 1.0 / w
        u = 2.0 * (x - lo) / (hi - lo) - 1.0
        z3 = u / np.sqrt((1.0 - u) * (1.0 + u))
    return np.where(kind == 0, x, np.where(kind == 3, z3, z12))


def chain_box(Z0, action_grad, lo, hi, eps, n_iter, n_leap, noise, jitter=0.0, minv=None, thin=1, keep_idx=None, jacobian=True):
    """Z0 (B, n) the start in z; action_grad(X) -> (A (B,), G (B, n)) in x; lo, hi (n,).  jacobian=False drops the
    log-Jacobian terms from the gradient and the energy (the WRONG sampler a test wants to see fail).  Returns
    _hmc_ref.chain's dict (x_trace, mean, var, kept of x) plus z, z_trace and x0 = T(Z0)."""
    Z = np.array(Z0, dtype=np.float64)
    B, n = Z.shape
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    kind = box_kinds(lo, hi)
    free = kind == 0
    eps = np.broadcast_to(np.asarray(eps, dtype=np.float64).reshape(-1), (B,))
    mi = np.ones((B, n)) if minv is None else np.array(np.broadcast_to(np.asarray(minv, dtype=np.float64), (B, n)))
    smi = np.sqrt(mi)
    keep = np.zeros(0, np.intp) if keep_idx is None else np.asarray(keep_idx, dtype=np.intp)
    X = box_map(kind, lo, hi, Z)[0]
    x0 = X.copy()

    def ag(X):
        A, G = action_grad(X)
        return np.array(A, dtype=np.float64), np.array(G, dtype=np.float64)

    def grad_z(Z, G):
        _, dx, dlj, lj = box_map(kind, lo, hi, Z)
        if not jacobian:
            return np.where(free, G, G * dx), np.zeros_like(lj)
        return np.where(free, G, G * dx - dlj), lj
    A, G = ag(X)
    mean, m2 = np.zeros((B, n)), np.zeros((B, n))
    out = dict(x_trace=np.empty((n_iter, B, n)), z_trace=np.empty((n_iter, B, n)), p_trace=np.empty((n_iter, B, n)), A=np.empty((B, n_iter)),
               dH=np.empty((B, n_iter)), accepted=np.empty((B, n_iter), np.int32), dh_bound=np.empty((B, n_iter)),
               margin=np.empty((B, n_iter)), kept=np.empty((B, n_iter // thin, keep.size)))
    for it in range(n_iter):
        nz, u_acc, u_jit = noise[it, :, :n], noise[it, :, n], noise[it, :, n + 1]
        P = nz / smi
        Zs, Xs, Gs, A0 = Z.copy(), X.copy(), G.copy(), A.copy()
        t0 = 0.5 * ((P * P) * mi)
        e = (eps * (1.0 + jitter * (2.0 * u_jit - 1.0)))[:, None]
        half = 0.5 * e
        c = e * mi
        A1 = A0
        GZ, l0 = grad_z(Z, G)
        for l in range(n_leap):
            P = P - (half if l == 0 else e) * GZ
            Z = Z + c * P
            X = box_map(kind, lo, hi, Z)[0]
            A1, G = ag(X)
            GZ, l1 = grad_z(Z, G)
        P = P - half * GZ
        t1 = 0.5 * ((P * P) * mi)
        with np.errstate(invalid="ignore", over="ignore"):
            K0, K1, L0, L1 = t0.sum(axis=1), t1.sum(axis=1), l0.sum(axis=1), l1.sum(axis=1)
            dH = ((A1 - L1) + K1) - ((A0 - L0) + K0)
            acc = np.isfinite(dH) & (np.log(u_acc) < -dH)
            terms = t0.sum(axis=1) + t1.sum(axis=1) + np.abs(l0).sum(axis=1) + np.abs(l1).sum(axis=1) + np.abs(A0) + np.abs(A1)
            out["dh_bound"][:, it] = (n + 4) * 2.0 ** -52 * terms
            out["margin"][:, it] = np.abs(np.log(u_acc) + dH)
        Z = np.where(acc[:, None], Z, Zs)
        X = np.where(acc[:, None], X, Xs)
        G = np.where(acc[:, None], G, Gs)
        A = np.where(acc, A1, A0)
        d = X - mean
        mean = mean + d / float(it + 1)
        m2 = m2 + d * (X - mean)
        out["x_trace"][it], out["z_trace"][it], out["p_trace"][it] = X, Z, P
        out["A"][:, it], out["dH"][:, it], out["accepted"][:, it] = A, dH, acc
        if (it + 1) % thin == 0:
            out["kept"][:, (it + 1) // thin - 1] = X[:, keep]
    out.update(x=X, z=Z, x0=x0, mean=mean, var=m2 / (n_iter - 1) if n_iter > 1 else np.zeros((B, n)),
               n_divergent=(~np.isfinite(out["dH"])).sum(axis=1).astype(np.int32))
    return out


decisions_are_safe = R.decisions_are_safe
