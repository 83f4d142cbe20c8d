"""NumPy reference of the device sampler (csrc/va_hmc.h), written independently of it (TEST INFRASTRUCTURE).

    philox4x32_10   the counter-based generator in NumPy integer arithmetic (uint64 products split by shifts and masks)
    words / u01 / box_muller / noise_row    what one (seed, chain, iteration) draws
    chain           B Hamiltonian Monte Carlo chains with the action and its gradient passed in as a callable

The chain evaluates every element-wise expression in the order csrc/va_hmc.h documents, one rounding per operation, which
is what NumPy does with float64 arrays; so positions, momenta, running means and sums of squared deviations must agree
with the device BIT FOR BIT as long as the accept decisions agree.  What cannot agree bit for bit, and its bounds:

TOL_DH -- the energy error dH = (A1 + K1) - (A0 + K0).  A0 and A1 are the evaluator's own numbers on both sides.  K0 and K1
are sums of n_var non-negative terms 1/2 p_i^2 minv_i, added in a different order here (numpy's pairwise sum) and there
(lane, tree, workgroup).  Any order of recursive summation of n terms is off the exact sum by at most (n - 1) u sum|t_i|
(Higham, Accuracy and Stability of Numerical Algorithms, section 4.2), u = 2^-53; two orders differ by at most twice that,
and the three additions that form dH add 3 u (|A0| + |A1| + K0 + K1).  Hence, with terms = the 2 n_var kinetic terms and
|A0|, |A1|,
        |dH_dev - dH_ref| <= n_var 2^-52 sum|terms|          (dh_bound(); n_var >= 3 covers the last three additions)
An iteration whose log(u) + dH lies within that bound (plus the 1 ulp of log, below) could be decided either way: a test
chooses its noise so that none does, and asserts so on this side (decision_margin).

TOL_NORMAL -- the normals z = sqrt(-2 log u1) cos(2 pi u2).  The HIP device library documents at most 1 ulp for log, 1 ulp
for sqrt and 2 ulp for cos in double precision (ROCm "HIP math API": Double precision mathematical functions); NumPy's are
within 1 ulp each.  With r = sqrt(-2 log u1) <= sqrt(64 log 2) = 6.66 (u1 >= 2^-32), e = 2^-52 one ulp relative:
  log     relative 1 e each side; the square root halves it: r differs by (1/2)(1 + 1) e + (1 + 1) e (sqrt itself) = 3 e r
  cos     the argument 2 pi u2 is the same double on both sides (one rounded product); 2 + 1 ulp of a value <= 1: 3 e absolute
  product one rounding each side: 2 e |z|
so |z_dev - z_ref| <= r (3 e + 3 e + 2 e) = 8 e r, which is what normal_bound() returns (e = 2^-52 is the largest
relative size of an ulp, at the bottom of a binade, so nothing is added for binade edges).  The host phases' normals
(glibc's log, sqrt, cos: within 1 ulp each, sqrt exact) are held to the same bound.

reverse_bound -- leapfrog is time-reversible in exact arithmetic.  Each of the 2 L steps (L forward, L back) rounds p and x
once per operation, 4 operations each: at most 8 u (|x| + |p| + eps |g| + eps |p|) <= 16 u S per step with S the largest
magnitude met, and a step's linearisation amplifies earlier errors by at most (1 + eps (1 + hmax)), hmax the largest
absolute row sum of the Hessian (minv = 1).  Hence |x_back - x_start| <= 2 L 16 u S (1 + eps (1 + hmax))^(2 L).
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(key, ctr):
    """key (k0, k1), ctr (c0, c1, c2, c3): integers or equal-shaped integer arrays; returns uint32 array (..., 4)"""
    k0, k1 = (np.asarray(v, dtype=np.uint64) & M32 for v in key)
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(v, dtype=np.uint64) & M32 for v in ctr])
    m0c, m1c = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    for _ in range(10):
        p0 = m0c * c0                      # < 2^64: both factors are below 2^32
        p1 = m1c * c2
        hi0, lo0 = p0 >> np.uint64(32), p0 & M32
        hi1, lo1 = p1 >> np.uint64(32), p1 & M32
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + w0) & M32
        k1 = (k1 + w1) & M32
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def words(seed, chain, iteration, n):
    """(n + 1, 4): stream 0 of the elements 0 .. n - 1, then the extra stream (element 0, stream 1)"""
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    el = philox4x32_10(key, (chain, iteration, np.arange(n, dtype=np.uint64), 0))
    ex = philox4x32_10(key, (chain, iteration, 0, 1))
    return np.concatenate([el.reshape(n, 4), ex.reshape(1, 4)], axis=0)


def u01(w):
    return (np.asarray(w, dtype=np.float64) + 1.0) * 2.0 ** -32


def box_muller(w0, w1):
    r = np.sqrt(-2.0 * np.log(u01(w0)))
    return r * np.cos(6.283185307179586 * u01(w1))


def normal_bound(w0):
    return 8.0 * 2.0 ** -52 * np.sqrt(-2.0 * np.log(u01(w0)))


def noise_row(seed, chain, iteration, n):
    """one (chain, iteration) row of the sampler's `noise`: n normals, accept uniform, jitter uniform"""
    w = words(seed, chain, iteration, n)
    return np.concatenate([box_muller(w[:n, 0], w[:n, 1]), u01(w[n, :2])])


def chain(X0, action_grad, eps, n_iter, n_leap, noise, jitter=0.0, minv=None, thin=1, keep_idx=None):
    """X0 (B, n); action_grad(X) -> (A (B,), G (B, n)); eps scalar or (B,); noise (n_iter, B, n + 2); minv None, (n,) or (B, n).
    Returns a dict: x (final), x_trace, p_trace (n_iter, B, n) (state after / momentum at the end of each iteration), mean,
    var, A, dH, accepted (B, n_iter), n_divergent, kept, dh_bound, margin (B, n_iter)."""
    X = np.array(X0, dtype=np.float64)
    B, n = X.shape
    eps = np.broadcast_to(np.asarray(eps, dtype=np.float64).reshape(-1), (B,))
    mi = np.ones((B, n)) if minv is None else np.array(np.broadcast_to(np.asarray(minv, dtype=np.float64), (B, n)))
    smi = np.sqrt(mi)
    keep = np.zeros(0, np.intp) if keep_idx is None else np.asarray(keep_idx, dtype=np.intp)
    A, G = action_grad(X)
    A, G = np.array(A, dtype=np.float64), np.array(G, dtype=np.float64)
    mean, m2 = np.zeros((B, n)), np.zeros((B, n))
    out = dict(x_trace=np.empty((n_iter, B, n)), p_trace=np.empty((n_iter, B, n)), A=np.empty((B, n_iter)), dH=np.empty((B, n_iter)),
               accepted=np.empty((B, n_iter), np.int32), dh_bound=np.empty((B, n_iter)), margin=np.empty((B, n_iter)),
               kept=np.empty((B, n_iter // thin, keep.size)))
    for it in range(n_iter):
        z, u_acc, u_jit = noise[it, :, :n], noise[it, :, n], noise[it, :, n + 1]
        P = z / smi
        Xs, Gs, A0 = X.copy(), G.copy(), A.copy()
        t0 = 0.5 * ((P * P) * mi)
        e = (eps * (1.0 + jitter * (2.0 * u_jit - 1.0)))[:, None]
        half = 0.5 * e
        c = e * mi
        A1 = A0
        for l in range(n_leap):
            P = P - (half if l == 0 else e) * G
            X = X + c * P
            A1, G = action_grad(X)
            A1, G = np.array(A1, dtype=np.float64), np.array(G, dtype=np.float64)
        P = P - half * G
        t1 = 0.5 * ((P * P) * mi)
        with np.errstate(invalid="ignore", over="ignore"):
            K0, K1 = t0.sum(axis=1), t1.sum(axis=1)
            dH = (A1 + K1) - (A0 + K0)
            acc = np.isfinite(dH) & (np.log(u_acc) < -dH)
            out["dh_bound"][:, it] = n * 2.0 ** -52 * (t0.sum(axis=1) + t1.sum(axis=1) + np.abs(A0) + np.abs(A1))
            out["margin"][:, it] = np.abs(np.log(u_acc) + dH)
        X = np.where(acc[:, None], X, Xs)
        G = np.where(acc[:, None], G, Gs)
        A = np.where(acc, A1, A0)
        d = X - mean
        mean = mean + d / float(it + 1)
        m2 = m2 + d * (X - mean)
        out["x_trace"][it], out["p_trace"][it] = X, P
        out["A"][:, it], out["dH"][:, it], out["accepted"][:, it] = A, dH, acc
        if (it + 1) % thin == 0:
            out["kept"][:, (it + 1) // thin - 1] = X[:, keep]
    out.update(x=X, mean=mean, var=m2 / (n_iter - 1) if n_iter > 1 else np.zeros((B, n)),
               n_divergent=(~np.isfinite(out["dH"])).sum(axis=1).astype(np.int32))
    return out


def decisions_are_safe(ref):
    """no iteration's log(u) + dH within the summation-order bound (plus one ulp of the logarithm): device and reference
    must then decide alike"""
    fin = np.isfinite(ref["dH"])
    slack = ref["dh_bound"] + 2.0 ** -52 * (np.abs(ref["dH"]) + 800.0)
    return bool(np.all(~fin | (ref["margin"] > 4.0 * slack)))


def reverse_bound(L, eps, hmax, S):
    return 2.0 * L * 16.0 * 2.0 ** -53 * S * (1.0 + eps * (1.0 + hmax)) ** (2 * L)


# ---------------------------------------------------------------- the CPU tests' action: a tridiagonal SPD quadratic
def tridiag_hessian(n=6):
    H = np.zeros((n, n))
    for i in range(n):
        H[i, i] = 2.0 + 0.25 * i
        if i + 1 < n:
            H[i, i + 1] = H[i + 1, i] = -0.75
    return H


def quadratic_action_grad(H):
    """A = 1/2 x^T H x and g = H x for a tridiagonal H, row by row in the order the CPU check program uses:
    g_i = (H[i,i-1] x[i-1] + H[i,i] x[i]) + H[i,i+1] x[i+1],  A = 1/2 sum_i x_i g_i in index order"""
    n = H.shape[0]
    d, o = np.diag(H).copy(), np.diag(H, 1).copy()

    def f(X):
        G = d * X
        G[:, 1:] = o * X[:, :-1] + G[:, 1:]
        G[:, :-1] = G[:, :-1] + o * X[:, 1:]
        A = np.zeros(X.shape[0])
        for i in range(n):
            A = A + X[:, i] * G[:, i]
        return 0.5 * A, G
    return f
