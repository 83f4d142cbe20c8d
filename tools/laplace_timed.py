"""What state error bars cost: Annealer.laplace (va_laplace: k_hvp, k_hblocks, k_selinv; csrc/va_selinv.h) against the host
route it replaces (Annealer.param_covariance: the coloured products over PCIe, Python's banded assembly, SciPy's
cholesky_banded and the Schur complement, one seed at a time) on the same 64 minimisers of the shipped example's shape
(Lorenz-96, D = 20, N = 161, one estimated parameter), trapezoid (W = 20, K = 161) and Simpson-Hermite (W = 40, K = 81).

    python tools/laplace_timed.py [--out profiles/laplace_timed.json] [--reps 3] [--skip-host]

Wall clock around the whole call, the median of --reps calls after a warm-up; Gauss-Newton Hessians, so that every point is
positive definite whatever the rung.  The host route returns the parameter covariance only; the device route returns the
state variances, the parameter covariance and log det H.  Per-kernel times come from a kernel trace of this script
(rocprofv3 --kernel-trace --stats -- python tools/laplace_timed.py --reps 1 --skip-host), not from here.  No ratio is a
threshold."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from varanneal_amd import twin, va_ode      # noqa: E402


def l96(t, x, k):
    return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - x + k


def median_ms(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), out


def one_disc(disc, B, reps, skip_host):
    D, N = 20, 161
    t, Y, _, Lidx = twin.make_twin(D, N)
    X0 = np.empty((B, N, D)); P0 = np.empty((B, 1))
    for b in range(B):
        x, p = twin.initial_guess(N, D, b, Y, Lidx)
        X0[b] = x; P0[b] = p[0]
    a = va_ode.Annealer()
    a.set_model(l96, D)
    a.set_data(Y, t=twin.DT * np.arange(N))
    a.anneal(X0, P0, 1.5, [0, 10, 20], 4.0, 4e-6, Lidx, [0], disc=disc, verbose=False)
    res = dict(disc=disc, D=D, N=N, points=B, W=(2 if disc == "SimpsonHermite" else 1) * D)
    res["laplace_ms"], r = median_ms(lambda: a.laplace(beta=-1, gauss_newton=True), reps)
    res["laplace_full_ms"], _ = median_ms(lambda: a.laplace(beta=-1, gauss_newton=True, full=True), reps)
    res["status_ok"] = int((r["status"] == 0).sum())
    res["rms_sigma_observed"] = float(np.sqrt(np.mean(r["state_var"][:, 0][:, :, Lidx])))
    unobs = [j for j in range(D) if j not in set(Lidx)]
    res["rms_sigma_unobserved"] = float(np.sqrt(np.mean(r["state_var"][:, 0][:, :, unobs])))
    if not skip_host:
        res["host_param_covariance_ms"], cov = median_ms(lambda: a.param_covariance(beta=-1, gauss_newton=True), max(1, reps // 3))
        res["param_cov_max_rel_diff"] = float(np.abs(cov - r["param_cov"][:, 0]).max() / np.abs(cov).max())
    a.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--points", type=int, default=64)
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()
    doc = dict(what="Annealer.laplace (device: k_hvp + k_hblocks + k_selinv, transfers included) against Annealer.param_covariance "
                    "(host: hess_vec per seed + banded assembly + SciPy) on the same minimisers, wall clock ms (median); no ratio is a threshold",
               runs=[one_disc(d, args.points, args.reps, args.skip_host) for d in ("trapezoid", "SimpsonHermite")], notes=[])
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")
