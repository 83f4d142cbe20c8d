"""What a forecast error bar costs: Annealer.predict_spread (laplace(full=True), a host Cholesky factor per point, then
va_predict_tangent: k_predict_tlm and k_spread, csrc/va_predict_tlm.h) on 64 minimisers of the shipped example's shape
(Lorenz-96, D = 20, N = 161, one estimated parameter, trapezoid), 40 steps ahead, against the same quantity on the host:
the NumPy tangent-linear RK4 of tests/_tlm_ref.py driven, one point at a time, from the same laplace output.

    python tools/spread_timed.py [--out profiles/spread_timed.json] [--reps 3] [--skip-host]

Wall clock around the whole call, transfers included, the median of --reps calls after a warm-up; Gauss-Newton Hessians, so
that every point is positive definite whatever the rung.  No ratio is a threshold."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _predict_ref import l96 as l96_row      # noqa: E402
from _tlm_ref import l96_jvp, tlm_rk4        # noqa: E402
from varanneal_amd import twin, va_ode       # noqa: E402


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


def host_spread(a, lap, n_steps, beta):
    """std (B, n_out, D) of rung `beta` from laplace's output: Cholesky, the NumPy tangent-linear RK4, sums of squares"""
    N, D = a.N_model, a.D
    mp = a.minpaths[:, beta]
    std = []
    for b in range(mp.shape[0]):
        S0 = np.empty((D + 1, D + 1))
        S0[:D, :D], S0[D:, :D] = lap["state_cov"][b, 0, N - 1], lap["state_param_cov"][b, 0, :, N - 1]
        S0[:D, D:], S0[D:, D:] = S0[D:, :D].T, lap["param_cov"][b, 0]
        V = np.linalg.cholesky(S0).T
        _, dX = tlm_rk4(l96_row, l96_jvp, mp[b, (N - 1) * D:N * D], mp[b, N * D], V, n_steps, twin.DT, t0=float(a.t_model[-1]))
        std.append(np.sqrt((dX * dX).sum(axis=0)))
    return np.array(std)


def run(B, n_steps, reps, skip_host):
    D, N = 20, 161
    t, Y, _, Lidx = twin.make_twin(D, N)
    X0 = np.empty((B, N, D)); P0 = np.empty((B, 1))
    for b in range(B):
        x, p = twin.initial_guess(N, D, b, Y, Lidx)
        X0[b] = x; P0[b] = p[0]
    a = va_ode.Annealer()
    a.set_model(l96, D)
    a.set_data(Y, t=twin.DT * np.arange(N))
    a.anneal(X0, P0, 1.5, [0, 10, 20], 4.0, 4e-6, Lidx, [0], disc="trapezoid", verbose=False)
    res = dict(disc="trapezoid", D=D, N=N, points=B, n_steps=n_steps, nvec=D + 1)
    res["predict_spread_ms"], r = median_ms(lambda: a.predict_spread(n_steps, beta=-1, gauss_newton=True), reps)
    res["predict_spread_full_ms"], _ = median_ms(lambda: a.predict_spread(n_steps, beta=-1, gauss_newton=True, full=True), reps)
    res["laplace_full_ms"], lap = median_ms(lambda: a.laplace(beta=-1, gauss_newton=True, full=True), reps)
    res["predict_ms"], _ = median_ms(lambda: a.predict(n_steps, beta=-1), reps)
    mp = a.minpaths[:, -1]
    V0 = np.zeros((B, D + 1, D + 1)); V0[:] = np.eye(D + 1)
    res["predict_tangent_ms"], _ = median_ms(lambda: a._pb.predict_tangent(mp[:, (N - 1) * D:N * D], mp[:, N * D:], V0, n_steps,
                                                                           t0=float(a.t_model[-1]), want=("var",)), reps)
    res["status_ok"] = int((r["status"] == 0).sum())
    res["rms_sigma_row0"] = float(np.sqrt(np.nanmean(r["std"][:, 0, 0] ** 2)))
    res["rms_sigma_last"] = float(np.sqrt(np.nanmean(r["std"][:, 0, -1] ** 2)))
    if not skip_host:
        res["host_numpy_tlm_ms"], hs = median_ms(lambda: host_spread(a, lap, n_steps, -1), max(1, reps // 3))
        ok = r["status"][:, 0] == 0
        res["std_max_rel_diff"] = float(np.abs(hs[ok] - r["std"][ok, 0]).max() / np.abs(hs[ok]).max())
    a.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--points", type=int, default=64)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()
    doc = dict(what="Annealer.predict_spread (device: laplace(full=True), host Cholesky, va_predict_tangent = k_predict_tlm + k_spread, "
                    "transfers included) against the NumPy tangent-linear RK4 on the host driven from the same laplace output "
                    "(host_numpy_tlm_ms: without laplace), wall clock ms (median); no ratio is a threshold",
               runs=[run(args.points, args.steps, args.reps, args.skip_host)], notes=[])
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")
