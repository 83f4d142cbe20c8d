"""What the strong-constraint refinement costs on each route: Annealer.shoot(device=True) -- every point's L-BFGS inside one
launch of k_shoot (csrc/va_shoot.h) -- against Annealer.shoot(device=False) -- SciPy's L-BFGS-B on the host around one
va_predict_adjoint call per evaluation and point -- on the same 64 points of Lorenz-96 at D = 20, N = 161, every second
column observed: rung 0 of an initialised annealer, whose paths start at an attractor state off by 1e-2 randn with k = 8.0.

    python tools/shoot_timed.py [--out profiles/shoot_timed.json] [--reps 3] [--points 64] [--skip-host]
    python tools/shoot_timed.py --box [--out profiles/shoot_box_timed.json]

--box: what the box costs.  In the same run, on the same points: shoot(device=True) without bounds, then with every entry
boxed to [-100, 100] (a two-sided box wide enough to stay inactive) shoot(device=True, box=True) -- k_shoot_box, one lane's
L-BFGS-B per point (csrc/va_shoot_box.h) -- and shoot(device=False), SciPy with the same bounds (one call, not warmed up).
Per-evaluation and per-iteration times beside them; at the same iteration counts the difference between the first two is
the step's cost.

Wall clock around the whole call, transfers included, the median of --reps calls after a warm-up of the device route (the
host route is not warmed up: one call is 64 minimisations).  Also nfev per point on both routes, and the kernel's time per
evaluation (call time / largest nfev of the call) beside profiles/adjoint_timed.json's time per host-driven call.  No figure
is a threshold."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _predict_ref import DT, K_TRUE, attractor_starts, l96, rk4      # noqa: E402
from varanneal_amd import va_ode                                      # noqa: E402


def _l96_user(t, x, k):
    return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - x + k


def timed(f, reps, warm):
    if warm:
        f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), out


def _annealer(B, D, N):
    Lidx = list(range(0, D, 2))
    rng = np.random.RandomState(2)
    truth = np.array(attractor_starts(D, B))
    Y = rk4(l96, truth[0], K_TRUE, N - 1, DT)[:, Lidx] + 0.05 * rng.randn(N, len(Lidx))
    X0 = np.empty((B, N, D))
    for b in range(B):
        X0[b] = rk4(l96, truth[0] + 1e-2 * rng.randn(D), 8.0, N - 1, DT)
    a = va_ode.Annealer()
    a.set_model(_l96_user, D)
    a.set_data(Y, t=DT * np.arange(N))
    a.anneal_init(X0, np.full((B, 1), 8.0), 2.0, [0], 1.0, 1.0, Lidx, [0], disc="trapezoid")
    return a, len(Lidx)


def _column(res, name, ms, r, per_point_calls=False):
    nfev = r["nfev"].reshape(-1)
    res[name + "_ms"] = ms
    res[name + "_nfev_min_median_max"] = [int(nfev.min()), float(np.median(nfev)), int(nfev.max())]
    res[name + "_status_counts"] = {str(int(s)): int((r["status"] == s).sum()) for s in np.unique(r["status"])}
    res[name + "_ms_per_evaluation"] = ms / float(nfev.sum() if per_point_calls else nfev.max())
    if "nit" in r:
        nit = r["nit"].reshape(-1)
        res[name + "_nit_min_median_max"] = [int(nit.min()), float(np.median(nit)), int(nit.max())]
        res[name + "_ms_per_iteration"] = ms / float(max(nit.max(), 1))
    res[name + "_cost_median"] = float(np.median(r["cost"]))


def run_box(B, D, N, reps, skip_host):
    a, nobs = _annealer(B, D, N)
    res = dict(D=D, N=N, points=B, observed_columns=nobs, box=[-100.0, 100.0])
    ms, r = timed(lambda: a.shoot(beta=0, device=True), reps, True)
    _column(res, "device", ms, r)
    a.bounds = [(-100.0, 100.0)] * (N * D + 1)
    ms, rb = timed(lambda: a.shoot(beta=0, device=True, box=True), reps, True)
    _column(res, "device_box", ms, rb)
    z = np.concatenate([rb["x0"].reshape(B, D), rb["params"].reshape(B, 1)], axis=1)
    res["device_box_entries_on_a_bound"] = int((np.abs(z) == 100.0).sum())
    res["device_box_over_device"] = res["device_box_ms"] / res["device_ms"]
    res["same_iteration_counts"] = bool(np.array_equal(r["nit"], rb["nit"]))
    res["largest_cost_difference_relative_box_vs_device"] = float((np.abs(rb["cost"] - r["cost"]) / r["cost"]).max())
    if not skip_host:
        ms, h = timed(lambda: a.shoot(beta=0, device=False), 1, False)
        _column(res, "host_bounds", ms, h, per_point_calls=True)
        res["host_over_device_box"] = res["host_bounds_ms"] / res["device_box_ms"]
        res["largest_cost_difference_relative_box_vs_host"] = float((np.abs(h["cost"] - rb["cost"]) / h["cost"]).max())
    a.bounds = None
    a.close()
    return res


def run(B, D, N, reps, skip_host):
    Lidx = list(range(0, D, 2))
    rng = np.random.RandomState(2)
    truth = np.array(attractor_starts(D, B))
    Y = rk4(l96, truth[0], K_TRUE, N - 1, DT)[:, Lidx] + 0.05 * rng.randn(N, len(Lidx))
    X0 = np.empty((B, N, D))
    for b in range(B):
        X0[b] = rk4(l96, truth[0] + 1e-2 * rng.randn(D), 8.0, N - 1, DT)
    a = va_ode.Annealer()
    a.set_model(_l96_user, D)
    a.set_data(Y, t=DT * np.arange(N))
    a.anneal_init(X0, np.full((B, 1), 8.0), 2.0, [0], 1.0, 1.0, Lidx, [0], disc="trapezoid")
    res = dict(D=D, N=N, points=B, observed_columns=len(Lidx))
    res["device_ms"], r = timed(lambda: a.shoot(beta=0, device=True), reps, True)
    nfev = r["nfev"].reshape(-1)
    res["device_nfev_min_median_max"] = [int(nfev.min()), float(np.median(nfev)), int(nfev.max())]
    res["device_status_counts"] = {str(int(s)): int((r["status"] == s).sum()) for s in np.unique(r["status"])}
    res["device_ms_per_evaluation"] = res["device_ms"] / float(nfev.max())
    res["device_cost_median"] = float(np.median(r["cost"]))
    if not skip_host:
        res["host_ms"], h = timed(lambda: a.shoot(beta=0, device=False), reps, False)
        hn = h["nfev"].reshape(-1)
        res["host_nfev_min_median_max"] = [int(hn.min()), float(np.median(hn)), int(hn.max())]
        res["host_status_counts"] = {str(int(s)): int((h["status"] == s).sum()) for s in np.unique(h["status"])}
        res["host_ms_per_evaluation"] = res["host_ms"] / float(hn.sum())
        res["host_cost_median"] = float(np.median(h["cost"]))
        res["host_over_device"] = res["host_ms"] / res["device_ms"]
        res["largest_cost_difference_relative"] = float((np.abs(h["cost"] - r["cost"]) / h["cost"]).max())
    a.close()
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--points", type=int, default=64)
    ap.add_argument("--rows", type=int, default=161)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--box", action="store_true")
    args = ap.parse_args()
    if args.box:
        doc = dict(what="Annealer.shoot(device=True) (k_shoot), Annealer.shoot(device=True, box=True) (k_shoot_box: one lane's L-BFGS-B "
                        "per point) with every entry boxed to an inactive [-100, 100], and Annealer.shoot(device=False) (SciPy with the "
                        "same bounds, one call) on the same points in one run; wall clock ms with transfers (median of %d); no figure "
                        "is a threshold" % args.reps,
                   runs=[run_box(args.points, 20, args.rows, args.reps, args.skip_host)], notes=[])
        txt = json.dumps(doc, indent=1)
        print(txt)
        if args.out:
            with open(args.out, "w") as fh:
                fh.write(txt + "\n")
        sys.exit(0)
    doc = dict(what="Annealer.shoot(device=True) (k_shoot: all points' L-BFGS in one launch, then one predict() call) against "
                    "Annealer.shoot(device=False) (SciPy on the host, one va_predict_adjoint call per evaluation and point) on the "
                    "same points, wall clock ms with transfers (median of %d); no figure is a threshold" % args.reps,
               runs=[run(args.points, 20, args.rows, args.reps, args.skip_host)], notes=[])
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")
