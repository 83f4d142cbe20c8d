"""What a gradient of the forecast costs: one misfit-mode call of va_predict_adjoint (k_predict_adj, csrc/va_predict_adj.h:
forward with checkpoints, then the backward sweep) on 64 trajectories of Lorenz-96 at D = 20 over 160 steps, every second
column observed, against va_predict over the same steps and against the NumPy adjoint of tests/_adj_ref.py per trajectory.

    python tools/adjoint_timed.py [--out profiles/adjoint_timed.json] [--reps 7] [--skip-host]

Wall clock around the whole call, transfers included, the median of --reps calls after a warm-up.  No ratio is a threshold."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _adj_ref                                           # noqa: E402
from _predict_ref import DT, K_TRUE, attractor_starts, l96      # noqa: E402
from varanneal_amd import _capi                            # noqa: E402


def median_ms(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), out


def run(T, D, n_steps, reps, skip_host):
    Lidx = list(range(0, D, 2))
    rng = np.random.RandomState(1)
    x0 = np.array(attractor_starts(D, T))
    p = np.full((T, 1), K_TRUE)
    w = np.full(len(Lidx), 1.0 / (len(Lidx) * (n_steps + 1)))
    res = dict(D=D, trajectories=T, n_steps=n_steps, observed_columns=len(Lidx))
    with _capi.Problem(1, D, 5, np.zeros((5, len(Lidx))), Lidx, DT, 4.0, 1e-2, np.array([[K_TRUE]]), [0]) as pb:
        out = pb.predict(x0, p, n_steps)
        Y = np.ascontiguousarray(out[:, :, Lidx] + 0.5 * rng.randn(T, n_steps + 1, len(Lidx)))
        res["predict_ms"], _ = median_ms(lambda: pb.predict(x0, p, n_steps), reps)
        res["predict_adjoint_misfit_ms"], r = median_ms(lambda: pb.predict_adjoint(x0, p, n_steps, Y=Y, weights=w), reps)
        G = np.zeros((T, 1, n_steps + 1, D))
        G[:, 0][:, :, Lidx] = 2.0 * w * (out[:, :, Lidx] - Y)
        res["predict_adjoint_cotangent_ms"], _ = median_ms(lambda: pb.predict_adjoint(x0, p, n_steps, G=G), reps)
    res["adjoint_over_predict"] = res["predict_adjoint_misfit_ms"] / res["predict_ms"]
    res["checkpoint_bytes_per_trajectory"] = 8 * n_steps * D
    if not skip_host:
        host = lambda: _adj_ref.misfit_rk4(l96, _adj_ref.l96_vjp, _adj_ref.l96_pgrad, x0[0], K_TRUE, Y[0], Lidx, w, n_steps, DT)
        res["host_numpy_adjoint_ms_per_trajectory"], h = median_ms(host, reps)
        res["gx0_max_rel_diff"] = float(np.abs(h[1] - r["gx0"][0, 0]).max() / np.abs(h[1]).max())
        res["cost_rel_diff"] = float(abs(h[0] - r["cost"][0]) / h[0])
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--points", type=int, default=64)
    ap.add_argument("--steps", type=int, default=160)
    ap.add_argument("--skip-host", action="store_true")
    args = ap.parse_args()
    doc = dict(what="va_predict_adjoint in misfit mode (k_predict_adj: forward with checkpoints, backward sweep; transfers included) "
                    "against va_predict over the same steps and the NumPy adjoint on the host per trajectory, wall clock ms "
                    "(median of %d); no ratio is a threshold" % args.reps,
               runs=[run(args.points, 20, args.steps, args.reps, args.skip_host)], notes=[])
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")
