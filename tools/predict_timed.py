"""What the forecast costs: va_predict (k_predict, csrc/va_predict.h) on Lorenz-96 for the two shapes a ladder leaves
behind -- T = 1920 trajectories (64 seeds x 30 rungs) of D = 20, and T = 64 of D = 200 -- 1000 steps each.

    python tools/predict_timed.py [--out profiles/predict_timed.json] [--steps 1000] [--reps 5]

Times are wall clock around the whole call (uploads, the kernel, the download of the output, a device synchronise), the
median of --reps calls after a warm-up: once keeping every step (the output is T x 1001 x D doubles) and once keeping the
last step only, which is close to the kernel alone.  Beside them, as context and not as a threshold, the same job as a
NumPy RK4 vectorised over the trajectories on the host, and the largest difference between the two end states."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from varanneal_amd import _capi, twin      # noqa: E402


def numpy_rk4(x, k, steps, dt):
    f = lambda x: np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - x + k
    for _ in range(steps):
        k1 = f(x); k2 = f(x + 0.5 * dt * k1); k3 = f(x + 0.5 * dt * k2); k4 = f(x + dt * k3)
        x = x + dt / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
    return x


def one_shape(T, D, steps, reps):
    rng = np.random.RandomState(T + D)
    base = twin.integrate_l96(D, 1, spinup=400)[0]
    x0 = base[None, :] + 0.05 * rng.randn(T, D)
    k = twin.K_TRUE + 0.1 * rng.randn(T, 1)
    Lidx = twin.default_lidx(D)
    res = dict(T=T, D=D, steps=steps, dt=twin.DT)
    with _capi.Problem(1, D, 5, np.zeros((5, len(Lidx))), Lidx, twin.DT, 4.0, 1e-2, k[:1], [0]) as pb:
        for name, every in (("all_steps", 1), ("last_step", steps)):
            pb.predict(x0, k, steps, every=every)                   # warm-up: code object, allocator
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                out = pb.predict(x0, k, steps, every=every)
                ts.append(time.perf_counter() - t0)
            res["device_ms_" + name] = 1e3 * float(np.median(ts))
            res["device_ms_%s_min_max" % name] = [1e3 * min(ts), 1e3 * max(ts)]
        short = pb.predict(x0, k, 40, every=40)[:, -1]
    t0 = time.perf_counter()
    numpy_rk4(x0, k, steps, twin.DT)
    res["numpy_host_ms"] = 1e3 * (time.perf_counter() - t0)
    # (40 steps: beyond that the chaotic system amplifies rounding and the two runs part, as any two orderings do)
    res["max_abs_diff_after_40_steps"] = float(np.abs(short - numpy_rk4(x0, k, 40, twin.DT)).max())
    res["us_per_substep_last_step"] = 1e3 * res["device_ms_last_step"] / steps
    res["finite"] = bool(np.all(np.isfinite(out)))
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    doc = dict(what="va_predict wall clock per call (median), Lorenz-96, RK4 substeps=1; numpy_host_ms is context, not a threshold",
               shapes=[one_shape(1920, 20, args.steps, args.reps), one_shape(64, 200, args.steps, args.reps)])
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")
