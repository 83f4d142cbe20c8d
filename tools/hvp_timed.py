"""What the Hessian costs: va_hess_vec (k_hvp, csrc/va_hvp.h) on Lorenz-96 with the trapezoid rule, for the probing launch
that recovers the whole block-banded Hessian (3 D + 1 directions at one point, va_ode.Annealer.action_hessian) at the
shipped example's shape (D = 20, N = 161: 61 directions) and at D = 200, N = 1000 (601 directions).

    python tools/hvp_timed.py [--out profiles/hvp_timed.json] [--reps 5]

Times are wall clock around the whole call (uploads, the two kernels, the download, a device synchronise), the median of
--reps calls after a warm-up.  Beside them, as context and not as a threshold, the same NUMBER of va_action_grad
evaluations (one call on a handle of that many seeds), which is what a finite-difference Hessian would pay."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from varanneal_amd import _capi, twin      # noqa: E402


def one_shape(D, N, reps):
    t, Y, _, Lidx = twin.make_twin(D, N)
    X0, P0 = twin.initial_guess(N, D, 0, Y, Lidx)
    xp = np.append(X0.ravel(), P0[0])
    nvec = 3 * D + 1
    V = np.random.RandomState(D).randn(nvec, xp.size)
    res = dict(D=D, N=N, directions=nvec, disc="trapezoid")
    with _capi.Problem(1, D, N, Y, Lidx, twin.DT, 4.0, 4e-6, np.array([P0]), [0], disc="trapezoid") as pb:
        for gn in (False, True):
            pb.hess_vec(xp[None, :], V, 50.0, gauss_newton=gn)
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                out = pb.hess_vec(xp[None, :], V, 50.0, gauss_newton=gn)
                ts.append(time.perf_counter() - t0)
            res["hess_vec_ms" + ("_gauss_newton" if gn else "")] = 1e3 * float(np.median(ts))
        res["finite"] = bool(np.all(np.isfinite(out)))
    XB = np.repeat(xp[None, :], nvec, axis=0) + 1e-3 * V
    with _capi.Problem(nvec, D, N, Y, Lidx, twin.DT, 4.0, 4e-6, np.repeat(np.array([P0]), nvec, axis=0), [0], disc="trapezoid") as pb:
        pb.action_grad(XB, 50.0)
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            pb.action_grad(XB, 50.0)
            ts.append(time.perf_counter() - t0)
        res["action_grad_same_count_ms"] = 1e3 * float(np.median(ts))
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    doc = dict(what="va_hess_vec wall clock per call (median): the probing launch of action_hessian; action_grad_same_count_ms "
                    "is context, not a threshold",
               shapes=[one_shape(20, 161, args.reps), one_shape(200, 1000, args.reps)])
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")
