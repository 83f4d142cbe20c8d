"""What tracking costs: va_enkf (k_enkf, csrc/va_enkf.h) on 64 points of the shipped example's shape (Lorenz-96, D = 20, every
second column observed), 32 members each, over a few thousand model steps, with an observation row every 2 and every 8 steps
-- the calls differ in the number of analyses and in nothing else, which separates the cost of an analysis from that of a
model step as tools/lyap_timed.py separates the QR -- against the same filter in NumPy on the host (tests/_enkf_ref.py) from
the same inputs.

    python tools/enkf_timed.py [--out profiles/enkf_timed.json] [--reps 3] [--steps 4000] [--host-points 1]

Wall clock around the whole call, transfers included, the median of --reps calls after a warm-up.  The host reference runs
--host-points of the points and is reported per point.  No ratio is a threshold."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _enkf_ref import enkf_ref, l96_rows                          # noqa: E402
from _predict_ref import DT, K_TRUE, attractor_starts, l96, rk4   # noqa: E402
from varanneal_amd import _capi                                   # noqa: E402


def median_ms(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), out


def run(T, M, n_steps, reps, host_points):
    D, ov, infl = 20, 0.25, 1.05
    rng = np.random.RandomState(3)
    nt = min(T, 4)                                                 # (distinct truths; an rk4 run of thousands of steps on the host each)
    which = np.arange(T) % nt
    starts = attractor_starts(D, nt)
    Lidx = list(range(0, D, 2))
    x0 = starts[which][:, None, :] + 0.5 * rng.randn(T, M, D)
    p = K_TRUE + 0.2 * rng.randn(T, M, 1)
    res = dict(D=D, members=M, points=T, n_steps=n_steps, dt=DT, L=len(Lidx), obs_var=ov, inflation=infl)
    Ys = {}
    with _capi.Problem(1, D, 5, np.zeros((5, len(Lidx))), Lidx, DT, 4.0, 1e-2, np.array([[K_TRUE]]), [0]) as pb:
        for oe in (2, 8):
            n_obs = n_steps // oe
            # (the data: the point's truth plus noise of its own)
            truth = np.array([rk4(l96, starts[i], K_TRUE, n_steps, DT, every=oe)[1:] for i in range(nt)])
            Y = truth[which][:, :, Lidx] + np.sqrt(ov) * rng.randn(T, n_obs, len(Lidx))
            Ys[oe] = Y
            ms, r = median_ms(lambda: pb.enkf(x0, p, Y, ov, obs_every=oe, est=[0], inflation=infl), reps)
            res["enkf_every%d_ms" % oe] = ms
            res["enkf_every%d_status_ok" % oe] = int((r["status"] == 0).sum())
            res["enkf_every%d_rms_innovation_last" % oe] = float(np.sqrt(np.nanmean((Y[:, -1] - r["mean_f"][:, -1][:, Lidx]) ** 2)))
        # n_steps model steps in both calls; n_steps / 2 against n_steps / 8 analyses of len(Lidx) observations each
        per_analysis = (res["enkf_every2_ms"] - res["enkf_every8_ms"]) / (n_steps / 2.0 - n_steps / 8.0)
        res["analysis_us_each"] = 1e3 * per_analysis
        res["model_step_us_each"] = 1e3 * (res["enkf_every8_ms"] - per_analysis * n_steps / 8.0) / n_steps
        res["analysis_share_at_every2"] = per_analysis * (n_steps / 2.0) / res["enkf_every2_ms"]
        res["predict_members_ms"], _ = median_ms(lambda: pb.predict(x0.reshape(-1, D), p.reshape(-1, 1), n_steps, every=n_steps), reps)
    if host_points > 0:
        Y = Ys[2]
        t0 = time.perf_counter()
        for i in range(host_points):
            enkf_ref(l96_rows, x0[i], p[i], [0], Y[i], Lidx, np.full(len(Lidx), ov), DT, obs_every=2, inflation=infl, batched=True)
        res["host_numpy_ms_per_point_every2"] = 1e3 * (time.perf_counter() - t0) / host_points
        res["host_points"] = host_points
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--points", type=int, default=64)
    ap.add_argument("--members", type=int, default=32)
    ap.add_argument("--steps", type=int, default=4000)
    ap.add_argument("--host-points", type=int, default=1)
    args = ap.parse_args()
    doc = dict(what="va_enkf (k_enkf: RK4 forecast of every member and serial square-root analysis on device, transfers included) with an "
                    "observation row every 2 and every 8 model steps, va_predict of the same members over the same steps (no analysis), "
                    "and the same filter in NumPy on the host per point; wall clock ms (median); no ratio is a threshold",
               runs=[run(args.points, args.members, args.steps, args.reps, args.host_points)], notes=[])
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")
