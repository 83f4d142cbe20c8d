"""What a Lyapunov spectrum costs: va_lyapunov (k_lyap, csrc/va_lyap.h) on 64 points of the shipped example's shape (Lorenz-96,
D = 20), the whole spectrum (K = 20) over a few thousand steps, with the QR every 1 / 4 / 16 steps -- the differences are the
QR's share -- against the tangent work alone (va_predict_tangent with 20 directions over the same steps: no QR, the
directions of a trajectory spread over independent workgroups) and against Benettin's method in NumPy on the host
(tests/_lyap_ref.py) from the same inputs.

    python tools/lyap_timed.py [--out profiles/lyap_timed.json] [--reps 3] [--steps 4000] [--host-points 2]

Wall clock around the whole call, transfers included, the median of --reps calls after a warm-up.  The host reference runs
--host-points of the trajectories (it takes about a second each) and is reported per trajectory.  No ratio is a threshold."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _lyap_ref import lyap_ref                                    # noqa: E402
from _predict_ref import DT, K_TRUE, attractor_starts, l96        # noqa: E402
from _tlm_ref import l96_jvp                                      # noqa: E402
from varanneal_amd import _capi                                   # noqa: E402


def median_ms(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = f()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts)), out


def run(T, n_steps, reps, host_points):
    D = K = 20
    x0 = attractor_starts(D, T)
    p = np.full((T, 1), K_TRUE)
    Lidx = list(range(0, D, 2))
    gain = np.zeros(D)
    gain[Lidx] = 5.0
    res = dict(D=D, K=K, points=T, n_steps=n_steps, dt=DT)
    with _capi.Problem(1, D, 5, np.zeros((5, len(Lidx))), Lidx, DT, 4.0, 1e-2, np.array([[K_TRUE]]), [0]) as pb:
        for q in (1, 4, 16):
            ms, r = median_ms(lambda: pb.lyapunov(x0, p, K, n_steps, qr_every=q), reps)
            res["lyapunov_qr%d_ms" % q] = ms
            res["lyapunov_qr%d_us_per_step" % q] = 1e3 * ms / n_steps
            if q == 4:
                r4 = r
        res["lyapunov_qr4_gain_ms"], rg = median_ms(lambda: pb.lyapunov(x0, p, K, n_steps, qr_every=4, coupling=gain), reps)
        res["lyapunov_qr4_k1_ms"], _ = median_ms(lambda: pb.lyapunov(x0, p, 1, n_steps, qr_every=4), reps)
        # the QR's share of a QR interval of 4 steps, from the calls that differ in nothing else
        per_qr = (res["lyapunov_qr1_ms"] - res["lyapunov_qr16_ms"]) / (n_steps - n_steps / 16.0)
        res["qr_us_each"] = 1e3 * per_qr
        res["qr_share_at_qr4"] = per_qr * (n_steps / 4.0) / res["lyapunov_qr4_ms"]
        V0 = np.zeros((T, K, D + 1))
        V0[:, :, :D] = np.eye(K, D)
        res["predict_tangent_20dir_ms"], _ = median_ms(lambda: pb.predict_tangent(x0, p, V0, n_steps, every=n_steps, want=("dx",)), reps)
    lam = r4["exponents"]
    res["status_ok"] = int((r4["status"] == 0).sum())
    res["lambda1_mean"], res["lambda1_std"] = float(lam[:, 0].mean()), float(lam[:, 0].std())
    res["sum_mean"] = float(lam.sum(axis=1).mean())
    res["lambda1_conditional_gain5_mean"] = float(rg["exponents"][:, 0].mean())
    if host_points > 0:
        t0 = time.perf_counter()
        hs = [lyap_ref(l96, l96_jvp, x0[i], K_TRUE, K, n_steps, DT, qr_every=4) for i in range(host_points)]
        res["host_numpy_ms_per_trajectory"] = 1e3 * (time.perf_counter() - t0) / host_points
        res["host_points"] = host_points
        # (chaotic over thousands of steps: the two agree as finite-time averages do, not to rounding)
        res["lambda1_host_minus_device"] = [float(h["logsum"][0] / (n_steps * DT) - lam[i, 0]) for i, h in enumerate(hs)]
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--points", type=int, default=64)
    ap.add_argument("--steps", type=int, default=4000)
    ap.add_argument("--host-points", type=int, default=2)
    args = ap.parse_args()
    doc = dict(what="va_lyapunov (k_lyap: tangent-linear RK4 and Gram-Schmidt QR on device, transfers included) at qr_every = 1 / 4 / 16, "
                    "va_predict_tangent with as many directions over the same steps (no QR), and Benettin's method in NumPy on the "
                    "host per trajectory; wall clock ms (median); no ratio is a threshold",
               runs=[run(args.points, args.steps, args.reps, args.host_points)], notes=[])
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")
