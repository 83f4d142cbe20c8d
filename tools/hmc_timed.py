"""What a leapfrog step of the device sampler costs (va_hmc; csrc/va_hmc.h): 64 chains of the shipped example's shape
(Lorenz-96, D = 20, N = 161, one estimated parameter), beside the time of an evaluation on the same handle and beside the
NumPy chain (tests/_hmc_ref.py) driven by Problem.action_grad, which moves every path over PCIe twice per step.

    python tools/hmc_timed.py [--out profiles/hmc_timed.json] [--reps 7] [--iters 400] [--leap 10]
    python tools/hmc_timed.py --box     the box sampler's step (va_hmc_box, a box on every entry) beside va_hmc's, same handle

Like with like.  The sampler launches plainly, so the evaluation beside it is eval_timed with graph replay switched off
(eval_plain_us: HIP events around plain launches of the evaluation kernel alone); the sampler's step is the MARGINAL one,
(time of a call with n_leap steps per iteration - time with n_leap - 1) / iters, in which uploads, read-back, begin, end and
commit cancel: one element-wise launch and one evaluation, both as the host can issue them.  Beside them: eval_timed as
bench.py takes it (graph replay: what the device can do when the host is out of the way) and the whole call / steps with
everything in it.  A timed window is one hmc() call (--iters x --leap steps, tens of ms), wall clock, the median of --reps
after a warm-up call, with the smallest and largest beside it; the NumPy chain is warmed with one iteration and timed over
--numpy-iters.  No ratio is a threshold."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from varanneal_amd import _capi, twin      # noqa: E402


def timed_s(f, reps):
    f()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def box_main(args):
    """--box: the marginal leapfrog step (calls with n_leap and n_leap - 1 steps, difference / iters) of hmc_box with a
    two-sided box on every entry, beside the same measurement of hmc, same handle, same run, same step size"""
    D, N, B, rf = 20, 161, args.chains, 1.5 ** 10
    t, Y, _, Lidx = twin.make_twin(D, N)
    XP = np.empty((B, N * D + 1)); P = np.empty((B, 1))
    for b in range(B):
        X0, P0 = twin.initial_guess(N, D, b, Y, Lidx)
        XP[b, :-1] = X0.ravel(); XP[b, -1] = P0[0]; P[b] = P0
    bounds = [(-20.0, 20.0)] * (N * D) + [(0.5, 20.0)]
    XP = np.clip(XP, [b[0] + 0.5 for b in bounds], [b[1] - 0.5 for b in bounds])
    steps = args.iters * args.leap
    doc = dict(what="va_hmc_box with a two-sided box on every entry beside va_hmc on the same handle in the same run, us per leapfrog "
                    "step: marginal (calls with n_leap and n_leap - 1 steps per iteration, difference / iters) and whole call / steps, "
                    "wall clock, median [min, max]; no threshold",
               D=D, N=N, chains=B, n_var=N * D + 1, iters=args.iters, n_leap=args.leap, reps=args.reps, bounds="(-20, 20) states, (0.5, 20) parameter")
    with _capi.Problem(B, D, N, Y, Lidx, twin.DT, 4.0, 4e-6, P, [0], disc="trapezoid") as pb:
        doc["eval_kernel"] = pb.info()["eval_kernel"]
        runs = dict(hmc=lambda leap: pb.hmc(XP, rf, args.iters, leap, 0.02, jitter=0.1, seed=1),
                    hmc_box=lambda leap: pb.hmc_box(XP, rf, args.iters, leap, 0.02, bounds=bounds, jitter=0.1, seed=1))
        for name, run in runs.items():
            full, less = timed_s(lambda: run(args.leap), args.reps), timed_s(lambda: run(args.leap - 1), args.reps)
            doc[name + "_call_step_us"] = [1e6 * v / steps for v in full]
            doc[name + "_marginal_step_us"] = 1e6 * (full[0] - less[0]) / args.iters
            doc[name + "_call_ms"], doc[name + "_call_one_step_less_ms"] = [1e3 * v for v in full], [1e3 * v for v in less]
            doc[name + "_accept_rate"] = float(run(args.leap)["accepted"].mean())
    doc["box_marginal_over_hmc_marginal"] = doc["hmc_box_marginal_step_us"] / doc["hmc_marginal_step_us"]
    txt = json.dumps(doc, indent=1)
    print(txt)
    with open(args.out or os.path.join(ROOT, "profiles", "hmc_box_timed.json"), "w") as fh:
        fh.write(txt + "\n")
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--leap", type=int, default=10)
    ap.add_argument("--chains", type=int, default=64)
    ap.add_argument("--numpy-iters", type=int, default=10)
    ap.add_argument("--box", action="store_true", help="time va_hmc_box with a box on every entry beside va_hmc on the same handle "
                                                       "(default --out profiles/hmc_box_timed.json)")
    args = ap.parse_args()
    if args.box:
        sys.exit(box_main(args))
    import _hmc_ref
    D, N, B, rf = 20, 161, args.chains, 1.5 ** 10
    t, Y, _, Lidx = twin.make_twin(D, N)
    XP = np.empty((B, N * D + 1)); P = np.empty((B, 1))
    for b in range(B):
        X0, P0 = twin.initial_guess(N, D, b, Y, Lidx)
        XP[b, :-1] = X0.ravel(); XP[b, -1] = P0[0]; P[b] = P0
    steps = args.iters * args.leap
    doc = dict(what="va_hmc, us per leapfrog step: marginal (calls with n_leap and n_leap - 1 steps per iteration, difference / iters) and "
                    "whole call / steps, wall clock, median [min, max]; beside eval_timed on the same handle with plain launches and with "
                    "graph replay (HIP events), and the NumPy chain around Problem.action_grad; no threshold",
               D=D, N=N, chains=B, n_var=N * D + 1, iters=args.iters, n_leap=args.leap, reps=args.reps)
    with _capi.Problem(B, D, N, Y, Lidx, twin.DT, 4.0, 4e-6, P, [0], disc="trapezoid") as pb:
        doc["eval_kernel"] = pb.info()["eval_kernel"]
        pb.action_grad(XP, rf)
        ne = 2000
        for name, graph in (("eval_graph_us", 1), ("eval_plain_us", 0)):
            pb.tune(graph=graph)
            pb.eval_timed_prepare(rf, ne)
            pb.eval_timed(rf, ne)
            ms = [pb.eval_timed(rf, ne) for _ in range(args.reps)]
            doc[name] = [1e3 * float(v) / ne for v in (np.median(ms), np.min(ms), np.max(ms))]
        pb.tune(graph=1)
        run = lambda leap: pb.hmc(XP, rf, args.iters, leap, 0.5, jitter=0.1, seed=1)
        full, less = timed_s(lambda: run(args.leap), args.reps), timed_s(lambda: run(args.leap - 1), args.reps)
        doc["hmc_call_step_us"] = [1e6 * v / steps for v in full]
        doc["hmc_marginal_step_us"] = 1e6 * (full[0] - less[0]) / args.iters
        doc["hmc_call_ms"], doc["hmc_call_one_step_less_ms"] = [1e3 * v for v in full], [1e3 * v for v in less]
        doc["accept_rate"] = float(run(args.leap)["accepted"].mean())
        ni = args.numpy_iters
        noise = np.stack([np.stack([_hmc_ref.noise_row(1, b, it, N * D + 1) for b in range(B)]) for it in range(ni)])
        fg = lambda X: pb.action_grad(X, rf)[::3]
        _hmc_ref.chain(XP, fg, 0.5, 1, args.leap, noise[:1], jitter=0.1)
        t0 = time.perf_counter()
        _hmc_ref.chain(XP, fg, 0.5, ni, args.leap, noise, jitter=0.1)
        doc["numpy_chain_step_us"] = 1e6 * (time.perf_counter() - t0) / (ni * args.leap)
    doc["marginal_step_over_plain_eval"] = doc["hmc_marginal_step_us"] / doc["eval_plain_us"][0]
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(txt + "\n")
