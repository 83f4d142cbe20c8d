"""usage: python tools/colparams_timed.py [OUT.json]  -- the column-parameter form (a Lorenz-96 forcing per site) against
what it replaces, per evaluation (va_eval_timed: replayed launches of (A, grad A), no line search), two repetitions:

  c4   D = 200, N = 5000, 64 seeds, trapezoid: l96 with P0 of length 200 (k_eval5, generated module) against the built-in
       scalar-forcing Lorenz-96 on the same shape and flags (k_eval5, library).  Target: <= 1.15 x.
  d20  D = 20, N = 1000, 64 seeds: the same model forced onto k_eval4 against the flat kernel.  Target: >= 2 x faster.

Prints one line per case and a JSON summary (written to OUT.json when given)."""
import json
import sys

import numpy as np

sys.path.insert(0, '.')
import bench
from varanneal_amd import _capi, codegen, twin


def l96(t, x, k):
    return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - x + k


def timed(pb, XP, iters):
    pb.action_grad(XP, 1.0)
    pb.eval_timed_prepare(1.0, iters)
    pb.eval_timed(1.0, iters)
    return [1e3 * pb.eval_timed(1.0, iters) / iters for _ in range(2)]       # us per evaluation


def run(D, N, B, iters, base, colp_kernel):
    Y, Lidx, XP1, P1 = bench.make_inputs(D, N, B, 0)
    ND = N * D
    P = np.tile(P1[:, :1], (1, D)) + 0.01 * np.arange(D)[None, :]
    XP = np.concatenate([XP1[:, :ND], P], axis=1)
    Pidx = list(range(D))
    m = codegen.module_for(l96, D, D, colparams=True,
                           col_variant=lambda ne, gh, reach=None: _capi.eval_plan(B, D, N, "trapezoid", ne, gh,
                                                                                eval_kernel=colp_kernel, reach=reach, Lidx=Lidx))
    with _capi.Problem(B, D, N, Y, Lidx, twin.DT, 4.0, 4e-6, P, Pidx, disc="trapezoid", eval_kernel=colp_kernel,
                       rhs=_capi.load_rhs_module(m["so"])) as pb:
        ek = pb.info()["eval_kernel"]
        t_new = timed(pb, XP, iters)
    if base == "builtin":
        with _capi.Problem(B, D, N, Y, Lidx, twin.DT, 4.0, 4e-6, P1, [0], disc="trapezoid") as pb:
            ek0 = pb.info()["eval_kernel"]
            t_old = timed(pb, XP1, iters)
    else:
        flat = codegen.module_for(l96, D, D)
        with _capi.Problem(B, D, N, Y, Lidx, twin.DT, 4.0, 4e-6, P, Pidx, disc="trapezoid", eval_kernel=1,
                           rhs=_capi.load_rhs_module(flat["so"])) as pb:
            ek0 = pb.info()["eval_kernel"]
            t_old = timed(pb, XP, iters)
    return dict(D=D, N=N, B=B, iters=iters, colp_kernel=ek, colp_us=t_new, base=base, base_kernel=ek0, base_us=t_old,
                ratio=min(t_new) / min(t_old))


def main():
    res = {"c4": run(200, 5000, 64, 50, "builtin", 0), "d20": run(20, 1000, 64, 200, "flat", 4)}
    c4, d20 = res["c4"], res["d20"]
    c4["target"], c4["met"] = "colp / scalar <= 1.15", c4["ratio"] <= 1.15
    d20["target"], d20["met"] = "flat / k_eval4 >= 2", 1.0 / d20["ratio"] >= 2.0
    print("c4:  per-site forcing on k_eval%d %.1f us, scalar forcing on k_eval%d %.1f us: %.3f x (target <= 1.15)"
          % (c4["colp_kernel"], min(c4["colp_us"]), c4["base_kernel"], min(c4["base_us"]), c4["ratio"]))
    print("d20: k_eval%d %.1f us, flat kernel %.1f us: %.2f x faster (target >= 2)"
          % (d20["colp_kernel"], min(d20["colp_us"]), min(d20["base_us"]), 1.0 / d20["ratio"]))
    print(json.dumps(res))
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
