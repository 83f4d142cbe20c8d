"""Shared helpers for the test-suite (golden loading, oracle construction)."""
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_npz_cases(fname):
    z = np.load(os.path.join(GOLD, fname), allow_pickle=False)
    cases = {}
    for key in z.files:
        c, k = key.split("/", 1)
        v = z[key]
        cases.setdefault(c, {})[k] = v.item() if v.ndim == 0 else v
    return cases


def rm_rf_for(case):
    """Expand the golden case's RM/RF0 (scalar | (L,) | (D,)) the way
    va_ode.py:612-640 does (np.resize over time)."""
    N, D = int(case["N_model"]), int(case["D"])
    Y = case["Y"]
    RM, RF0 = case["RM"], case["RF0"]
    RM = float(RM) if np.ndim(RM) == 0 else np.resize(RM, Y.shape)
    RF0 = float(RF0) if np.ndim(RF0) == 0 else np.resize(RF0, (N - 1, D))
    return RM, RF0


def oracle_problem(case):
    import va_oracle
    N, D = int(case["N_model"]), int(case["D"])
    RM, RF0 = rm_rf_for(case)
    P = case["XP"][N * D:]
    return va_oracle.Problem(D, N, case["Y"], case["Lidx"], case["dt_model"], RM, RF0, P, [0],
                             disc=str(case["disc"]), merr_nskip=int(case["merr_nskip"]))


def colparam_model(S, V, interleaved=False, driven=False):
    """A Lorenz-96 family in column-parameter form (codegen.colparam_form): S shared scalars p[0:S] (scalar j couples
    the neighbour x_{i+o_j} with its own weight, so that no two scalars have proportional gradients) and V per-site
    vectors after them -- as blocks p[S + vD + i] or interleaved p[S + Vi + v] -- entering f_i as a forcing F_i, a
    damping -g_i x_i, a coupling h_i x_{i-1}, a quadratic k_i x_i^2 and a coupling x_{i+1} (v = 0 ... 4; five is one more than
    the form takes).  driven: the forcing is
    modulated by the model time, F_i (1 + sin t / 2), a non-autonomous model."""
    offs = (-1, 1, 2)

    def f(t, x, p):
        D = x.shape[1]
        out = np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - x
        for j in range(S):
            out = out + (0.01 * (j + 1)) * p[j] * np.roll(x, offs[j % 3], 1)
        vec = [p[S + v:S + V * D:V] if interleaved else p[S + v * D:S + (v + 1) * D] for v in range(V)]
        terms = [lambda: (1.0 + 0.5 * np.sin(t))[:, None] if driven else 1.0, lambda: -x,
                 lambda: 0.1 * np.roll(x, 1, 1), lambda: 0.05 * x * x, lambda: 0.1 * np.roll(x, -1, 1)]
        for v in range(V):
            out = out + vec[v] * terms[v]()
        return out
    f.__name__ = "colparam_s%d_v%d%s%s" % (S, V, "_il" if interleaved else "", "_t" if driven else "")
    return f
