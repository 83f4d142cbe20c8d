"""Run tests/cpu_emul/hvp_check.cpp (TEST INFRASTRUCTURE): the phases of csrc/va_hvp.h thread by thread on the host."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DISC = {"euler": 0, "trapezoid": 1, "SimpsonHermite": 2, "forwardmap": 3}


def build_exe(path, user_header=None):
    cmd = ["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "varanneal_amd", "csrc"),
           "-o", path, os.path.join(ROOT, "tests", "cpu_emul", "hvp_check.cpp")]
    if user_header:
        cmd.insert(1, '-DVA_USER_RHS_HEADER="%s"' % user_header)
    subprocess.check_call(cmd)
    return path


def _nums(*arrays):
    return "\n".join(" ".join(repr(float(v)) for v in np.asarray(a, dtype=float).ravel()) for a in arrays if np.size(a)) + "\n"


def host_hv(exe, tmpdir, c, tile_rows=0, gn=0, X=None, V=None):
    """c: a case as tests/_hess_ref.py makes them.  Returns (HV [npts, nvec, n], (T, ntiles))."""
    X = c["X"] if X is None else X
    V = c["V"] if V is None else V
    npts, nvec, n = V.shape
    P = np.asarray(c["P"], float)                           # [NP], or [npts, NP]: every point its own
    P = np.broadcast_to(P, (npts, P.shape[-1]))
    stim, tm = c.get("stim"), c.get("t_model")
    nstim = 0 if stim is None else np.asarray(stim).reshape(c["N"], -1).shape[1]
    rm_arr, rf_arr = isinstance(c["RM"], np.ndarray), isinstance(c["RF0"], np.ndarray)
    head = [c["D"], c["N"], DISC[c["disc"]], c["nskip"], repr(c["dt"]), repr(c["rf_scale"]), gn, tile_rows, npts, nvec, P.shape[1],
            len(c["Pidx"]), nstim, int(tm is not None), len(c["Lidx"])] + list(c["Lidx"]) + list(c["Pidx"])
    txt = " ".join(str(v) for v in head) + "\n"
    txt += "%d\n" % rm_arr + _nums(c["RM"]) + "%d\n" % rf_arr + _nums(c["RF0"])
    txt += _nums(*([tm] if tm is not None else []) + ([stim] if nstim else []) + [X, P, V])
    f = os.path.join(str(tmpdir), "hvp_in.txt")
    with open(f, "w") as fh:
        fh.write(txt)
    out = subprocess.run([exe, "hv", f], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr)
    w = out.stdout.split()
    return np.array([float(v) for v in w[2:]]).reshape(npts, nvec, n), (int(w[0]), int(w[1]))


def fn_values(exe, tmpdir, D, NP, nstim, x, v, s, q, p, t, st):
    """the model's jvp [D], vjp2 [D] and summed pgrad2 [NP] at one point, from the host build of its header"""
    f = os.path.join(str(tmpdir), "hvp_fn.txt")
    with open(f, "w") as fh:
        fh.write("%d %d %d\n" % (D, NP, nstim) + _nums(x, v, s, q if NP else [0.0], p if NP else [0.0], [t], st if nstim else [0.0]))
    out = subprocess.run([exe, "fn", f], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr)
    w = np.array([float(u) for u in out.stdout.split()])
    return w[:D], w[D:2 * D], w[2 * D:]


def sympy_second_order(exprs, D, NP, nstim, x, v, s, q, p, t, st):
    """the same three from SymPy's Jacobians and Hessians of the traced expressions (no code of the generator's)"""
    import sympy as sp
    xs = sp.symbols("x0:%d" % D, real=True)
    ps = sp.symbols("p0:%d" % max(NP, 1), real=True)[:NP]
    ss = sp.symbols("st0:%d" % max(nstim, 1), real=True)[:nstim]
    z = list(xs) + list(ps)
    at = dict(zip(z, list(x) + list(p)))
    at.update(dict(zip(ss, st)))
    at[sp.Symbol("t", real=True)] = t
    w = np.concatenate([v, q])
    jvp, second = np.zeros(D), np.zeros(D + NP)
    for i, e in enumerate(exprs):
        g = [sp.diff(e, a) for a in z]
        jvp[i] = sum(float(g[k].subs(at)) * w[k] for k in range(D + NP) if g[k] != 0)
        for a in range(D + NP):
            if g[a] == 0:
                continue
            for b in range(D + NP):
                h = sp.diff(g[a], z[b])
                if h != 0:
                    second[b] += s[i] * float(h.subs(at)) * w[a]
    return jvp, second[:D], second[D:]
