"""CPU: the column-parameter form of a generated model (codegen.colparam_form: shared scalars + per-column parameter
vectors, e.g. a forcing per site) -- recognition, tracing past the flat kernel's 128 parameters, the generated
kernels cross-compiled for gfx950, and the Annealer's route for the built-in model called with a parameter vector."""
import os
import shutil

import numpy as np
import pytest

from varanneal_amd import _capi, codegen, va_ode


def l96(t, x, k):
    """examples/Lorenz96_D20/Lorenz96_anneal.py:15-16 (the reference takes any k: a scalar or one per site)"""
    return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - x + k


def forcing_damping(t, x, p):
    """a copy of tests/test_codegen.py's _many_parameters: forcing p[:D], damping p[D:2D]"""
    D = x.shape[1]
    return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - p[D:2 * D] * x + p[:D]


def shared_and_vectors(t, x, p):
    D = x.shape[1]
    return p[0] * np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - p[1] * x + p[2:2 + D] * np.tanh(p[2 + D:2 + 2 * D])


def interleaved(t, x, p):
    D = x.shape[1]
    return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - p[1:2 * D:2] * x + p[0:2 * D:2]


def _form(f, D, NP):
    exprs, syms = codegen.trace(f, D, NP)
    return codegen.colparam_form(exprs, syms, D, NP)


@pytest.mark.parametrize("f,NP,S,V,sidx,vidx0", [
    (l96, 20, 0, 1, [], [[0, 1, 2]]),
    (forcing_damping, 40, 0, 2, [], [[0, 1, 2], [20, 21, 22]]),
    (shared_and_vectors, 42, 2, 2, [0, 1], [[2, 3, 4], [22, 23, 24]]),
    (interleaved, 40, 0, 2, [], [[0, 2, 4], [1, 3, 5]]),
])
def test_recognised(f, NP, S, V, sidx, vidx0):
    D = 20
    cp = _form(f, D, NP)
    assert cp is not None and cp["S"] == S and cp["V"] == V and list(cp["sidx"]) == sidx
    assert cp["vidx"].shape == (V, D) and cp["vidx"][:, :3].tolist() == vidx0
    # every parameter is exactly one shared scalar or one vector entry
    assert sorted(list(cp["sidx"]) + list(np.ravel(cp["vidx"]))) == list(range(NP))
    exprs, syms = codegen.trace(f, D, NP)
    colp = codegen.column_form(exprs, syms, D, NP, 0, cp=cp)
    assert colp is not None and "struct RhsUserColP" in colp["text"] and "NCV = %d" % V in colp["text"]
    assert colp["offsets"] == [-2, -1, 1]


def neighbour_forcing(t, x, k):
    return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - x + np.roll(k, 1)      # f_i uses k[i-1]


def two_columns(t, x, p):
    D = x.shape[1]
    k = np.append(p[:D - 1], p[D - 2])                                                    # p[D-2] in columns D-2 and D-1
    return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - x + k


def partial_vector(t, x, p):
    D = x.shape[1]
    k = np.append(p[:D - 1], 0.0)                                                         # D-1 entries for D columns
    return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - x + k


@pytest.mark.parametrize("f,NP", [(neighbour_forcing, 20), (two_columns, 19), (partial_vector, 19)])
def test_not_recognised(f, NP):
    assert _form(f, 20, NP) is None


def test_forty_parameters_keep_their_form():
    """without colparams the 40-parameter model generates what it did before (no column form, no colp)"""
    m = codegen.module_for(forcing_damping, 20, 40, compile=False,
                           col_variant=lambda ne, gh: (4, 1, 7, 1) if ne else None)
    assert m["col"] is None and m["ghost"] is None and m["colp"] is None
    m = codegen.module_for(forcing_damping, 20, 40, compile=False, colparams=True,
                           col_variant=lambda ne, gh: (4, 1, 7, 1) if ne else None)
    assert m["col"] is None and m["colp"] is not None and m["col_variant"] == (4, 1, 7, 1)
    assert "#define VA_USER_COLP 1" in m["text"] and "acc[39] +=" in m["text"]       # (and the flat struct, NP <= 128)


def test_trace_past_the_old_cap():
    """D = 200 with 400 parameters (forcing + damping per site) traces and generates; the flat struct is a stub"""
    m = codegen.module_for(forcing_damping, 200, 400, compile=False)
    assert m["colp"] is not None and m["colp"]["V"] == 2 and m["colp"]["S"] == 0
    assert "static constexpr bool FLAT = false;" in m["text"]
    assert "static const int va_colp_vidx[400]" in m["text"]


def test_past_the_cap_without_the_form_is_refused():
    def coupled(t, x, p):                   # every parameter in two columns: no column-parameter form
        D = x.shape[1]
        return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - x + p[:D] + np.roll(p[:D], 1)
    with pytest.raises(NotImplementedError, match="more than 128 parameters"):
        codegen.module_for(coupled, 200, 200, compile=False)


@pytest.mark.skipif(shutil.which(codegen.HIPCC) is None and not os.path.exists(codegen.HIPCC), reason="needs hipcc")
@pytest.mark.parametrize("D,variant", [(20, (4, 1, 7, 1)), (200, (5, 1, 0, 0))])
def test_cross_compiles(D, variant, tmp_path, monkeypatch):
    """the generated header with k_eval4 (D = 20) / k_eval5 (D = 200, no flat kernel) compiled for gfx950"""
    monkeypatch.setattr(codegen, "CACHE", str(tmp_path))
    m = codegen.module_for(l96, D, D, colparams=True, col_variant=lambda ne, gh, reach=None: variant)
    assert m["col_variant"] == variant and os.path.getsize(m["so"]) > 0


class _Recorder(object):
    """device stand-in: records what the Annealer hands to the device layer, answers with zeros of the right shapes"""
    made = []

    def __init__(self, batch, D, N_model, Y, Lidx, dt_model, RM, RF0, P, Pidx, **kw):
        self.B, self.D, self.N, self.NPest = batch, D, N_model, len(Pidx)
        self.P, self.kw = np.array(P), kw
        _Recorder.made.append(self)

    def close(self):
        pass

    def anneal(self, XP, rf_scale, opt_args=None, want_paths=False, **kw):
        B, nb = self.B, len(rf_scale)
        z = np.zeros((B, nb))
        mp = np.zeros((B, nb, self.N * self.D + self.P.shape[-1]))
        return dict(x=None, A=z, me=z, fe=z, status=np.zeros((B, nb), np.int32), nit=np.zeros((B, nb), np.int32),
                    nfev=np.zeros((B, nb), np.int64), minpaths=mp, pest=np.zeros((B, nb, self.NPest)))


def test_builtin_model_with_a_parameter_vector_goes_to_codegen(monkeypatch):
    calls = []

    def fake_module_for(f, D, NP, *a, **kw):
        calls.append((f, D, NP, kw))
        return dict(so="/nonexistent/libva_rhs_test.so")
    monkeypatch.setattr(codegen, "module_for", fake_module_for)
    monkeypatch.setattr(_capi, "load_rhs_module", lambda path: 1000)
    monkeypatch.setattr(_capi, "Problem", _Recorder)
    _Recorder.made = []
    D, N = 20, 11
    rng = np.random.RandomState(1)
    a = va_ode.Annealer()
    a.set_model(l96, D)
    a.set_data(rng.randn(N, D // 2), t=0.025 * np.arange(N))
    a.anneal(rng.randn(N, D), np.full(D, 8.0), 2.0, [0, 1], 4.0, 1e-2, list(range(0, D, 2)), list(range(D)),
             disc="trapezoid", verbose=False)
    assert len(calls) == 1
    f, Dm, NPm, kw = calls[0]
    assert f is l96 and (Dm, NPm) == (D, D) and kw["colparams"] is True
    assert _Recorder.made[-1].kw["rhs"] == 1000 and _Recorder.made[-1].P.shape[-1] == D
    # the built-in model with its one parameter keeps the built-in kernels
    calls.clear()
    b = va_ode.Annealer()
    b.set_model(l96, D)
    b.set_data(rng.randn(N, D // 2), t=0.025 * np.arange(N))
    b.anneal(rng.randn(N, D), np.array([8.0]), 2.0, [0], 4.0, 1e-2, list(range(0, D, 2)), [0], disc="trapezoid",
             verbose=False)
    assert calls == [] and _Recorder.made[-1].kw["rhs"] == "lorenz96"


def test_recognised_at_the_limits():
    """24 shared scalars (RHS_MAX_NP: the 32-column partial sums) and 4 vectors (CP_VMAX), interleaved, are recognised;
    one more scalar or one more vector is not -- and each of those models has the form bar the cap"""
    from _util import colparam_model
    D = 20
    cp = _form(colparam_model(24, 4, interleaved=True), D, 24 + 4 * D)
    assert cp is not None and cp["S"] == 24 and cp["V"] == 4 and list(cp["sidx"]) == list(range(24))
    assert cp["vidx"][:, :2].tolist() == [[24, 28], [25, 29], [26, 30], [27, 31]]
    for S, V in ((25, 1), (0, 5)):
        NP = S + V * D
        assert _form(colparam_model(S, V), D, NP) is None, (S, V)
        exprs, syms = codegen.trace(colparam_model(S, V), D, NP)
        cp = codegen.colparam_form(exprs, syms, D, NP, max_ncv=5, max_shared=25)
        assert cp is not None and (cp["S"], cp["V"]) == (S, V)


@pytest.mark.parametrize("S,V", [(25, 1), (0, 5)])
def test_past_the_limits_and_the_cap_is_refused(S, V):
    """D = 200: 225 / 1000 parameters, past the flat kernel's 128, one scalar / one vector more than the form takes"""
    from _util import colparam_model
    with pytest.raises(NotImplementedError, match="more than 128 parameters"):
        codegen.module_for(colparam_model(S, V), 200, S + V * 200, compile=False)
