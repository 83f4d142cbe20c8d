"""CPU: the ladder bookkeeping of both drop-ins (va_ode.Annealer, va_nnet.Annealer) and the ADmin
surface, against a backend that only logs its calls and answers with canned numbers.

No oracle and no library: `_capi.Problem` / `_capi.NnetProblem` are replaced by `FakeBackend`.  Every
number it returns is a small integer or a dyadic fraction of (rung counter, seed index), and every
input is one too, so all arithmetic on the way into the result tables is exact in float64: expected
tables are worked out here rung by rung and compared with np.array_equal, printed text and saved
files included."""
import re

import numpy as np
import pytest

from varanneal_amd import _capi, va_nnet, va_ode

OPTS = {"maxiter": 7, "maxcor": 5}
NBETA = 4
ALPHA = 2


def canned(r, b):
    """what the backend answers for the r-th rung it minimises (1-based, over its life) and seed b;
    the minimiser it pretends to find is x -> x / 2 + shift"""
    me, fe = r + 0.125 * b, 2.0 * r + 0.5 * b
    return dict(shift=r + 0.25 * b, A=me + fe, me=me, fe=fe, status=(r + b) % 3, nit=10 * r + b, nfev=20 * r + b + 1)


def eval_canned(XP, rf):
    """the backend's (A, me, fe, grad) at XP"""
    A = XP.sum(axis=1) + rf
    return A, 0.25 * A, 0.75 * A, 2.0 * XP + rf


class FakeBackend(object):
    """Stand-in for _capi.Problem / _capi.NnetProblem: the three entry points, logged."""

    def _setup(self, batch, nx, P, estpos, full_rows, kw):
        self.B, self.nx, self.estpos = batch, nx, list(estpos)
        self.P = np.array(P, dtype=np.float64).reshape(batch, -1)
        self.n_var = nx + len(self.estpos)
        self.full_rows = full_rows                   # anneal() answers [X | P] rows, not [X | p_est]
        self.created = kw
        self.log, self.rungs, self.closed = [], 0, False

    def close(self):
        self.closed = True

    def action_grad(self, XP, rf_scale=1.0, want_grad=True):
        assert XP.shape == (self.B, self.n_var)
        self.log.append(("action_grad", np.array(XP), float(rf_scale), want_grad))
        A, me, fe, g = eval_canned(np.asarray(XP), rf_scale)
        return A, me, fe, (g if want_grad else None)

    def _rung(self, x):
        self.rungs += 1
        c = [canned(self.rungs, b) for b in range(self.B)]
        x = np.array([0.5 * x[b] + c[b]["shift"] for b in range(self.B)])
        return x, {k: np.array([cb[k] for cb in c]) for k in ("A", "me", "fe", "status", "nit", "nfev")}

    def minimize_lbfgs(self, XP, rf_scale, opt_args=None):
        assert XP.shape == (self.B, self.n_var)
        self.log.append(("minimize_lbfgs", np.array(XP), float(rf_scale), opt_args))
        x, r = self._rung(XP)
        self.P[:, self.estpos] = x[:, self.nx:]
        return dict(r, x=x)

    def anneal(self, XP, rf_scale, opt_args=None, want_paths=False):
        assert XP.shape == (self.B, self.n_var)
        self.log.append(("anneal", np.array(XP), np.array(rf_scale), opt_args, want_paths))
        x, rows, tabs = np.array(XP), [], []
        for _ in rf_scale:
            x, r = self._rung(x)
            self.P[:, self.estpos] = x[:, self.nx:]
            rows.append(np.concatenate([x[:, :self.nx], self.P], axis=1) if self.full_rows else x)
            tabs.append(r)
        out = {k: np.stack([t[k] for t in tabs], axis=1) for k in tabs[0]}
        return dict(out, x=None, pest=None, minpaths=np.stack(rows, axis=1) if want_paths else None)


class FakeOde(FakeBackend):
    def __init__(self, batch, D, N_model, Y, Lidx, dt_model, RM, RF0, P, Pidx, p_time_dependent=False, **kw):
        NP = np.shape(P)[-1]
        estpos = [n * NP + k for n in range(N_model) for k in Pidx] if p_time_dependent else list(Pidx)
        self._setup(batch, N_model * D, P, estpos, not p_time_dependent, dict(kw, p_time_dependent=p_time_dependent))


class FakeNnet(FakeBackend):
    def __init__(self, batch, structure, data_in, data_out, Lidx, RM, RF0, P, Pidx, **kw):
        self._setup(batch, int(np.sum(structure)) * np.shape(data_in)[0], P, Pidx, False, kw)


@pytest.fixture
def fake(monkeypatch):
    from varanneal_amd import codegen
    monkeypatch.setattr(_capi, "Problem", FakeOde)
    monkeypatch.setattr(_capi, "NnetProblem", FakeNnet)
    # the ODE model below is no built-in: its module would be generated and compiled
    monkeypatch.setattr(codegen, "module_for", lambda *a, **k: {"so": "generated.so"})
    monkeypatch.setattr(_capi, "load_rhs_module", lambda path: 1000)


class Minimize(object):
    """recorder in the place of scipy.optimize.minimize"""

    def __init__(self):
        self.calls = []

    def __call__(self, fun, x0, **kw):
        import scipy.optimize as opt
        self.calls.append((np.array(x0), kw))
        n = len(self.calls)
        f, g = fun(x0)
        return opt.OptimizeResult(x=0.5 * x0 + n, fun=f + n, status=n % 3, nit=3 * n, nfev=5 * n, message="stopped %d" % n)


@pytest.fixture
def minimize(monkeypatch):
    import scipy.optimize as opt
    m = Minimize()
    monkeypatch.setattr(opt, "minimize", m)
    return m


# ---------------------------------------------------------------------------------- expectations
class Expected(object):
    """The result tables of a ladder on the canned backend, worked out rung by rung."""

    def __init__(self, Xf, Pf, estpos, batched, results=None):
        B, nx = Xf.shape
        self.B, self.nx, self.batched = B, nx, batched
        self.mp = np.zeros((B, NBETA, nx + Pf.shape[1]))
        self.A, self.me, self.fe = np.zeros((B, NBETA)), np.zeros((B, NBETA)), np.zeros((B, NBETA))
        self.flags = np.zeros((B, NBETA), np.int8)
        self.nit, self.nfev = np.zeros((B, NBETA), np.int32), np.zeros((B, NBETA), np.int64)
        self.starts, self.ends = [], []              # the start point and the minimiser of every rung
        P = np.array(Pf)
        x = np.concatenate([Xf, Pf[:, estpos]], axis=1)
        for k in range(NBETA):
            self.starts.append(x.copy())
            for b in range(B):
                if results is None:
                    c = canned(k + 1, b)
                    x[b] = 0.5 * x[b] + c["shift"]
                else:                                # the SciPy route: (x, A, me, fe, status, nit, nfev) per rung
                    c = dict(zip(("x", "A", "me", "fe", "status", "nit", "nfev"), results(k, x[b])))
                    x[b] = c["x"]
                P[b, estpos] = x[b, nx:]
                self.mp[b, k] = np.concatenate([x[b, :nx], P[b]])
                self.A[b, k], self.me[b, k], self.fe[b, k] = c["A"], c["me"], c["fe"]
                self.flags[b, k], self.nit[b, k], self.nfev[b, k] = c["status"], c["nit"], c["nfev"]
            self.ends.append(x.copy())
        self.P = P

    def view(self, a):
        return a if self.batched else a[0]

    def check_tables(self, a):
        for got, want in ((a.minpaths, self.mp), (a.A_array, self.A), (a.me_array, self.me), (a.fe_array, self.fe),
                          (a.exitflags, self.flags), (a.nit_array, self.nit), (a.nfev_array, self.nfev)):
            assert got.dtype == want.dtype and np.array_equal(got, self.view(want))
        assert np.array_equal(a._mp, self.mp) and np.array_equal(a._Pfull, self.P)


def rf_scale():
    return float(ALPHA) ** np.arange(NBETA)


def check_log(log, exp, plan, opt_args=OPTS):
    """plan: 'steps' | 'fused' | 'mixed' (two single rungs, the rest in one call)"""
    nsteps = {"steps": NBETA, "fused": 0, "mixed": 2}[plan]
    assert len(log) == nsteps + (nsteps < NBETA)
    for k in range(nsteps):
        name, XP, rf, oa = log[k]
        assert name == "minimize_lbfgs" and np.array_equal(XP, exp.starts[k]) and rf == rf_scale()[k] and oa is opt_args
    if nsteps < NBETA:
        name, XP, rf, oa, want_paths = log[nsteps]
        assert name == "anneal" and np.array_equal(XP, exp.starts[nsteps]) and np.array_equal(rf, rf_scale()[nsteps:])
        assert oa is opt_args and want_paths is True


def mask(text):
    text = re.sub(r"Time = \S+ s", "Time = T s", text)
    return re.sub(r"\): \S+ s,", "): T s,", text)


def header_text(k, rf0):
    return ("------------------------------\nStep %d of %d\nbeta = %d, RF = %.8e\n\n"
            % (k + 1, NBETA, k, rf0 * float(ALPHA) ** k))


def step_text(exp, k, message=None):
    """what anneal_step prints; single seed: scalars, a batch: the arrays"""
    pick = (lambda t: t[0, k]) if exp.B == 1 else (lambda t: t[:, k])
    out = "Optimization complete!\nTime = T s\nExit flag = {0}\n".format(pick(exp.flags))
    if message is not None:
        out += "Exit message: {0}\n".format(message)
    return out + "Iterations = {0}\nObj. function value = {1}\n\n".format(pick(exp.nit), pick(exp.A))


def ladder_text(exp, k0):
    return ("Ladder of %d steps x %d seed(s): T s, %d action+gradient evaluations\n"
            % (NBETA - k0, exp.B, int(exp.nfev[:, k0:].sum())))


def check_ladder_state(a, rf0):
    assert a.betaidx == NBETA - 1 and a.beta == NBETA - 1 and a.Nbeta == NBETA
    assert np.array_equal(a.RF, rf0 * float(ALPHA) ** (NBETA - 1))
    assert np.array_equal(a._rf_scale, rf_scale())
    assert a.taped is False and a.initalized is True and a.adolcID == 3


# ---------------------------------------------------------------------------------- the ODE class
D, N, NP, PIDX, LIDX = 3, 5, 3, [2, 0], [0, 2]
ND = N * D
T_MODEL = 0.25 * np.arange(N)
Y = 0.25 * np.arange(1, 2 * N + 1).reshape(N, 2) - 1.0
RF0 = 0.5


def ode_inputs(batched, tdp, pidx=PIDX):
    B = 2 if batched else 1
    X0 = 0.25 * (np.arange(B * ND).reshape(B, N, D) % 11) - 1.0
    P0 = 0.5 * np.arange(1, B * (N if tdp else 1) * NP + 1).reshape((B, N, NP) if tdp else (B, NP))
    if not batched:
        X0, P0 = X0[0], P0[0]
    Xe = X0.copy()
    Xe[..., LIDX] = Y                                # init_to_data
    estpos = [n * NP + k for n in range(N) for k in pidx] if tdp else list(pidx)
    return X0, P0, Xe.reshape(B, ND), P0.reshape(B, -1).copy(), estpos


def ode_annealer():
    a = va_ode.Annealer()
    a.set_model(lambda t, x, p: -p[0] * x, D)
    a.set_data(Y, t=T_MODEL)
    return a


def ode_args(X0, P0, pidx=PIDX):
    return X0, P0, ALPHA, np.arange(NBETA), 4.0, RF0, LIDX, pidx


def run_plan(a, plan, args, **kw):
    if plan == "mixed":
        a.anneal_init(*args, opt_args=OPTS, adolcID=3, **kw)
        a.anneal_step()
        a.anneal_step()
        a._anneal_fused()
    else:
        a.anneal(*args, opt_args=OPTS, adolcID=3, fused=None if plan == "fused" else False, **kw)


def ode_fused_text(exp, k0):
    out = ""
    for k in range(k0, NBETA):
        out += ("Step %d of %d  beta = %d  RF = %.8e  exit flag = %s  iterations = %s  A = %s\n"
                % (k + 1, NBETA, k, RF0 * float(ALPHA) ** k, exp.view(exp.flags)[..., k], exp.view(exp.nit)[..., k],
                   exp.view(exp.A)[..., k]))
    return out + "\n" + ladder_text(exp, k0)


def check_written_back(P0, exp, estpos):
    """the caller's parameter array holds the last rung's estimates, its other entries untouched"""
    assert np.array_equal(P0.reshape(exp.B, -1), exp.P)
    assert np.array_equal(exp.P[:, estpos], exp.mp[:, -1, exp.nx:][:, estpos])


def check_ode_savers(a, exp, tdp, tmp_path):
    B = exp.B
    paths = np.concatenate([np.broadcast_to(T_MODEL[:, None], (B, NBETA, N, 1)),
                            exp.mp[:, :, :ND].reshape(B, NBETA, N, D)], axis=3)
    params = exp.mp[:, :, ND:].reshape((B, NBETA, N, NP) if tdp else (B, NBETA, NP))
    ae = np.zeros((B, NBETA, 5))
    ae[:, :, 0] = np.arange(NBETA)
    ae[:, :, 1], ae[:, :, 2], ae[:, :, 3] = exp.A, exp.me, exp.fe
    ae[:, :, 4] = exp.fe / (RF0 * rf_scale())
    for name, save, want, width in (("paths", a.save_paths, paths, D + 1), ("params", a.save_params, params, NP),
                                    ("ae", a.save_action_errors, ae, 5)):
        f = str(tmp_path / (name + ".npy"))
        save(f)
        got = np.load(f)
        assert got.dtype == np.float64 and np.array_equal(got, exp.view(want))
        save(f, dtype=np.float32)
        assert np.load(f).dtype == np.float32 and np.array_equal(np.load(f), exp.view(want).astype(np.float32))
        f = str(tmp_path / (name + ".txt"))
        save(f, fmt="%.10e")
        assert np.array_equal(np.loadtxt(f), want.reshape(-1, width))
    a.save_as_minAone(str(tmp_path), seed=B - 1)
    rows = np.loadtxt(str(tmp_path / ("D%d_M%d_PATH3.dat" % (D, len(LIDX)))))
    assert np.array_equal(rows, np.hstack([np.arange(NBETA)[:, None], exp.flags[B - 1][:, None], exp.A[B - 1][:, None],
                                           exp.mp[B - 1]]))


@pytest.mark.parametrize("plan", ["steps", "fused", "mixed"])
@pytest.mark.parametrize("tdp", [False, True])
@pytest.mark.parametrize("batched", [False, True])
def test_ode_ladder(fake, capsys, tmp_path, batched, tdp, plan):
    X0, P0, Xf, Pf, estpos = ode_inputs(batched, tdp)
    P_before = P0.copy()
    a = ode_annealer()
    run_plan(a, plan, ode_args(X0, P0), verbose=True)
    exp = Expected(Xf, Pf, estpos, batched)
    assert np.array_equal(X0.reshape(exp.B, ND), Xf)                 # init_to_data wrote into the caller's X0
    pb = a._pb
    assert isinstance(pb, FakeOde) and pb.created["p_time_dependent"] is tdp and pb.created["rhs"] == 1000
    assert pb.created["lbfgs_m"] == 5 and pb.created["max_beta"] == NBETA and pb.created["keep_paths"] == 1
    assert pb.created["device"] == 0 and pb.created["bounds"] is None and a._rhs_module == {"so": "generated.so"}
    check_log(pb.log, exp, plan)
    exp.check_tables(a)
    assert a.P is P0 and a.minpaths.shape == ((exp.B,) if batched else ()) + (NBETA, ND + Pf.shape[1])
    check_written_back(P0, exp, estpos)
    rest = [j for j in range(Pf.shape[1]) if j not in estpos]
    assert np.array_equal(P0.reshape(exp.B, -1)[:, rest], P_before.reshape(exp.B, -1)[:, rest])
    check_ladder_state(a, RF0)
    assert a.beta_array.dtype == np.uint16 and a._estpos == estpos and a.NPest == 2 and a.B == exp.B
    text = {"steps": "".join(header_text(k, RF0) + step_text(exp, k) for k in range(NBETA)),
            "fused": ode_fused_text(exp, 0),
            "mixed": step_text(exp, 0) + step_text(exp, 1) + ode_fused_text(exp, 2)}[plan]
    assert mask(capsys.readouterr().out) == text
    check_ode_savers(a, exp, tdp, tmp_path)
    a.close()
    assert pb.closed and a._pb is None


@pytest.mark.parametrize("plan", ["steps", "fused"])
@pytest.mark.parametrize("tdp", [False, True])
def test_ode_no_estimated_parameters(fake, capsys, tmp_path, tdp, plan):
    X0, P0, Xf, Pf, estpos = ode_inputs(False, tdp, pidx=[])
    P_before = P0.copy()
    a = ode_annealer()
    run_plan(a, plan, ode_args(X0, P0, []), verbose=False)
    exp = Expected(Xf, Pf, [], False)
    check_log(a._pb.log, exp, plan)
    exp.check_tables(a)
    assert np.array_equal(P0, P_before) and a._pb.n_var == ND and a.NPest == 0
    check_ladder_state(a, RF0)
    assert capsys.readouterr().out == ""
    a.save_params(str(tmp_path / "p.npy"))
    assert capsys.readouterr().out == ("WARNING: You did not estimate any parameters.  Writing fixed parameter "
                                       "values to file anyway.\n")
    assert np.array_equal(np.load(str(tmp_path / "p.npy")), np.broadcast_to(P_before, (NBETA,) + P_before.shape))


def scipy_results(minimize_calls_before=0):
    """rung results on the SciPy route: the recorder's answer, me / fe from one more evaluation"""
    def results(k, x0):
        n = minimize_calls_before + k + 1
        rf = rf_scale()[k]
        x = 0.5 * x0 + n
        A, me, fe, _ = eval_canned(x[None, :], rf)
        return x, eval_canned(x0[None, :], rf)[0][0] + n, me[0], fe[0], n % 3, 3 * n, 5 * n
    return results


def check_scipy_route(pb, minimize, exp, method, bounds):
    """one SciPy call per rung: fg evaluated at the start point, then (me, fe) at the minimiser"""
    assert len(minimize.calls) == NBETA and len(pb.log) == 2 * NBETA
    for k, (x0, kw) in enumerate(minimize.calls):
        assert np.array_equal(x0, exp.starts[k][0])
        assert kw["method"] == method and kw["jac"] is True and kw["options"] is OPTS
        if bounds == "absent":
            assert sorted(kw) == ["jac", "method", "options"]
        else:
            assert sorted(kw) == ["bounds", "jac", "method", "options"] and kw["bounds"] is bounds
        name, XP, rf, want_grad = pb.log[2 * k]
        assert name == "action_grad" and np.array_equal(XP, exp.starts[k]) and rf == rf_scale()[k] and want_grad is True
        name, XP, rf, want_grad = pb.log[2 * k + 1]
        assert name == "action_grad" and np.array_equal(XP, exp.ends[k]) and rf == rf_scale()[k] and want_grad is False


@pytest.mark.parametrize("route", ["TNC", "NCG", "bounds"])
def test_ode_scipy_route(fake, minimize, capsys, route):
    X0, P0, Xf, Pf, estpos = ode_inputs(False, False)
    a = ode_annealer()
    kw = dict(method=route) if route != "bounds" else dict(bounds=[(-9.0, 9.0)] * D + [(0.0, 8.0), (-1.0, 1.0), (2.0, 3.0)],
                                                           bounded_minimiser="scipy")
    a.anneal(*ode_args(X0, P0), opt_args=OPTS, adolcID=3, verbose=True, **kw)
    assert a._device_minimiser is False and a._device_bounds is False and a._pb.created["bounds"] is None
    exp = Expected(Xf, Pf, estpos, False, results=scipy_results())
    if route == "bounds":
        # va_ode.py:582-605: state bounds per time point, then one pair per estimated parameter
        assert a.bounds == [(-9.0, 9.0)] * ND + [(0.0, 8.0), (-1.0, 1.0)]
        check_scipy_route(a._pb, minimize, exp, "L-BFGS-B", a.bounds)
    else:
        assert a.bounds is None
        check_scipy_route(a._pb, minimize, exp, {"TNC": "TNC", "NCG": "CG"}[route], None if route == "TNC" else "absent")
    exp.check_tables(a)
    check_written_back(P0, exp, estpos)
    check_ladder_state(a, RF0)
    text = "".join(header_text(k, RF0) + step_text(exp, k, message="stopped %d" % (k + 1)) for k in range(NBETA))
    assert mask(capsys.readouterr().out) == text
    with pytest.raises(ValueError):
        a.anneal(*ode_args(X0, P0), fused=True, **kw)
    Xb, Pb = ode_inputs(True, False)[:2]
    with pytest.raises(ValueError):                  # SciPy on the host: one seed only
        ode_annealer().anneal(*ode_args(Xb, Pb), **kw)


def test_ode_tracking_saves_after_every_rung(fake, tmp_path):
    """track_* switches the fused ladder off and writes the tables after every rung"""
    X0, P0, Xf, Pf, estpos = ode_inputs(False, False)
    a = ode_annealer()
    seen = []
    real = a.save_paths

    def save_paths(*args):
        seen.append((a.betaidx, a._A[0].copy()))
        real(*args)
    a.save_paths = save_paths
    a.anneal(*ode_args(X0, P0), opt_args=OPTS, adolcID=3, verbose=False,
             track_paths={"filename": str(tmp_path / "tp.npy"), "dtype": np.float32},
             track_params={"filename": str(tmp_path / "tq.txt"), "fmt": "%.10e"},
             track_action_errors={"filename": str(tmp_path / "ta.npy")})
    exp = Expected(Xf, Pf, estpos, False)
    check_log(a._pb.log, exp, "steps")
    exp.check_tables(a)
    assert [k for k, _ in seen] == [1, 2, 3, 3]
    assert all(np.array_equal(A[:k + 1], exp.A[0, :k + 1]) and not A[k + 1:].any() for k, (_, A) in enumerate(seen))
    assert np.load(str(tmp_path / "tp.npy")).dtype == np.float32
    assert np.array_equal(np.loadtxt(str(tmp_path / "tq.txt")), exp.mp[0, :, ND:])
    assert np.array_equal(np.load(str(tmp_path / "ta.npy"))[:, 1], exp.A[0])


# ---------------------------------------------------------------------------------- the network class
STRUCTURE, M = [3, 2, 2], 2
NDNET = 7
NDENS = M * NDNET
NPNET = 2 * 3 + 2 + 2 * 2 + 2
NN_PIDX = [1, 0, 7, 12]
DIN = 0.25 * np.arange(1, 7).reshape(M, 3)
DOUT = -0.5 * np.arange(1, 5).reshape(M, 2)
NN_RF0 = 0.25


def nnet_inputs(batched):
    B = 2 if batched else 1
    X0 = 0.25 * (np.arange(B * NDENS).reshape(B, NDENS) % 9) - 0.5
    P0 = 0.5 * np.arange(1, B * NPNET + 1).reshape(B, NPNET) - 3.0
    if not batched:
        X0, P0 = X0[0], P0[0]
    Xe = X0.copy().reshape(B, M, NDNET)
    Xe[:, :, :3] = DIN                               # init_to_data: input layer, output layer
    Xe[:, :, NDNET - 2:] = DOUT
    return X0, P0, Xe.reshape(B, NDENS), P0.reshape(B, NPNET).copy()


def nnet_annealer():
    a = va_nnet.Annealer()
    a.set_structure(STRUCTURE)
    a.set_activation("tanh")
    a.set_input_data(DIN)
    a.set_output_data(DOUT)
    return a


def nnet_args(X0, P0):
    return X0, P0, ALPHA, np.arange(NBETA), 2.0, NN_RF0, NN_PIDX


def layers(row):
    return [row[0:3], row[3:5], row[5:7]]


def check_nnet_savers(a, exp, tmp_path):
    mp = exp.mp[0]
    f = lambda name: str(tmp_path / name)
    a.save_states(f("st.npy"))
    st = np.load(f("st.npy"), allow_pickle=True)
    assert st.shape == (M, NBETA, 3) and st.dtype == object
    a.save_io(f("io.npy"))
    io = np.load(f("io.npy"), allow_pickle=True)
    assert io.shape == (M, NBETA, 2) and io.dtype == object
    for m in range(M):
        for k in range(NBETA):
            want = layers(mp[k, m * NDNET:(m + 1) * NDNET])
            assert all(np.array_equal(st[m, k, n], want[n]) and st[m, k, n].dtype == np.float64 for n in range(3))
            assert np.array_equal(io[m, k, 0], want[0]) and np.array_equal(io[m, k, 1], want[2])
    a.save_params(f("p.npy"), dtype=np.float32)
    assert np.load(f("p.npy")).dtype == np.float32 and np.array_equal(np.load(f("p.npy")), mp[:, NDENS:].astype(np.float32))
    a.save_params(f("p.txt"), fmt="%.10e")
    assert np.array_equal(np.loadtxt(f("p.txt")), mp[:, NDENS:])
    ae = np.column_stack([np.arange(NBETA), exp.A[0], exp.me[0], exp.fe[0], exp.fe[0] / (NN_RF0 * rf_scale())])
    a.save_action_errors(f("ae.npy"))
    assert np.load(f("ae.npy")).dtype == np.float64 and np.array_equal(np.load(f("ae.npy")), ae)
    a.save_action_errors(f("ae.txt"), fmt="%.10e")
    assert np.array_equal(np.loadtxt(f("ae.txt")), ae)
    a.save_Wb(f("W.npy"), f("b.npy"))
    W, b = np.load(f("W.npy"), allow_pickle=True), np.load(f("b.npy"), allow_pickle=True)
    assert W.shape == (NBETA, 2) and W.dtype == object           # ragged: (2, 3) and (2, 2) weight matrices
    assert b.shape == (NBETA, 2, 2) and b.dtype == np.float64    # uniform: two biases per layer
    for k in range(NBETA):
        p = mp[k, NDENS:]
        assert np.array_equal(W[k, 0], p[0:6].reshape(2, 3)) and np.array_equal(b[k, 0], p[6:8])
        assert np.array_equal(W[k, 1], p[8:12].reshape(2, 2)) and np.array_equal(b[k, 1], p[12:14])
    Wl, bl = a.weights_biases()
    assert np.array_equal(Wl[1], W[-1, 1]) and np.array_equal(bl[0], b[-1, 0])


@pytest.mark.parametrize("plan", ["steps", "fused", "mixed"])
@pytest.mark.parametrize("batched", [False, True])
def test_nnet_ladder(fake, capsys, tmp_path, batched, plan):
    X0, P0, Xf, Pf = nnet_inputs(batched)
    P_before = P0.copy()
    a = nnet_annealer()
    run_plan(a, plan, nnet_args(X0, P0), verbose=True)
    exp = Expected(Xf, Pf, NN_PIDX, batched)
    assert np.array_equal(X0.reshape(exp.B, NDENS), Xf)              # init_to_data wrote into the caller's X0
    pb = a._pb
    assert isinstance(pb, FakeNnet) and pb.created == dict(act="tanh", lbfgs_m=5, max_beta=NBETA, keep_paths=1, device=0)
    check_log(pb.log, exp, plan)
    exp.check_tables(a)
    assert a.P is P0 and a.minpaths.shape == ((exp.B,) if batched else ()) + (NBETA, NDENS + NPNET)
    check_written_back(P0, exp, NN_PIDX)
    rest = [j for j in range(NPNET) if j not in NN_PIDX]
    assert np.array_equal(P0.reshape(exp.B, -1)[:, rest], P_before.reshape(exp.B, -1)[:, rest])
    check_ladder_state(a, NN_RF0)
    assert a.beta_array.dtype == np.arange(NBETA).dtype and a._act == "tanh" and a.NPest == 4 and a.B == exp.B
    text = {"steps": "".join(header_text(k, NN_RF0) + step_text(exp, k) for k in range(NBETA)),
            "fused": ladder_text(exp, 0),
            "mixed": step_text(exp, 0) + step_text(exp, 1) + ladder_text(exp, 2)}[plan]
    assert mask(capsys.readouterr().out) == text
    if batched:
        for save in (a.save_states, a.save_io, a.save_params, a.save_action_errors):
            with pytest.raises(ValueError):
                save(str(tmp_path / "x.npy"))
    else:
        check_nnet_savers(a, exp, tmp_path)
    a.close()
    assert pb.closed and a._pb is None


def test_nnet_scipy_route_prints_no_exit_message(fake, minimize, capsys):
    X0, P0, Xf, Pf = nnet_inputs(False)
    a = nnet_annealer()
    a.anneal(*nnet_args(X0, P0), method="TNC", opt_args=OPTS, adolcID=3, verbose=True)
    exp = Expected(Xf, Pf, NN_PIDX, False, results=scipy_results())
    check_scipy_route(a._pb, minimize, exp, "TNC", None)
    exp.check_tables(a)
    check_written_back(P0, exp, NN_PIDX)
    text = "".join(header_text(k, NN_RF0) + step_text(exp, k) for k in range(NBETA))
    assert mask(capsys.readouterr().out) == text


# ---------------------------------------------------------------------------------- the ADmin surface
def admin_case(which):
    if which == "ode":
        X0, P0, Xf, Pf, estpos = ode_inputs(False, False)
        return ode_annealer(), ode_args(X0, P0), Xf, Pf, estpos
    X0, P0, Xf, Pf = nnet_inputs(False)
    return nnet_annealer(), nnet_args(X0, P0), Xf, Pf, NN_PIDX


@pytest.mark.parametrize("which", ["ode", "nnet"])
def test_admin_surface(fake, minimize, which):
    a, args, Xf, Pf, estpos = admin_case(which)
    a.anneal_init(*args, opt_args=OPTS, adolcID=3, verbose=False)
    a.anneal_step()                                  # the evaluations below run at the second rung's RF
    log = a._pb.log
    del log[:]
    XP = 0.25 * np.arange(a._pb.n_var)
    A, me, fe, g = (v[0] for v in eval_canned(XP[None, :], 2.0))
    a.tape_A(a.gen_xtrace())
    assert a.taped is True and a.gen_xtrace().shape == XP.shape
    assert a.A_taped(XP) == A and a.A_gaussian(XP) == A and a.A(XP) == A
    assert a.me_gaussian(XP) == me and a.fe_gaussian(XP) == fe
    assert [(e[0], e[2], e[3]) for e in log] == [("action_grad", 2.0, False)] * 5
    assert all(np.array_equal(e[1], XP[None, :]) for e in log)
    del log[:]
    assert np.array_equal(a.gradA_taped(XP), g)
    A2, g2 = a.A_gradA_taped(XP)
    assert A2 == A and np.array_equal(g2, g)
    assert [(e[0], e[2], e[3]) for e in log] == [("action_grad", 2.0, True)] * 2
    # a batch of points: arrays come back
    del log[:]
    assert a.B == 1 and np.array_equal(a.A_gaussian(XP[None, :]), [A])
    # min_lbfgs_scipy without bounds: the device minimiser
    del log[:]
    x, Amin, status = a.min_lbfgs_scipy(XP)
    c = canned(2, 0)
    assert np.array_equal(x, 0.5 * XP + c["shift"]) and (Amin, status) == (c["A"], c["status"])
    assert type(Amin) is float and type(status) is int
    assert len(log) == 1 and log[0][0] == "minimize_lbfgs" and np.array_equal(log[0][1], XP[None, :])
    assert log[0][2] == 2.0 and log[0][3] is OPTS
    # CG / TNC: SciPy on the host around action_grad
    for n, (call, meth) in enumerate(((a.min_cg_scipy, "CG"), (a.min_tnc_scipy, "TNC")), 1):
        del log[:]
        x, Amin, status = call(XP)
        assert np.array_equal(x, 0.5 * XP + n) and (Amin, status) == (A + n, n % 3)
        x0, kw = minimize.calls[-1]
        assert np.array_equal(x0, XP) and kw["method"] == meth and kw["jac"] is True and kw["options"] is OPTS
        assert sorted(kw) == (["jac", "method", "options"] if meth == "CG" else ["bounds", "jac", "method", "options"])
        assert meth == "CG" or kw["bounds"] is None
        assert [(e[0], e[2], e[3]) for e in log] == [("action_grad", 2.0, True)]
    with pytest.raises(NotImplementedError):
        a.hessianA_taped(XP)
    with pytest.raises(NotImplementedError):
        a.jacA_taped(XP)
    with pytest.raises(NotImplementedError):
        a.min_lm_scipy(XP)


def test_admin_min_lbfgs_scipy_with_bounds(fake, minimize):
    """with bounds, min_lbfgs_scipy is SciPy's L-BFGS-B on the host and receives them"""
    X0, P0, Xf, Pf, estpos = ode_inputs(False, False)
    a = ode_annealer()
    a.anneal_init(*ode_args(X0, P0), opt_args=OPTS, bounds=[(-9.0, 9.0)] * D + [(0.0, 8.0)] * NP,
                  bounded_minimiser="scipy", verbose=False)
    XP = 0.25 * np.arange(ND + 2)
    x, Amin, status = a.min_lbfgs_scipy(XP)
    x0, kw = minimize.calls[-1]
    assert np.array_equal(x0, XP) and sorted(kw) == ["bounds", "jac", "method", "options"]
    assert kw["method"] == "L-BFGS-B" and kw["bounds"] is a.bounds and len(a.bounds) == ND + 2
    assert np.array_equal(x, 0.5 * XP + 1) and (Amin, status) == (eval_canned(XP[None, :], 1.0)[0][0] + 1, 1)
    assert [(e[0], e[2], e[3]) for e in a._pb.log] == [("action_grad", 1.0, True)]


def test_admin_needs_one_initialised_seed(fake):
    with pytest.raises(RuntimeError):
        ode_annealer().min_cg_scipy(np.zeros(3))
    X0, P0 = ode_inputs(True, False)[:2]
    a = ode_annealer()
    a.anneal_init(*ode_args(X0, P0), verbose=False)
    with pytest.raises(ValueError):
        a.min_lbfgs_scipy(np.zeros(ND + 2))
