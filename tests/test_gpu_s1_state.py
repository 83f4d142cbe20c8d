"""An S1 evaluation carries its phase and RF in the kernel argument (Dev::s1_rf) instead of reading every seed's state;
a line-search launch still reads the states, behind the loads that do not depend on them.

What can go wrong: a launch that claims PH_START / an RF for seeds that are not there (states moved by a ladder, a graph
captured with another RF and replayed), the separate tail kernel or plain launches reading a different RF than the
folded tail, and a ladder whose idle seeds no longer return early.  Shapes: D = 20 on k_eval4 with 84-row tiles, the
geometry of the C3 shape (runs of 7 rows; asked for by tile_rows, three seeds alone would get runs of 4) -- N = 100 (two
tiles, the second partial: both edge variants), N = 260 (four tiles, interior ones too), Simpson-Hermite N = 101 on the tiles
the planner gives it -- D = 200, N = 700 on k_eval5, and a traced Lorenz-96 module at D = 20, N = 100; three seeds with
their own start points and parameters.  Reference: the C oracle, at the tolerances of tests/test_gpu_parity.py for the same quantities."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RTOL_A = 1e-12      # tests/test_gpu_parity.py: single evaluation
RTOL_G = 1e-10
OPTS = {'gtol': 1e-8, 'ftol': 1e-8, 'maxfun': 1000000, 'maxiter': 1000000}
B = 3
RF1, RF2 = 7.0, 1.5 ** 12
SHAPES = {"N100": ("trapezoid", 20, 100, 4), "N260": ("trapezoid", 20, 260, 4), "SH101": ("SimpsonHermite", 20, 101, 4),
          "D200": ("trapezoid", 200, 700, 5), "traced": ("trapezoid", 20, 100, 4)}


def _l96_user(t, x, p):
    return np.roll(x, 1, 1) * (np.roll(x, -1, 1) - np.roll(x, 2, 1)) - x + p[0]


class Case:
    """inputs of one shape and the oracle's (A, me, fe, grad) per seed at RF1 and RF2, computed once"""

    def __init__(self, name):
        from varanneal_amd import twin
        self.name = name
        self.disc, self.D, self.N, self.kernel = SHAPES[name]
        D, N = self.D, self.N
        t, Y, _, Lidx = twin.make_twin(D, N)
        if len(Lidx) % 2 and D > 64:
            Lidx = Lidx[:-1]; Y = Y[:, :-1]
        self.Y, self.Lidx, self.dt = Y, Lidx, twin.DT
        rng = np.random.RandomState(100 * D + N)
        self.XP = np.concatenate([3.0 * rng.randn(B, N * D), 6.0 + 3.0 * rng.rand(B, 1)], axis=1)
        self.P = self.XP[:, -1:].copy()
        self.ref = {}
        for rf in (RF1, RF2):
            self.ref[rf] = [self.oracle(b).action_grad(self.XP[b], rf) for b in range(B)]
        self.rhs = "lorenz96"
        self.tile_rows = 84 if (self.kernel == 4 and self.disc == "trapezoid") else 0

    def oracle(self, b):
        import va_oracle
        return va_oracle.Problem(self.D, self.N, self.Y, self.Lidx, self.dt, 4.0, 4e-6, self.P[b], [0], disc=self.disc)

    def problem(self, capi, **kw):
        if self.name == "traced" and self.rhs == "lorenz96":
            from varanneal_amd import codegen
            m = codegen.module_for(_l96_user, self.D, 1,
                                   col_variant=lambda ne, gh: capi.eval_plan(B, self.D, self.N, self.disc, ne, gh,
                                                                             tile_rows=self.tile_rows))
            assert m["col_variant"] == (4, 1, 7, 1)
            self.rhs = capi.load_rhs_module(m["so"])
        pb = capi.Problem(B, self.D, self.N, self.Y, self.Lidx, self.dt, 4.0, 4e-6, self.P, [0], disc=self.disc,
                          rhs=self.rhs, tile_rows=self.tile_rows, **kw)
        assert pb.info()["eval_kernel"] == self.kernel
        if self.tile_rows:
            assert pb.info()["tile_rows"] == 84 and pb.info()["run_rows"] == 7
        return pb

    def check(self, out, rf):
        A, me, fe, g = out
        for b in range(B):
            Ao, meo, feo, go = self.ref[rf][b]
            assert abs(A[b] - Ao) <= RTOL_A * abs(Ao), (self.name, b)
            assert abs(me[b] - meo) <= RTOL_A * max(abs(meo), abs(Ao)) and abs(fe[b] - feo) <= RTOL_A * abs(feo), (self.name, b)
            assert np.abs(g[b] - go).max() <= RTOL_G * np.abs(go).max(), (self.name, b)


_cases = {}


@pytest.fixture(scope="module")
def capi():
    from varanneal_amd import _capi
    _capi.lib()
    return _capi


@pytest.fixture(params=list(SHAPES))
def case(request):
    if request.param not in _cases:
        _cases[request.param] = Case(request.param)
    return _cases[request.param]


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def test_s1_after_the_states_have_moved(capi, case):
    """a short ladder leaves the seeds wherever its last cycle put them (idle, further up the RF ladder); the evaluation
    after it arms them again and must not see any of that"""
    with case.problem(capi, max_beta=2) as pb:
        pb.anneal(case.XP, [1.0, 1.5], dict(OPTS, maxiter=4))
        case.check(pb.action_grad(case.XP, RF1), RF1)
        case.check(pb.action_grad(case.XP, RF2), RF2)


def test_two_rf_values_through_the_timed_graph(capi, case):
    """the replayed graph holds the RF by value: a graph captured at RF1 must not serve RF2"""
    with case.problem(capi) as pb:
        pb.action_grad(case.XP, RF1)
        pb.eval_timed_prepare(RF1, 8); pb.eval_timed(RF1, 8)
        case.check(pb.read_eval_outputs(), RF1)
        pb.eval_timed_prepare(RF2, 8); pb.eval_timed(RF2, 8)
        timed = pb.read_eval_outputs()
        direct = pb.action_grad(case.XP, RF2)
        assert _same(timed, direct), case.name
        case.check(timed, RF2)
        # and back, without a prepare of its own
        pb.eval_timed(RF1, 8)
        again = pb.read_eval_outputs()
        assert _same(again, pb.action_grad(case.XP, RF1)), case.name


@pytest.mark.parametrize("knobs", [{"fold": 0}, {"graph": 0}, {"fold": 0, "graph": 0}], ids=["fold0", "graph0", "fold0-graph0"])
def test_separate_tail_and_plain_launches_give_the_same_bits(capi, case, knobs):
    """k_finalize_eval (fold = 0) and plain launches (graph = 0) take the RF from the same field as the folded tail"""
    got = []
    for kn in ({}, knobs):
        with case.problem(capi) as pb:
            pb.tune(**kn)
            ev = pb.action_grad(case.XP, RF2)
            pb.eval_timed(RF1, 8)
            ev1 = pb.read_eval_outputs()
            pb.eval_timed(RF2, 9)
            ev2 = pb.read_eval_outputs()
        got.append(list(ev) + list(ev1) + list(ev2))
    assert _same(got[0], got[1]), (case.name, knobs)
    case.check(got[1][:4], RF2); case.check(got[1][4:8], RF1); case.check(got[1][8:], RF2)


@pytest.mark.parametrize("persist", [0, 1])
def test_line_search_launches_still_read_the_states(capi, persist):
    """three rungs on the N = 260 shape, step for step against the oracle.  persist = 0: the three-launch cycle, whose
    evaluation launch reads every seed's phase -- the seeds need different numbers of evaluations, so the ones that are
    done sit idle beside running ones and must return early; persist = 1: whatever the handle chooses by itself."""
    if "N260" not in _cases:
        _cases["N260"] = Case("N260")
    c = _cases["N260"]
    o = dict(OPTS, maxiter=12)
    ref = [c.oracle(b).anneal(c.XP[b], 1.5, np.arange(3), o) for b in range(B)]
    assert len({int(r["nfev"].sum()) for r in ref}) > 1          # (the seeds do not finish together)
    with c.problem(capi, max_beta=3) as pb:
        pb.tune(persist=persist)
        r = pb.anneal(c.XP, 1.5 ** np.arange(3), o)
        after = pb.action_grad(c.XP, RF1)
    for b in range(B):
        for k in range(3):
            assert (r["nit"][b, k], r["nfev"][b, k], r["status"][b, k]) == (ref[b]["nit"][k], ref[b]["nfev"][k], ref[b]["status"][k]), (b, k)
            assert abs(r["A"][b, k] - ref[b]["A"][k]) <= 1e-6 * abs(ref[b]["A"][k]), (b, k)
    c.check(after, RF1)
