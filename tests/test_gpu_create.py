"""GPU: problem creation (csrc/va_capi.hip: va_problem_create, va_nnet_problem_create).  A refused descriptor says why in
the words it always has and leaves a process in which the next handle works; both constructors give the same handle on a
caller's stream and on one of their own, and again after a destroy; the network handle on the device carries the plan the
CPU check of csrc/va_nnet_geo.h records.  Every refusal here comes from a host check: no kernel is launched for it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch        # ahead of the library: both then share the HIP runtime torch brings, and torch.cuda sees the device

import va_oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -4            # VA_EINVAL, VA_EUNSUPPORTED (include/varanneal_amd.h)
RTOL_A, RTOL_G = 1e-12, 1e-10            # single evaluations, as tests/test_gpu_parity.py
D, N, B, L = 8, 11, 2, 4
LIDX = [0, 2, 4, 6]
NN_S, NN_M = (3, 4, 2), 5


@pytest.fixture(scope="module")
def capi():
    from varanneal_amd import _capi
    _capi.lib()
    return _capi


@pytest.fixture(scope="module")
def ode():
    """the valid problem, a start point per seed, and what the NumPy action and the oracle's gradient say of each.
    (tests/_util.py builds its oracle problems from stored cases only; this D = 8, N = 11 problem is none of them, so the
    same reference, va_oracle.Problem and its numpy_action, is built here directly, with test_gpu_parity.py's tolerances)"""
    rng = np.random.default_rng(811)
    Y = rng.standard_normal((N, L))
    P = np.array([[8.17], [7.9]])
    XP = np.concatenate([rng.standard_normal((B, N * D)), P], axis=1)
    want = []
    for b in range(B):
        o = va_oracle.Problem(D, N, Y, LIDX, 0.025, 4.0, 4e-6, P[b], [0], disc="trapezoid")
        want.append((o.numpy_action(XP[b], 50.0), o.action_grad(XP[b], 50.0)[3]))
    return dict(Y=Y, P=P, XP=XP, want=want)


def ode_desc(capi, ode, **kw):
    return capi.make_desc(B, D, N, ode["Y"], LIDX, 0.025, 4.0, 4e-6, ode["P"], [0], disc="trapezoid", **kw)


def check_valid_problem(capi, ode):
    with capi.Problem(B, D, N, ode["Y"], LIDX, 0.025, 4.0, 4e-6, ode["P"], [0], disc="trapezoid") as pb:
        A, me, fe, g = pb.action_grad(ode["XP"], 50.0)
    for b, ((A0, me0, fe0), g0) in enumerate(ode["want"]):
        assert abs(A[b] - A0) <= RTOL_A * abs(A0) and abs(me[b] - me0) <= RTOL_A * abs(A0) and abs(fe[b] - fe0) <= RTOL_A * abs(A0)
        assert np.abs(g[b] - g0).max() <= RTOL_G * np.abs(g0).max()


def nnet_args(capi):
    from varanneal_amd import twin
    din, dout, _ = twin.make_nnet_twin(NN_S, NN_M)
    X, P, Pidx = twin.nnet_initial_guess(NN_S, NN_M, 0)
    Lidx = [np.arange(NN_S[0]), np.arange(NN_S[-1])]
    return (1, NN_S, din, dout, Lidx, 4.0e4, 0.0038, P[None, :], Pidx), np.append(X, P[Pidx])[None, :]


def refused(capi, create, desc):
    h = C.c_void_p()
    rc = create(C.byref(desc), C.byref(h))
    msg = capi.lib().va_last_error().decode()
    assert not h.value
    return rc, msg


# ---- descriptor mutations: (what to change, code, words of va_last_error()), read off the checks as they stood before
# creation was split into steps
def _rm_kind_3(d, keep):
    keep.append(np.ones((N, L)))
    d.rm_kind, d.rm_array = 3, keep[-1].ctypes.data_as(C.POINTER(C.c_double))


def _bounds(lower_at_3, upper_at_3):
    def mutate(d, keep):
        lo, hi = np.full(N * D + 1, -1e3), np.full(N * D + 1, 1e3)
        lo[3], hi[3] = lower_at_3, upper_at_3
        keep += [lo, hi]
        d.lower, d.upper = lo.ctypes.data_as(C.POINTER(C.c_double)), hi.ctypes.data_as(C.POINTER(C.c_double))
    return mutate


def _lidx_twice(d, keep):
    keep.append(np.array([0, 2, 2, 6], dtype=np.int32))
    d.Lidx = keep[-1].ctypes.data_as(C.POINTER(C.c_int32))


def _set(**fields):
    def mutate(d, keep):
        for k, v in fields.items():
            setattr(d, k, v)
    return mutate


ODE_REFUSALS = [
    ("rm_kind=3", _rm_kind_3, EINVAL, "rm_kind 3"),
    ("lower>upper", _bounds(2.0, 1.0), EINVAL, "lower[3] > upper[3] (or NaN)"),
    ("NaN bound", _bounds(float("nan"), 1.0), EINVAL, "lower[3] > upper[3] (or NaN)"),
    ("Lidx twice", _lidx_twice, EUNSUPPORTED, "Lidx lists state column 2 twice"),
    ("N_model", _set(N_model=N + 1), EINVAL, "N_model (12) must equal (N_data-1)*merr_nskip+1 (11)"),
    ("SimpsonHermite even", _set(disc=2, N_model=N + 1, N_data=N + 1), EINVAL, "SimpsonHermite needs an odd number of time points (N_model=12)"),
    ("lbfgs_m", _set(lbfgs_m=33), EINVAL, "lbfgs_m=33 > 32"),
    ("device", _set(device=99), EINVAL, "device 99 of "),
]


def _pidx_twice(d, keep):
    pidx = np.arange(d.NPest, dtype=np.int32)
    pidx[1] = pidx[0]
    keep.append(pidx)
    d.Pidx = pidx.ctypes.data_as(C.POINTER(C.c_int32))


NNET_REFUSALS = [
    ("NP", _set(NP=25), EINVAL, "NP=25 but the structure holds 26 weights and biases"),
    ("Pidx twice", _pidx_twice, EINVAL, "Pidx[1]=0 listed twice"),
    ("nothing observed", _set(L_in=0, L_out=0), EINVAL, "no observed neurons"),
]


@pytest.mark.parametrize("name,mutate,code,words", ODE_REFUSALS, ids=[r[0] for r in ODE_REFUSALS])
def test_refused_problem_keeps_its_words_and_leaves_a_working_process(capi, ode, name, mutate, code, words):
    d, keep = ode_desc(capi, ode)
    mutate(d, keep)
    rc, msg = refused(capi, capi.lib().va_problem_create, d)
    assert rc == code and words in msg, (rc, msg)
    check_valid_problem(capi, ode)


@pytest.mark.parametrize("name,mutate,code,words", NNET_REFUSALS, ids=[r[0] for r in NNET_REFUSALS])
def test_refused_network_keeps_its_words_and_leaves_a_working_process(capi, ode, name, mutate, code, words):
    args, _ = nnet_args(capi)
    d, keep = capi.make_nnet_desc(*args)
    assert d.NP == 26 and d.NPest >= 2
    keep = list(keep)
    mutate(d, keep)
    rc, msg = refused(capi, capi.lib().va_nnet_problem_create, d)
    assert rc == code and words in msg, (rc, msg)
    check_valid_problem(capi, ode)


def test_both_constructors_share_their_back_half(capi, ode):
    """an ODE handle and a small-path network handle, on a caller's stream and on their own, created, evaluated, destroyed
    and created again: one result, bit for bit"""
    args, XPn = nnet_args(capi)
    mine = torch.cuda.Stream()
    got_ode, got_net = [], []
    for stream in (mine.cuda_stream, None):
        for again in range(2):
            with capi.Problem(B, D, N, ode["Y"], LIDX, 0.025, 4.0, 4e-6, ode["P"], [0], disc="trapezoid", stream=stream) as pb:
                got_ode.append(pb.action_grad(ode["XP"], 50.0))
            with capi.NnetProblem(*args, stream=stream) as nb:
                assert nb.info()["ntiles"] == len(NN_S)            # the small path: one workgroup per layer
                got_net.append(nb.action_grad(XPn, 1.0e4))
    torch.cuda.synchronize()
    for got in (got_ode, got_net):
        for other in got[1:]:
            for a, b in zip(got[0], other):
                assert np.array_equal(a, b)
    assert np.all(np.isfinite(got_net[0][3])) and np.abs(got_net[0][3]).max() > 0.0


@pytest.fixture(scope="module")
def plan_of():
    """the plan csrc/va_nnet_geo.h makes for a network on THIS device's CU count, through the CPU check built with g++"""
    import importlib.util
    import tempfile
    spec = importlib.util.spec_from_file_location("dump_nnet_plans", os.path.join(ROOT, "tools", "dump_nnet_plans.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "nnet_plan_check")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "varanneal_amd", "csrc"), "-o", exe,
                               os.path.join(ROOT, "tests", "cpu_emul", "nnet_plan_check.cpp")])

        def plan(batch, M, s, L_in, L_out):
            row = tool.row(batch, M, ncu, s, L_in=L_in, L_out=L_out)
            out = subprocess.run([exe], input=" ".join(str(v) for v in row) + "\n", capture_output=True, text=True, check=True)
            return tool.parse(out.stdout.splitlines()[0])[0]
        yield plan


@pytest.mark.parametrize("s,M,path", [((3, 4, 2), 5, "small"), ((40, 70, 10), 70, "tiled"), ((128, 128, 10), 64, "fb")])
def test_network_plan_on_the_device_is_the_recorded_one(capi, plan_of, s, M, path):
    from varanneal_amd import twin
    din, dout, _ = twin.make_nnet_twin(s, M)
    X, P, Pidx = twin.nnet_initial_guess(s, M, 0)
    Lidx = [np.arange(s[0]), np.arange(s[-1])]
    p = plan_of(2, M, s, s[0], s[-1])
    # (the tiled network fits k_nnet_fb as well: what sets it apart from "fb" is that its partial rows are not folded)
    assert (p["small"] > 0, p["fb_ok"] == 1, p["fold_rows"] == 1) == {"small": (True, False, False), "tiled": (False, True, False),
                                                                      "fb": (False, True, True)}[path]
    with capi.NnetProblem(2, s, din, dout, Lidx, 4.0e4, 0.0038, np.tile(P, (2, 1)), Pidx) as nb:
        info = nb.info()
        assert (info["tile_rows"], info["ntiles"]) == (64, p["nprow"])             # NN_TILE
        rc = capi.lib().va_problem_tune(nb._h, nb.TUNE["nnet_fused"], p["fused"])    # (the value the plan chose: nothing changes)
        assert (rc == 0) == bool(p["fb_ok"]), capi.lib().va_last_error()
