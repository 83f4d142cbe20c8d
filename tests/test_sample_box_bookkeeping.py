"""CPU: how va_ode.Annealer.sample drives the backend, bounded and unbounded, on test_ladder_bookkeeping's fake device
extended by the two sampling entry points: which entry is called with what, the pull-in of starts on a bound and its count,
z handed from call to call, the conversion of Laplace variances into masses of z."""
import numpy as np
import pytest

import _hmc_box_ref as BR
import test_ladder_bookkeeping as LB
from varanneal_amd import _capi, va_ode

fake = LB.fake


class SamplingOde(LB.FakeOde):
    """FakeOde plus hmc / hmc_box: logged, answered with numbers that say which call they came from"""

    def _sampled(self, name, XP, n_iter, thin, keep_idx, extra):
        self.n_sampling = getattr(self, "n_sampling", 0) + 1
        c, B, n = self.n_sampling, self.B, self.n_var
        keep = np.zeros(0, np.int64) if keep_idx is None else np.asarray(keep_idx)
        x = 0.5 * np.asarray(XP) + 0.125 * c
        acc = np.zeros((B, n_iter), np.int32)
        acc[:, :max(1, n_iter // 2)] = 1
        out = dict(x=x, mean=x + 1.0, var=np.full((B, n), 4.0), A=np.full((B, n_iter), float(c)), dH=np.zeros((B, n_iter)), accepted=acc,
                   n_divergent=np.zeros(B, np.int32), kept=np.repeat(x[:, None, keep], n_iter // thin, axis=1))
        if extra:
            out["z"] = np.full((B, n), 0.25 * c)
        return out

    def hmc(self, XP, rf_scale, n_iter, n_leap, eps, **kw):
        self.log.append(("hmc", (np.array(XP), rf_scale, n_iter, n_leap, np.array(eps)), kw))
        return self._sampled("hmc", XP, n_iter, kw.get("thin", 1), kw.get("keep_idx"), False)

    def hmc_box(self, XP, rf_scale, n_iter, n_leap, eps, **kw):
        self.log.append(("hmc_box", (np.array(XP), rf_scale, n_iter, n_leap, np.array(eps)), kw))
        return self._sampled("hmc_box", XP, n_iter, kw.get("thin", 1), kw.get("keep_idx"), True)


@pytest.fixture
def sampling(fake, monkeypatch):
    monkeypatch.setattr(_capi, "Problem", SamplingOde)


# states: column 0 two-sided, column 1 bounded below, column 2 free; parameters (Pidx = [2, 0]): bounded above, two-sided
BOUNDS = [(-8.0, 2.75), (2.5, None), (None, None), (None, 9.0), (0.0, 64.0)]


def _annealed(bounds, batched=True, **kw):
    X0, P0, _, _, _ = LB.ode_inputs(batched, False)
    a = LB.ode_annealer()
    a.anneal(*LB.ode_args(X0, P0), opt_args=LB.OPTS, verbose=False, bounds=bounds, **kw)
    return a


def _laplace(a, calls):
    def laplace(beta):
        calls.append(list(beta))
        return dict(state_var=np.full((a.B, 1, LB.ND), 4.0), param_cov=np.tile(9.0 * np.eye(2), (a.B, 1, 1, 1)))
    return laplace


@pytest.mark.parametrize("minimiser", ["device", "scipy"])
def test_bounded_annealer_samples_through_hmc_box(sampling, minimiser, monkeypatch):
    if minimiser == "scipy":
        import scipy.optimize as opt
        monkeypatch.setattr(opt, "minimize", LB.Minimize())
    batched = minimiser == "device"                                               # (SciPy around the device: one seed only)
    a = _annealed(BOUNDS, batched=batched, bounded_minimiser=minimiser)
    lead = (lambda v: v) if batched else (lambda v: v[None])
    assert (a._pb.created["bounds"] is None) == (minimiser == "scipy")           # sample() works on either handle
    lap = []
    a.laplace = _laplace(a, lap)
    a._pb.log[:] = []
    r = a.sample(4, beta=[1, 2], n_leap=3, warmup=5, warmup_block=3, thin=2, seed=7, mass='laplace')
    log = a._pb.log
    assert [e[0] for e in log] == ["hmc_box"] * 6 and [e[1][2] for e in log] == [3, 2, 8, 3, 2, 8]
    assert lap == [[1], [2]]
    lo, hi = BR.bounds_arrays(a.bounds)
    kind = BR.box_kinds(lo, hi)
    assert len(a.bounds) == LB.ND + 2 and list(kind[:3]) + list(kind[-2:]) == [3, 1, 0, 2, 3]
    # the first start: rung 1's minimisers, the entries on or outside a bound pulled inside
    src = a._mp[:, 1]
    start = np.concatenate([src[:, :LB.ND], src[:, LB.ND:][:, a._estpos]], axis=1)
    low, high = start <= lo, start >= hi
    assert low.any() or high.any()                                                # (the canned minimisers do cross the bounds)
    step = np.where(kind == 3, 1e-6 * (hi - np.where(kind == 3, lo, 0.0)), 1e-6 * np.maximum(1.0, np.abs(np.where(kind == 1, lo, np.where(kind == 2, hi, 0.0)))))
    want = np.where(low, lo + step, np.where(high, hi - step, start))
    assert np.array_equal(log[0][1][0], want) and np.all(want > lo) and np.all(want < hi)
    assert np.array_equal(lead(r["n_pulled_in"]), np.stack([(low | high).sum(axis=1), np.zeros(a.B, np.int64)], axis=1))
    # every call gets the annealer's bounds; z is None once, then the z the call before returned, with its x
    for e in log:
        assert e[2]["bounds"] is a.bounds
    assert log[0][2]["z0"] is None
    for c in range(1, 6):
        assert np.array_equal(log[c][2]["z0"], np.full((a.B, LB.ND + 2), 0.25 * c))
        assert np.array_equal(log[c][1][0], 0.5 * log[c - 1][1][0] + 0.125 * c)
    # masses of z: the Laplace variances over the slope squared, at the pulled-in start and at rung 2's start in z
    var = np.concatenate([np.full((a.B, LB.ND), 4.0), np.full((a.B, 2), 9.0)], axis=1)
    for calls, z in ((log[:3], BR.box_inverse(kind, lo, hi, want)), (log[3:], np.full((a.B, LB.ND + 2), 0.75))):
        slope = BR.box_map(kind, lo, hi, z)[1]
        for e in calls:
            assert np.array_equal(e[2]["minv"], var / (slope * slope))           # (va_ode's transcription of the map: the reference's bits)
    assert r["mass_note"] == [None, None]
    # warm-up rescaling, sampling call's extras, seeds all different
    assert np.array_equal(log[1][1][4], va_ode.hmc_rescale_step(log[0][1][4], np.full(a.B, 1.0 / 3.0)))
    assert log[2][2]["thin"] == 2 and len(log[2][2]["keep_idx"]) == LB.D + 2 and "thin" not in log[0][2]
    assert len({e[2]["seed"] for e in log}) == 6
    assert lead(r["x_last"]).shape == (a.B, 2, 4, LB.D) and lead(r["params"]).shape == (a.B, 2, 4, 2)
    assert np.array_equal(lead(r["x"])[:, 1], 0.5 * log[5][1][0] + 0.125 * 6)
    a.close()


def test_identity_fallback_is_not_converted(sampling):
    a = _annealed(BOUNDS)

    def refuses(beta):
        raise NotImplementedError("no factor")
    a.laplace = refuses
    a._pb.log[:] = []
    r = a.sample(2, beta=-1, n_leap=3, mass='laplace')
    assert [e[0] for e in a._pb.log] == ["hmc_box"] and a._pb.log[0][2]["minv"] is None
    assert "identity mass: laplace() refused" in r["mass_note"][0]
    a.close()


def test_a_conversion_that_is_not_finite_falls_back_with_a_note(sampling):
    """a Laplace variance so large that var / (dx/dz)^2 overflows at seed 1's start: that seed runs at identity, and says so"""
    a = _annealed(BOUNDS)

    def laplace(beta):
        sv = np.full((a.B, 1, LB.ND), 4.0)
        sv[1, 0, 0] = 1e308
        return dict(state_var=sv, param_cov=np.tile(9.0 * np.eye(2), (a.B, 1, 1, 1)))
    a.laplace = laplace
    a._pb.log[:] = []
    r = a.sample(2, beta=1, n_leap=3, mass='laplace')
    minv = a._pb.log[0][2]["minv"]
    assert np.all(minv[1] == 1.0) and not np.any(minv[0] == 1.0) and np.all(np.isfinite(minv))
    assert "identity mass for seed(s) [1]" in r["mass_note"][0] and "(dx/dz)^2" in r["mass_note"][0]
    a.close()


def test_unbounded_annealer_still_calls_hmc_as_before(sampling):
    a = _annealed(None)
    lap = []
    a.laplace = _laplace(a, lap)
    a._pb.log[:] = []
    r = a.sample(4, beta=[1, 2], n_leap=3, warmup=5, warmup_block=3, thin=2, seed=7, mass='laplace')
    log = a._pb.log
    assert [e[0] for e in log] == ["hmc"] * 6 and [e[1][2] for e in log] == [3, 2, 8, 3, 2, 8]
    src = a._mp[:, 1]
    assert np.array_equal(log[0][1][0], np.concatenate([src[:, :LB.ND], src[:, LB.ND:][:, a._estpos]], axis=1))
    var = np.concatenate([np.full((a.B, LB.ND), 4.0), np.full((a.B, 2), 9.0)], axis=1)
    golden = 0x9E3779B97F4A7C15
    for c, e in enumerate(log):
        assert sorted(e[2]) == (["jitter", "keep_idx", "minv", "seed", "thin"] if c % 3 == 2 else ["jitter", "minv", "seed"])
        assert e[2]["jitter"] == 0.1 and np.array_equal(e[2]["minv"], var) and e[2]["seed"] == (7 + golden * (c + 1)) & (2 ** 64 - 1)
        assert e[1][1] == float(a._rf_scale[1 + c // 3]) and e[1][3] == 3
        if c:
            assert np.array_equal(e[1][0], 0.5 * log[c - 1][1][0] + 0.125 * c)
    assert np.array_equal(log[0][1][4], np.full(a.B, float(LB.ND + 2) ** -0.25))
    assert "n_pulled_in" not in r and r["mass_note"] == [None, None]
    a.close()
