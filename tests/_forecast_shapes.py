"""The lane geometries of the forecast kernels (k_predict, k_predict_tlm, k_predict_adj, k_shoot) as a table: per kernel the
shapes the suite runs and the plan (wave, threads, E, chunk, nchunks, RW) its planner (csrc/va_predict_geo.h,
va_predict_tlm_geo.h, va_predict_adj_geo.h, va_shoot_geo.h) must give each of them, worked out by hand from the planners'
rules.  tests/test_forecast_geometry_cpu.py holds the planners to it and runs the host emulations at every WIDE entry;
tests/test_gpu_forecast_geometry.py runs the kernels there.  The planner is the authority: where it disagrees, this table
is what gets corrected.

NARROW entries are the shapes of the older tests (test_predict*_cpu.py, test_gpu_predict*.py, test_shoot_cpu.py,
test_gpu_shoot_device.py); they stand here so that coverage is counted over all of it.  WIDE entries are the smallest shapes
that reach each remaining instantiation or edge.  Elements of a workgroup: D (predictor), (chunk + 1) D (tangent, adjoint,
shooting with chunk = 1); threads = min(256, elements rounded up to 64) past one wave; E = ceil(elements / threads).

An entry: (shape, plan, note).  shape is D (predictor), (D, nvec or ncot) (tangent and adjoint: one slot geometry) or
(D, points) (shooting); plan is (wave, threads, E, chunk, nchunks, RW), chunk and nchunks None for the predictor."""
import numpy as np

T = 3                               # trajectories of the WIDE predictor, tangent and adjoint entries

PREDICT_NARROW = [
    (5, (1, 64, 1, None, None, 12), "one wave, 12 trajectories side by side"),
    (20, (1, 64, 1, None, None, 3), "one wave, 3 side by side"),
    (64, (1, 64, 1, None, None, 1), "the wave filled"),
    (67, (0, 128, 1, None, None, 1), "first barrier form, idle lanes"),
    (200, (0, 256, 1, None, None, 1), "256 threads, idle lanes"),
]
PREDICT_WIDE = [
    (257, (0, 256, 2, None, None, 1), "E = 2, one live lane in the second pass"),
    (513, (0, 256, 3, None, None, 1), "E = 3, one live lane in the third pass"),
    (769, (0, 256, 4, None, None, 1), "E = 4, one live lane in the fourth pass"),
    (1024, (0, 256, 4, None, None, 1), "E = 4, every lane full"),
]

# tangent: nvec = D + 1 in the older tests; adjoint: their (D, ncot)
TLM_NARROW = [
    ((5, 6), (1, 64, 1, 6, 1, 1), "nominal and 6 directions in 35 lanes of a wave"),
    ((20, 21), (1, 64, 1, 2, 11, 1), "3 slots to a wave, 11 chunks, the last half full"),
    ((64, 65), (0, 256, 4, 13, 5, 1), "14 slots of 64: 896 elements"),
    ((67, 68), (0, 256, 4, 14, 5, 1), "15 slots of 67: 1005 elements, the last chunk with 12 directions"),
]
ADJ_NARROW = [
    ((5, 1), (1, 64, 1, 1, 1, 6), "one wave, six trajectories side by side"),
    ((20, 5), (1, 64, 1, 2, 3, 1), "chunks of 2, 2 and 1"),
    ((64, 3), (0, 256, 1, 3, 1, 1), "256 elements on 256 threads"),
    ((67, 3), (0, 256, 2, 3, 1, 1), "268 elements: E = 2"),
]
# one slot geometry for both: (D, nvec or ncot)
SLOTS_WIDE = [
    ((33, 2), (0, 128, 1, 2, 1, 1), "first barrier form: 99 elements on 128 threads, idle lanes"),
    ((100, 2), (0, 256, 2, 2, 1, 1), "300 elements: E = 2"),
    ((200, 2), (0, 256, 3, 2, 1, 1), "600 elements: E = 3"),
    ((300, 3), (0, 256, 4, 2, 2, 1), "900 elements: E = 4; chunks of 2 and 1, an idle slot in the last"),
    ((512, 2), (0, 256, 4, 1, 2, 1), "1024 elements: E = 4 with every lane full, one direction per workgroup"),
    ((513, 1), (0, 256, 5, 1, 1, 1), "1026 elements: E = 5"),
    ((700, 1), (0, 256, 6, 1, 1, 1), "1400 elements: E = 6"),
    ((800, 2), (0, 256, 7, 1, 2, 1), "1600 elements: E = 7, two workgroups per trajectory"),
    ((1024, 1), (0, 256, 8, 1, 1, 1), "2048 elements: E = 8 with every lane full"),
]

SHOOT_NARROW = [
    ((5, 7), (1, 64, 1, 1, 1, 6), "a wave of six points, one beside idle slots"),
    ((20, 7), (1, 64, 1, 1, 1, 1), "one wave per point"),
    ((33, 7), (0, 128, 1, 1, 1, 1), "128 threads with barriers"),
    ((130, 2), (0, 256, 2, 1, 1, 1), "260 elements: E = 2"),
]
SHOOT_WIDE = [
    ((300, 2), (0, 256, 3, 1, 1, 1), "600 elements: E = 3"),
    ((512, 2), (0, 256, 4, 1, 1, 1), "1024 elements: E = 4, the widest state the kernel takes"),
]

TABLE = {
    "k_predict": PREDICT_NARROW + PREDICT_WIDE,
    "k_predict_tlm": TLM_NARROW + SLOTS_WIDE,
    "k_predict_adj": ADJ_NARROW + SLOTS_WIDE,
    "k_shoot": SHOOT_NARROW + SHOOT_WIDE,
}

# the chunk shrink of the adjoint planner: Lorenz-96 with a forcing per site, D = NP = 40, 6 cotangent sets.  One set takes
# 2 * 40 + 40 * 41 = 1720 doubles beside the 200 of the nominal's images and the parameters, so 64 KiB = 8192 doubles hold
# 4 sets and not 5 (200 + 4 * 1720 = 7080, 200 + 5 * 1720 = 8800); 6 sets over ceil(6 / 4) = 2 workgroups are chunks of 3
# and 3: 160 elements on 192 threads
ADJ_SHRINK = dict(D=40, NP=40, ncot=6, plan=(0, 192, 1, 3, 2, 1), lds_bytes=8 * (200 + 3 * 1720))


def expected(kernel, shape):
    """the plan (wave, threads, E, chunk, nchunks, RW) the planner of `kernel` must give the table's entry `shape`"""
    for s, plan, _ in TABLE[kernel]:
        if s == shape:
            return plan
    raise KeyError((kernel, shape))


def directions(D, nvec):
    """the WIDE entries' directions (nvec, D + 1): mixed, a state part and a forcing part each"""
    return np.random.RandomState(7000 + D).randn(nvec, D + 1)
