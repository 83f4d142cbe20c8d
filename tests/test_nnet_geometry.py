"""CPU: the network action's launch plan (csrc/va_nnet_geo.h, the header the host includes), checked through a g++ build
of tests/cpu_emul/nnet_plan_check.cpp: over the grid of networks tools/dump_nnet_plans.py lists every integer of the
plan -- chunks, workgroup counts, the small / fused / folded paths, fragment offsets, the three job tables in the order
their workgroups meet the XCDs -- equals tests/golden/nnet_plans.txt line for line."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "nnet_plans.txt")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("nnplan") / "nnet_plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-I", os.path.join(ROOT, "varanneal_amd", "csrc"),
                           "-o", path, os.path.join(ROOT, "tests", "cpu_emul", "nnet_plan_check.cpp")])
    return path


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return fh.read().splitlines()


@pytest.fixture(scope="module")
def tool():
    import importlib.util
    spec = importlib.util.spec_from_file_location("dump_nnet_plans", os.path.join(ROOT, "tools", "dump_nnet_plans.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plans_equal_the_recorded_ones(exe, tool, golden):
    rows = "".join(" ".join(str(v) for v in r) + "\n" for r in tool.grid())
    out = subprocess.run([exe], input=rows, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = out.stdout.splitlines()
    assert len(got) == len(golden)
    for g, w in zip(got, golden):
        assert g == w


def test_the_grid_holds_every_axis_and_every_path(tool, golden):
    """every axis value, and every branch of the plan: the three sizes of `small`, k_nnet_fb fitting or not and on or off,
    folded partial rows or not, more than one example chunk, both orders of place()"""
    grid = tool.grid()
    assert len(grid) == len(golden) and 100 <= len(grid) <= 200
    assert [line for line in golden if line.startswith("refused")] == ["refused -4 n_var=2472000000 does not fit 32-bit indexing"]
    col = {name: set(r[k] for r in grid) for k, name in enumerate(tool.FIELDS)}
    assert col["batch"] == set(tool.BS) and col["M"] >= set(tool.MS) and col["ncu"] == set(tool.NCUS)
    assert col["activation"] == set(tool.ACTS) and max(tool.ACTS) >= 1000 and col["rm_matrix"] == {0, 1}
    assert col["NPest_mode"] == {0, 1, 2}
    assert set(r[8:] for r in grid) == set(tool.STRUCTURES)
    # each structure meets every M, and every (batch, CU count) pair; so does each M; where mch can double, a structure of
    # one tile and one of 64 meet every pair
    pairs = set((B, c) for B in tool.BS for c in tool.NCUS)
    assert set((r[1], r[8:]) for r in grid) >= set((M, s) for M in tool.MS for s in tool.STRUCTURES)
    for s in tool.STRUCTURES:
        assert set((r[0], r[2]) for r in grid if r[8:] == s) == pairs
    for M in tool.MS:
        assert set((r[0], r[2]) for r in grid if r[1] == M) == pairs
    for s in ((16, 16), (4,) * 65):
        assert set((r[0], r[2]) for r in grid if r[1] == 1000 and r[8:] == s) == pairs
    plans = [tool.parse(line) for line in golden]
    sc = [p[0] for p in plans if p[0] is not None]
    assert set(p["small"] for p in sc) == {0, 16, 32}
    assert set(p["fb_ok"] for p in sc) == {0, 1} and set(p["fused"] for p in sc) == {0, 1}
    assert set(p["fold_rows"] for p in sc) == {0, 1}
    assert any(p["nmch"] > 1 for p in sc)
    # batch and the CU count decide: mch doubled or not, k_nnet_fb on or off, on the same network with both chips
    by_net = {}
    for r, p in zip(grid, plans):
        if p[0] is not None and r[1] == 1000:
            by_net.setdefault(r[8:], set()).add((r[2], p[0]["mch"], p[0]["fused"]))
    for s in ((16, 16), (4,) * 65):
        assert set((c, m) for c, m, _ in by_net[s]) >= {(64, 256), (64, 512), (256, 256)}
    assert set((c, f) for c, _, f in by_net[(16, 16)]) >= {(64, 1), (64, 0), (256, 0)}
    assert all(p["nprow"] == (32 if p["fold_rows"] else p["nraw"]) for p in sc)
    # place(): eight families of equal width go member by member (the first two jobs are two row blocks of one column
    # tile); fewer than eight, or ragged ones, family by family (the first two jobs are two column tiles of one row block)
    first_two = {(r[1], r[8:]): p[1]["t1"][:2] for r, p in zip(grid, plans) if p[1].get("t1") is not None and len(p[1]["t1"]) >= 2}
    uniform = first_two[(1000, (128, 128, 10))]           # 16 row blocks x 2 column tiles
    assert uniform[0][1:3] == (0, 0) and uniform[1][1:3] == (64, 0)
    serial = first_two[(70, (128, 128, 10))]              # 2 row blocks
    assert serial[0][1:3] == (0, 0) and serial[1][1:3] == (0, 64)
