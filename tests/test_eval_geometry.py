"""CPU: the evaluation kernels' chooser (csrc/va_eval_geo.h, the header the host includes), checked through a g++ build of
tests/cpu_emul/plan_check.cpp: over the grid of problems tools/dump_eval_plans.py lists every integer it
produces -- kernel, tile, Geo4 / Geo5, observation strips, the key of the column-run instantiation -- equals
tests/golden/eval_plans.txt line for line."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "eval_plans.txt")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("plan") / "plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "varanneal_amd", "csrc"), "-o", path,
                           os.path.join(ROOT, "tests", "cpu_emul", "plan_check.cpp")])
    return path


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return fh.read().splitlines()


@pytest.fixture(scope="module")
def tool():
    import importlib.util
    spec = importlib.util.spec_from_file_location("dump_eval_plans", os.path.join(ROOT, "tools", "dump_eval_plans.py"))
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


def test_the_grid_holds_every_axis_and_every_fallback(tool, golden):
    """every axis value, the benchmark's shapes, every kernel chosen and every kernel asked for and refused"""
    grid = tool.grid()
    assert len(grid) == len(golden) and 2000 <= len(grid) <= 6000
    col = {name: set(r[k] for r in grid) for k, name in enumerate(tool.FIELDS)}
    assert col["D"] >= set(tool.DS) and col["N"] >= set(tool.NS) and col["B"] >= set(tool.BS)
    assert col["disc"] == {0, 1, 2, 3} and col["eval_kernel"] == {0, 1, 2, 3, 4, 5} and col["nskip"] == {1, 2}
    assert col["rm_kind"] == {0, 1, 2} and col["rf_kind"] == {0, 1, 2} and col["tile_rows"] >= {0, 7, 40, 200}
    assert col["bounds"] == {0, 1} and col["tdp"] == {0, 1} and col["lin"] == {0, 1} and col["rhs"] == {0, tool.USER}
    assert col["ne"] >= {0, 4, 8} and col["ghost"] >= {0, 2} and col["xl"] >= {-1, 2, 30}
    for D, N, B, L in ((20, 1000, 64, 7), (200, 5000, 64, 80), (20, 1000, 1, 7), (20, 200, 1, 7)):      # bench.py: c3, c4, c2, c1
        assert tool.row(D, N, B, L=L) in grid
    emode = [int(line.split()[0]) for line in golden]
    assert set(emode) == {1, 3, 4, 5}
    for asked in (3, 4, 5):
        assert any(r[9] == asked and e != asked for r, e in zip(grid, emode))
