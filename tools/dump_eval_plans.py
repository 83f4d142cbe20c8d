"""The grid of problems the evaluation kernels' chooser is recorded on (tests/golden/eval_plans.txt), and what a
built library answers for it through the C-ABI.  No GPU call.

    python tools/dump_eval_plans.py --grid                     the grid: one problem per line, the 20 integers
                                                               tests/cpu_emul/plan_check.cpp reads
    python tools/dump_eval_plans.py --lib PATH                 va_eval_plan_reach's four integers (kernel, disc, K, W)
                                                               per problem of the grid

Regenerating the golden file (only when the chooser is meant to change):
    g++ -std=c++17 -O1 -I varanneal_amd/csrc -o plan_check tests/cpu_emul/plan_check.cpp
    python tools/dump_eval_plans.py --grid | ./plan_check > tests/golden/eval_plans.txt
Two libraries choose alike when their --lib outputs are byte-identical.
"""
import argparse
import ctypes as C
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIELDS = ("D", "N", "B", "disc", "rm_kind", "rf_kind", "nskip", "L", "tile_rows", "eval_kernel", "bounds", "tdp", "rhs", "lin",
          "ne", "ghost", "xl", "xr", "gl", "gr")
DS = (4, 5, 8, 14, 16, 20, 24, 32, 64, 66, 100, 128, 200, 226, 450, 512, 1000, 1024, 1026, 2000)
NS = (33, 161, 1001, 5001)                       # odd: Simpson-Hermite is legal
BS = (1, 8, 64, 1024, 4096)
WEIGHTS = ((0, 0), (1, 0), (0, 1), (2, 0), (0, 2))         # (rm_kind, rf_kind): scalar, RM array, RF array, full RM, full RF
USER = 1000                                      # VA_RHS_USER_BASE: any generated module
NONE = (-1, -1, -1, -1)
L96 = (2, 1, 1, 2)
# (ne, ghost, reaches): no form; a column form of 4 / of 8 products; a ghosted form alone; the built-in's forms with its
# reaches; reaches too long for tile5_ok; long gather reaches (the products change lanes through LDS, not DPP shifts)
FORMS = ((0, 0, NONE), (4, 0, NONE), (8, 2, NONE), (0, 2, NONE), (2, 2, L96), (2, 2, (30, 30, 2, 2)), (4, 2, (2, 1, 3, 3)))


def row(D, N, B, disc=1, w=(0, 0), nskip=1, L=None, tile_rows=0, ek=0, bounds=0, tdp=0, rhs=0, lin=0, form=FORMS[4]):
    return (D, N, B, disc, w[0], w[1], nskip, D // 2 if L is None else L, tile_rows, ek, bounds, tdp, rhs, lin,
            form[0], form[1]) + tuple(form[2])


def grid():
    rows = []
    # the benchmark's shapes (bench.py WORKLOADS: c3, c4, c2 and the widths between; L = 7 / 80 as BASELINE has them)
    for D, N, B, L in ((20, 1000, 64, 7), (200, 5000, 64, 80), (20, 1000, 1, 7), (20, 200, 1, 7), (100, 5000, 64, 40), (300, 3000, 64, 120),
                       (500, 2000, 64, 200), (900, 1000, 64, 360), (20, 1000, 256, 7), (20, 1000, 1024, 7), (20, 1000, 4096, 7)):
        for disc in range(4):
            if disc != 2 or N % 2:
                rows.append(row(D, N, B, disc=disc, L=L))
    # every size, every form, every kernel asked for; the other axes drawn sparsely (seeded: the grid is one fixed list)
    rnd = random.Random(20240)
    k = 0
    for D in DS:
        for N in NS:
            for B in BS:
                for form in (FORMS[k % len(FORMS)], FORMS[(k + 3) % len(FORMS)]):
                    rows.append(row(D, N, B, disc=rnd.randrange(4), w=rnd.choice(WEIGHTS[:3] * 3 + WEIGHTS[3:]), nskip=rnd.choice((1, 1, 2)),
                                    L=rnd.choice((1, D // 2, D)), tile_rows=rnd.choice((0, 0, 0, 7, 40, 200)), ek=rnd.randrange(6),
                                    bounds=int(rnd.random() < 0.1), tdp=int(rnd.random() < 0.1), rhs=rnd.choice((0, USER)),
                                    lin=int(form[0] == 0 and rnd.random() < 0.5), form=form))
                k += 1
    # the automatic choice on plain problems: every size, scalar weights, built-in and generated
    for D in DS:
        for N in NS:
            for B in BS:
                rows.append(row(D, N, B, disc=1 + (D // 2 + N // 2 + B) % 2, rhs=USER if (D + N + B) % 3 == 0 else 0))
    # k_eval4's run lengths: D = 20 (the one width with runs of 12 rows) and its neighbours, weights x tile_rows x model
    for D in (16, 20, 32):
        for N in (161, 1001, 5001):
            for B in (8, 64, 1024, 4096):
                for disc in (1, 2):
                    for w in WEIGHTS[:3]:
                        for nskip in (1, 2):
                            for rhs in (0, USER):
                                for tr in (0, 7, 40, 200, 250):
                                    if (D // 4 + N // 2 + B // 8 + disc + w[0] + 2 * w[1] + nskip + rhs // 1000 + tr // 5) % (4 if D == 20 else 16) == 0:
                                        rows.append(row(D, N, B, disc=disc, w=w, nskip=nskip, tile_rows=tr, rhs=rhs,
                                                        form=FORMS[2] if tr == 7 else FORMS[4]))
    # column forms with many products per element: k_eval4 shortens its runs until two workgroups share a CU
    for D in (16, 20, 32, 64):
        for ne in (8, 16, 24):
            for disc in (1, 2):
                for B in (64, 4096):
                    rows.append(row(D, 1001, B, disc=disc, rhs=USER, form=(ne, 2, NONE)))
    # k_eval3's staging arrays against the LDS, and wide ghost margins
    for D in (64, 100, 200, 512, 1000, 1024):
        for ghost in (2, 24):
            for disc in (1, 2):
                for tr in (0, 200):
                    rows.append(row(D, 5001, 64, disc=disc, ek=3, tile_rows=tr, rhs=USER, form=(0, ghost, NONE)))
    # k_eval5: observation strips (few, half, all columns observed), segment counts, ring depth with and without weight arrays
    for D in (66, 200, 450, 2000):
        for L in (1, 2, D // 2, D - 1, D):
            for w in WEIGHTS[:3]:
                rows.append(row(D, 1001, 8, w=w, L=L, tile_rows=40 * (w[0] + (L & 1)), ek=5, disc=1 + (L & 1)))
    # (every column observed twice, which no handle accepts: the one way to k_eval5's refusal of over-long observation rows)
    for ek in (0, 5):
        rows.append(row(200, 1001, 8, L=400, ek=ek))
    # the flat kernel's tile: with and without the dense linear part, with a run length asked for
    for D in (4, 20, 100, 200, 1000, 2000, 6000):
        for lin in (0, 1):
            for tr in (0, 7, 40, 200):
                rows.append(row(D, 1001, 8, disc=1 + (tr == 7), tile_rows=tr, rhs=USER, lin=lin, form=FORMS[0]))
                rows.append(row(D, 33, 4096, disc=1 + (tr == 40), tile_rows=tr, rhs=USER, lin=lin, form=FORMS[0]))
    # the built-in problems a handle is created for on the GPU (tests/test_gpu_eval_plan.py): small, every kernel asked for
    for D in (8, 20, 200, 101):
        for ek in (0, 1, 3, 4, 5):
            rows.append(row(D, 161, 8, ek=ek))
            rows.append(row(D, 161, 8, ek=ek, disc=2, tile_rows=40))
    rows += [row(20, 161, 8, nskip=2, tile_rows=200), row(20, 161, 64, disc=2)]
    seen, out = set(), []
    for r in rows:
        if r not in seen:
            seen.add(r)
            out.append(r)
    return out


def ask(lib, rows, out):
    """va_eval_plan_reach per row (the C-ABI carries no `lin`: it only shapes the flat kernel's tile)"""
    from varanneal_amd._capi import ProblemDesc, c_dp, c_ip
    import numpy as np
    L = C.CDLL(lib)
    L.va_eval_plan_reach.argtypes = [C.POINTER(ProblemDesc), C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.va_last_error.restype = C.c_char_p
    dummy = (C.c_double * 1)()
    for r in rows:
        v = dict(zip(FIELDS, r))
        d = ProblemDesc()
        d.struct_size = C.sizeof(ProblemDesc)
        d.D, d.N_model, d.batch, d.disc, d.rm_kind, d.rf_kind = v["D"], v["N"], v["B"], v["disc"], v["rm_kind"], v["rf_kind"]
        d.merr_nskip, d.L, d.tile_rows, d.eval_kernel = v["nskip"], v["L"], v["tile_rows"], v["eval_kernel"]
        d.N_data = (v["N"] - 1) // v["nskip"] + 1
        d.p_time_dependent, d.rhs = v["tdp"], v["rhs"]
        if v["bounds"]:
            d.lower = C.cast(dummy, c_dp)
            d.upper = C.cast(dummy, c_dp)
        li = np.ascontiguousarray([l * v["D"] // v["L"] for l in range(v["L"])], dtype=np.int32)
        d.Lidx = li.ctypes.data_as(c_ip)
        reach = (C.c_int32 * 4)(v["xl"], v["xr"], v["gl"], v["gr"]) if v["xl"] >= 0 else None
        res = (C.c_int32 * 4)()
        rc = L.va_eval_plan_reach(C.byref(d), v["ne"], v["ghost"], reach, res)
        if rc:
            raise RuntimeError("va_eval_plan_reach: %d %s" % (rc, L.va_last_error()))
        out.write("%s -> %d %d %d %d\n" % (" ".join(str(x) for x in r), res[0], res[1], res[2], res[3]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", action="store_true")
    ap.add_argument("--lib")
    a = ap.parse_args()
    rows = grid()
    if a.grid:
        for r in rows:
            print(" ".join(str(x) for x in r))
    elif a.lib:
        ask(os.path.abspath(a.lib), rows, sys.stdout)
    else:
        ap.error("--grid or --lib PATH")
