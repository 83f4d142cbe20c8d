"""The grid of networks the network action's launch plan is recorded on (tests/golden/nnet_plans.txt).  No GPU call.

    python tools/dump_nnet_plans.py --grid          the grid: one network per line, the integers
                                                    tests/cpu_emul/nnet_plan_check.cpp reads

Regenerating the golden file (only when the plan is meant to change):
    g++ -std=c++17 -O1 -I varanneal_amd/csrc -o nnet_plan_check tests/cpu_emul/nnet_plan_check.cpp
    python tools/dump_nnet_plans.py --grid | ./nnet_plan_check > tests/golden/nnet_plans.txt
"""
import argparse

FIELDS = ("batch", "M", "ncu", "activation", "rm_matrix", "NPest_mode", "L_in", "L_out")
# what nnet_plan_check prints before the first '|'
SCALARS = ("NL", "NDnet", "nvar", "mch", "nmch", "n0", "n1", "n2", "n3", "n4", "nraw", "small", "wfsz", "nfb", "fb_ok", "fused",
           "fb_slots", "fold_rows", "nprow")
MS = (1, 5, 32, 33, 64, 70, 256, 257, 1000)
BS = (1, 8, 512)
NCUS = (256, 64)
USER = 1000                                      # VA_ACT_USER_BASE: any generated activation
ACTS = (0, 1, 2, 3, 4, USER)                     # sigmoid, tanh, linear, relu, softplus, generated
STRUCTURES = ((3, 4, 2), (16, 16),
              (32, 32, 32), (33, 8),             # the NN_SMALL edge
              (128, 128, 10), (129, 10),         # the NN_FB_W edge
              (784, 30, 10),
              (4,) * 65,                         # past NN_FB_LAYERS and NN_ROWS_DIRECT
              (64, 65, 64))                      # the tile edge


def row(batch, M, ncu, s, act=0, rm_matrix=0, npest_mode=1, L_in=None, L_out=None):
    return (batch, M, ncu, act, rm_matrix, npest_mode, max(1, s[0] // 2) if L_in is None else L_in,
            s[-1] if L_out is None else L_out) + tuple(s)


def grid():
    """Which inputs an integer of the plan depends on decides what is crossed with what.  The layer and job tables t1 / t2,
    n0..n4, nraw, small, the fragment offsets, nfb, fold_rows and nprow depend on the structure and M alone: every
    structure meets every M.  batch and the CU count enter twice: the doubling of mch, which only M = 1000 can reach
    (mch is 256 once M > 256 and doubles while 2 mch <= M), there iff tiles * batch >= 3 ncu; and `fused`, iff
    ceil(M / 32) * batch >= 2 ncu.  So each (structure, M) keeps ONE (batch, CU count) pair, drawn so that every structure
    and every M meets every pair, and at M = 1000 a structure of one tile and one of 64 keep all six, which puts both
    answers of both comparisons on either side of each CU count."""
    rows = []
    pairs = [(B, ncu) for B in BS for ncu in NCUS]
    every_pair = ((16, 16), (4,) * 65)
    # the activation, the measurement matrices and the estimated parameters are drawn in turn over the whole product
    k = -1
    for si, s in enumerate(STRUCTURES):
        for mi, M in enumerate(MS):
            for c, (B, ncu) in enumerate(pairs):
                k += 1
                if c == (si + mi) % 6 or (M == 1000 and s in every_pair):
                    rows.append(row(B, M, ncu, s, act=ACTS[k % 6], rm_matrix=int(k % 4 == 3), npest_mode=k % 3))
    # where the fused kernel is otherwise on: every activation, with and without matrices, on both chips
    for ncu in NCUS:
        for act in ACTS:
            for rm in (0, 1):
                rows.append(row(512, 64, ncu, (128, 128, 10), act=act, rm_matrix=rm))
    # observed neurons on one side only
    rows += [row(8, 70, 256, (3, 4, 2), L_in=0), row(8, 70, 256, (3, 4, 2), L_out=0), row(8, 70, 256, (784, 30, 10), L_in=784, L_out=1)]
    # more unknowns than 32-bit indexing carries: the one refusal these integers can express
    rows.append(row(1, 3000000, 256, (784, 30, 10), npest_mode=0))
    seen, out = set(), []
    for r in rows:
        if r not in seen:
            seen.add(r)
            out.append(r)
    return out


def parse(line):
    """one line of nnet_plan_check's output -> (dict of the scalars, {"t1": [tiles] or None when hashed, ...});
    (None, {}) for a refusal"""
    if line.startswith("refused"):
        return None, {}
    parts = [p.split() for p in line.split("|")]
    sc = dict(zip(SCALARS, (int(x) for x in parts[0])))
    tabs = {}
    for p in parts[3:]:
        n = int(p[1])
        tabs[p[0]] = None if n > 64 else [tuple(int(x) for x in p[2 + 10 * i:12 + 10 * i]) for i in range(n)]
    return sc, tabs


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", action="store_true")
    a = ap.parse_args()
    if not a.grid:
        ap.error("--grid")
    for r in grid():
        print(" ".join(str(x) for x in r))
