// hvp_check.cpp -- CPU check of the Hessian-vector kernel (csrc/va_hvp.h, csrc/va_hvp_geo.h: the headers the kernel and the
// host include).  Test infrastructure only (tests/test_hvp_cpu.py).  Built for the built-in Lorenz-96, or with
// -DVA_USER_RHS_HEADER='"header"' for a generated model (varanneal_amd/codegen.py).
//   hvp_check geo disc NP D...   -> per D: "OK D T ntiles Tmax lds_bytes grid(N=161, 61 products)" | "NO D maxD reason"
//   hvp_check hv file            -> hvp_host (the kernel's phases, thread by thread) on the problem in `file`:
//        D N disc nskip dt rf_scale gn tile_rows npts nvec NP NPest nstim has_t | L Lidx | Pidx | rm_kind rm.. | rf_kind rf..
//        | [t] | [stim] | X | P | V;  prints "T ntiles" then npts*nvec*ld values, one per line, round-trip exact
//   hvp_check fn file            -> the model's second-order functions at one point: D NP nstim | x v s | q p | t st;
//        prints jvp[D], vjp2[D], then sum_i pgrad2 [NP]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "va_hvp.h"
#ifdef VA_USER_RHS_HEADER
#include VA_USER_RHS_HEADER
typedef va::RhsUser Rhs;
#else
typedef va::RhsL96 Rhs;
#endif

static FILE *fh;
static double num() { double v; if (fscanf(fh, "%lf", &v) != 1) { fprintf(stderr, "short input\n"); exit(5); } return v; }
static void fill(std::vector<double> &a, size_t n) { a.resize(n); for (double &v : a) v = num(); }

int main(int argc, char **argv)
{
    if (argc >= 5 && !strcmp(argv[1], "geo")) {
        for (int i = 4; i < argc; ++i) {
            const int D = atoi(argv[i]);
            va::HvpGeo g;
            if (!va::plan_hvp(D, 161, atoi(argv[2]), atoi(argv[3]), 1, 61, 0, g)) { printf("NO %d %d %s\n", D, g.maxD, g.why); continue; }
            printf("OK %d %d %d %d %zu %ld\n", D, g.T, g.ntiles, g.Tmax, g.lds_bytes, g.grid);
        }
        return 0;
    }
    if (argc != 3) return 2;
    fh = fopen(argv[2], "r");
    if (!fh) return 4;
    if (!strcmp(argv[1], "fn")) {
        const int D = (int)num(), NP = (int)num(), nstim = (int)num();
        std::vector<double> x, v, s, q, p, st;
        fill(x, D); fill(v, D); fill(s, D); fill(q, NP > 0 ? NP : 1); fill(p, NP > 0 ? NP : 1);
        const double t = num();
        fill(st, nstim > 0 ? nstim : 1);
        if (NP != Rhs::NP) return 6;
        for (int i = 0; i < D; ++i) printf("%.17g\n", Rhs::jvp(x.data(), v.data(), q.data(), i, D, p.data(), t, st.data()));
        for (int j = 0; j < D; ++j) printf("%.17g\n", Rhs::vjp2(x.data(), s.data(), v.data(), q.data(), j, D, p.data(), t, st.data()));
        std::vector<double> acc(NP > 0 ? NP : 1, 0.0);
        for (int i = 0; i < D; ++i) Rhs::pgrad2(x.data(), s.data(), v.data(), q.data(), i, D, p.data(), t, st.data(), acc.data());
        for (int k = 0; k < NP; ++k) printf("%.17g\n", acc[k]);
        return 0;
    }
    if (strcmp(argv[1], "hv")) return 2;
    va::HvpArgs a;
    memset(&a, 0, sizeof a);
    va::Dims &dm = a.dm;
    dm.D = (int)num(); dm.N = (int)num(); dm.disc = (int)num(); dm.nskip = (int)num(); dm.dt = num();
    const double rf_scale = num();
    a.gn = (int)num();
    const int tile_rows = (int)num();
    a.npts = (int)num(); a.nvec = (int)num(); dm.NP = (int)num(); dm.NPest = (int)num();
    const int nstim = (int)num(), has_t = (int)num();
    if (dm.NP != Rhs::NP) { fprintf(stderr, "NP %d: the model has %d\n", dm.NP, Rhs::NP); return 6; }
    dm.NPt = dm.NP; dm.NPe = dm.NPest; dm.ND = dm.N * dm.D; dm.N_data = (dm.N - 1) / dm.nskip + 1;
    dm.L = (int)num();
    std::vector<int> lmap(dm.D, -1), pidx(dm.NPest);
    for (int l = 0; l < dm.L; ++l) lmap[(int)num()] = l;          // (ascending, as on the device)
    for (int &k : pidx) k = (int)num();
    std::vector<double> rm, rf, tm, stim, X, P, V;
    const int rm_kind = (int)num();
    if (rm_kind) fill(rm, (size_t)dm.N_data * dm.L); else dm.rm = num();
    const int rf_kind = (int)num();
    if (rf_kind) fill(rf, (size_t)(dm.N - 1) * dm.D); else dm.rf0 = num();
    if (has_t) fill(tm, dm.N);
    if (nstim) fill(stim, (size_t)dm.N * nstim);
    a.ld = dm.ND + dm.NPest;
    fill(X, (size_t)a.npts * a.ld); fill(P, (size_t)a.npts * dm.NP); fill(V, (size_t)a.npts * a.nvec * a.ld);
    fclose(fh);
    dm.cme = dm.L > 0 ? 1.0 / ((double)dm.L * dm.N_data) : 0.0;
    dm.cfe = 1.0 / ((double)dm.D * (dm.N - 1));
    a.c = 2.0 * rf_scale * dm.cfe;
    va::HvpGeo g;
    if (!va::plan_hvp(dm.D, dm.N, dm.disc, dm.NP, a.npts, a.nvec, tile_rows, g)) { fprintf(stderr, "refused: %s\n", g.why); return 3; }
    dm.T = g.T; dm.ntiles = g.ntiles;
    a.pp.lmap = lmap.data(); a.pp.Pidx = pidx.data(); a.pp.Pfull = P.data();
    a.pp.rm_arr = rm_kind ? rm.data() : nullptr; a.rm_ld = dm.L;
    a.pp.rf0_arr = rf_kind ? rf.data() : nullptr;
    a.pp.tmodel = has_t ? tm.data() : nullptr; a.pp.stim = nstim ? stim.data() : nullptr; a.pp.nstim = nstim;
    std::vector<double> HV((size_t)a.npts * a.nvec * a.ld, -777.0), part((size_t)a.npts * a.nvec * g.ntiles * (dm.NP ? dm.NP : 1), -777.0);
    a.X = X.data(); a.V = V.data(); a.HV = HV.data(); a.part = part.data();
    va::hvp_host<Rhs>(a);
    printf("%d %d\n", g.T, g.ntiles);
    for (double v : HV) printf("%.17g\n", v);
    return 0;
}
