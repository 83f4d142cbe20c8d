// shoot_box_check.cpp -- CPU check of the boxed shooting kernel (csrc/va_shoot_box.h, csrc/va_shoot_geo.h: the headers the
// kernel and the host include).  Test infrastructure only (tests/test_shoot_box_cpu.py).
//   shoot_box_check geo NP NPest m D0 D1   -> per D in [D0, D1], planned for T = 7: "OK D RW threads E wave lds_bytes grid n
//        point_doubles sRW sthreads sE swave slds sgrid" (s*: plan_shoot's own figures) | "NO D reason"
//   shoot_box_check run D T n_steps dt m maxiter maxfun maxls ftol gtol in out -> Lorenz-96 through shoot_box_host (the
//        kernel's phases, lane by lane): `in` holds shoot_check's text (T*D start values, T forcings, L, the L observed
//        columns, L weights, T*n_out*L observations), then box_shared (0 | 1) and lower, upper: n = D + 1 values each when
//        shared, T*n otherwise ("-inf" / "inf": no bound); `out` receives x0 (T*D), k (T), cost, cost_start, grad_max, nit,
//        nfev, status (T each) as raw doubles.  Prints "RW threads E wave lds_bytes grid".  Exit 3 with the reason on
//        stderr for refused options and bounds.  The workspace is allocated to the planned size exactly, so that a
//        sanitizer build of a one-point run sees an overrun of the packed layout.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "va_shoot_box.h"

int main(int argc, char **argv)
{
    if (argc == 7 && !strcmp(argv[1], "geo")) {
        const int NP = atoi(argv[2]), NPest = atoi(argv[3]), m = atoi(argv[4]);
        for (int D = atoi(argv[5]); D <= atoi(argv[6]); ++D) {
            va::ShootGeo g, s;
            if (!va::plan_shoot_box(D, 7, NP, NPest, 0, m, g)) { printf("NO %d %s\n", D, g.why); continue; }
            if (!va::plan_shoot(D, 7, NP, NPest, 0, m, s)) { printf("NO %d plan_shoot: %s\n", D, s.why); continue; }
            printf("OK %d %d %d %d %d %zu %ld %d %zu %d %d %d %d %zu %ld\n", D, g.adj.RW, g.adj.threads, g.adj.E, g.adj.wave, g.lds_bytes,
                   g.adj.grid, g.n, g.point_doubles, s.adj.RW, s.adj.threads, s.adj.E, s.adj.wave, s.lds_bytes, s.adj.grid);
        }
        return 0;
    }
    if (argc != 14 || strcmp(argv[1], "run")) return 2;
    va::ShootBoxArgs ba{};
    va::ShootArgs &sa = ba.sh;
    va::PredictAdjArgs &a = sa.adj;
    a.D = atoi(argv[2]); a.T = atoi(argv[3]); a.ncot = 1; a.n_steps = atoi(argv[4]); a.substeps = 1; a.every = 1; a.dt = atof(argv[5]);
    a.t0 = 0.0; a.NP = va::RhsL96::NP; a.NPest = 1; a.nstim = 0; a.stim = nullptr; a.n_out = a.n_steps + 1;
    sa.m = atoi(argv[6]); sa.maxiter = atoll(argv[7]); sa.maxfun = atoll(argv[8]); sa.maxls = atoi(argv[9]);
    sa.ftol = atof(argv[10]); sa.gtol = atof(argv[11]);
    char why[192];
    if (!va::shoot_check_args(sa.m, sa.maxiter, sa.maxfun, sa.maxls, why, sizeof why)) { fprintf(stderr, "refused: %s\n", why); return 3; }
    va::ShootGeo geo;
    if (!va::plan_shoot_box(a.D, a.T, a.NP, a.NPest, a.nstim, sa.m, geo)) { fprintf(stderr, "refused: %s\n", geo.why); return 3; }
    a.geo = geo.adj;
    const size_t T = (size_t)a.T, n = (size_t)geo.n;
    std::vector<double> x(T * a.D), p(T), Y, w, gx0(T * a.D, -1.0), gp(T, -1.0), cost(T, 0.0),
        ckpt(va::predict_adj_ckpt_doubles(a.geo, a.D, va::predict_adj_q(a)), -1.0), work(T * geo.point_doubles, -1.0), lower, upper;
    std::vector<va::ShootBoxState> st(T);
    std::vector<int> lidx;
    FILE *fh = fopen(argv[12], "r");
    if (!fh) return 4;
    for (double &v : x) if (fscanf(fh, "%lf", &v) != 1) return 5;
    for (double &v : p) if (fscanf(fh, "%lf", &v) != 1) return 5;
    if (fscanf(fh, "%d", &a.L) != 1 || a.L < 0 || a.L > a.D) return 5;
    lidx.resize(a.L); w.resize(a.L);
    for (int &v : lidx) if (fscanf(fh, "%d", &v) != 1) return 5;
    for (double &v : w) if (fscanf(fh, "%lf", &v) != 1) return 5;
    Y.resize(T * a.n_out * a.L);
    for (double &v : Y) if (fscanf(fh, "%lf", &v) != 1) return 5;
    if (fscanf(fh, "%d", &ba.box_shared) != 1) return 5;
    const size_t nb = ba.box_shared ? n : T * n;
    lower.resize(nb); upper.resize(nb);
    for (double &v : lower) if (fscanf(fh, "%lf", &v) != 1) return 5;
    for (double &v : upper) if (fscanf(fh, "%lf", &v) != 1) return 5;
    fclose(fh);
    if (!va::shoot_box_check_bounds(lower.data(), upper.data(), ba.box_shared ? 1 : (long)T, (int)n, why, sizeof why)) {
        fprintf(stderr, "refused: %s\n", why);
        return 3;
    }
    const int pidx = 0;
    a.Y = Y.data(); a.w = w.data(); a.Lidx = lidx.data(); a.y_stride = (size_t)a.n_out * a.L; a.G = nullptr;
    a.x0 = x.data(); a.p = p.data(); a.Pidx = &pidx; a.out = nullptr; a.gx0 = gx0.data(); a.gp = gp.data(); a.cost = cost.data();
    a.ckpt = ckpt.data();
    sa.x = x.data(); sa.p = p.data(); sa.st = nullptr; sa.work = work.data(); sa.point_doubles = geo.point_doubles;
    ba.st = st.data(); ba.lower = lower.data(); ba.upper = upper.data();
    va::shoot_box_host<va::RhsL96>(ba);
    std::vector<double> res[6];
    for (const va::ShootBoxState &s : st) {
        res[0].push_back(s.f); res[1].push_back(s.f_start); res[2].push_back(s.gmax); res[3].push_back((double)s.iter);
        res[4].push_back((double)s.nfev); res[5].push_back((double)s.status);
    }
    fh = fopen(argv[13], "wb");
    if (!fh) return 6;
    if (fwrite(x.data(), sizeof(double), x.size(), fh) != x.size() || fwrite(p.data(), sizeof(double), p.size(), fh) != p.size()) return 7;
    for (const std::vector<double> &v : res)
        if (fwrite(v.data(), sizeof(double), v.size(), fh) != v.size()) return 7;
    fclose(fh);
    printf("%d %d %d %d %zu %ld\n", a.geo.RW, a.geo.threads, a.geo.E, a.geo.wave, geo.lds_bytes, a.geo.grid);
    return 0;
}
