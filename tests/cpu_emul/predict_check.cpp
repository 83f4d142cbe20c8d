// predict_check.cpp -- CPU check of the RK4 predictor (csrc/va_predict.h, csrc/va_predict_geo.h: the headers the kernel and
// the host include).  Test infrastructure only (tests/test_predict_cpu.py).
//   predict_check geo D...                                  -> per D: "OK D RW threads E wave lds_bytes grid(T=7)" | "NO D reason"
//   predict_check traj D T n_steps substeps every dt file   -> Lorenz-96 through predict_host (the kernel's phases, lane by
//        lane): file holds T*D start values, then T forcings; prints T*n_out*D values, one per line, round-trip exact
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "va_predict.h"

int main(int argc, char **argv)
{
    if (argc >= 3 && !strcmp(argv[1], "geo")) {
        for (int i = 2; i < argc; ++i) {
            const int D = atoi(argv[i]);
            va::PredictGeo g;
            if (!va::plan_predict(D, 7, 1, 0, g)) { printf("NO %d %s\n", D, g.why); continue; }
            printf("OK %d %d %d %d %d %zu %ld\n", D, g.RW, g.threads, g.E, g.wave, g.lds_bytes, g.grid);
        }
        return 0;
    }
    if (argc != 9 || strcmp(argv[1], "traj")) return 2;
    va::PredictArgs a;
    a.D = atoi(argv[2]); a.T = atoi(argv[3]); a.n_steps = atoi(argv[4]); a.substeps = atoi(argv[5]); a.every = atoi(argv[6]);
    a.dt = atof(argv[7]); a.t0 = 0.0; a.NP = va::RhsL96::NP; a.nstim = 0; a.stim = nullptr;
    a.n_out = a.n_steps / a.every + 1;
    if (!va::plan_predict(a.D, a.T, a.NP, a.nstim, a.geo)) { fprintf(stderr, "refused: %s\n", a.geo.why); return 3; }
    std::vector<double> x0((size_t)a.T * a.D), p((size_t)a.T), out((size_t)a.T * a.n_out * a.D, -1.0);
    FILE *fh = fopen(argv[8], "r");
    if (!fh) return 4;
    for (double &v : x0) if (fscanf(fh, "%lf", &v) != 1) return 5;
    for (double &v : p) if (fscanf(fh, "%lf", &v) != 1) return 5;
    fclose(fh);
    a.x0 = x0.data(); a.p = p.data(); a.out = out.data();
    va::predict_host<va::RhsL96>(a);
    for (double v : out) printf("%.17g\n", v);
    return 0;
}
