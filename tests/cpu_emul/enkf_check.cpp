// enkf_check.cpp -- CPU check of the ensemble Kalman filter kernel (csrc/va_enkf.h, csrc/va_enkf_geo.h: the headers the kernel
// and the host include).  Test infrastructure only (tests/test_enkf_cpu.py).
//   enkf_check plan D M NP NQ nstim          -> "OK D M threads E wave pitch lds_bytes grid emin emax" | "NO D M reason", planned for
//        T = 3: how many lanes enkf_load gives every (member, column) of a point (1 and 1 when right)
//   enkf_check args T M NP NQ L n_obs obs_every substeps inflation est obs_var -> "OK" | "NO reason"
//        est: none | ok | out | neg | rep | null;  obs_var: ok | zero | neg | nan | inf | null
//   enkf_check run D T M NQ n_obs obs_every substeps dt t0 inflation in out -> Lorenz-96 through enkf_host (the kernel's
//        phases, lane by lane): `in` holds T*M*D start values, T*M forcings, T*n_obs*L observations (L = ceil(D / 2): every second
//        column) and L variances as raw doubles; NQ = 1 estimates the forcing; `out` receives mean_f, sd_f, mean_a, sd_a, x_end,
//        p_end, status (as doubles) as raw doubles
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "va_enkf.h"

template <int E>
static void cover(const va::EnkfArgs &a, std::vector<int> &nel)
{
    std::vector<double> mem(va::enkf_lds_doubles(a.M, a.D, a.NP, a.NQ, a.nstim) + 1, 0.0);
    const va::EnkfLds l = va::enkf_lds(a, mem.data());
    for (long wg = 0; wg < a.geo.grid; ++wg)
        for (int tid = 0; tid < a.geo.threads; ++tid) {
            va::EnkfLane<E> L;
            va::enkf_load<E>(a, l, wg, tid, L);
            for (int e = 0; e < E; ++e) {
                const va::EnkfElem &el = L.el[e];
                if (el.live) ++nel[((size_t)wg * a.M + el.xoff / a.geo.pitch) * a.D + el.col];
            }
        }
}

static void plan_line(int D, int M, int NP, int NQ, int nstim)
{
    va::EnkfArgs a = {};
    a.T = 3; a.D = D; a.M = M; a.NP = NP; a.NQ = NQ; a.nstim = nstim; a.n_obs = 1; a.obs_every = 1; a.substeps = 1; a.dt = 0.025;
    if (!va::plan_enkf(D, a.T, M, NP, NQ, nstim, a.geo)) { printf("NO %d %d %s\n", D, M, a.geo.why); return; }
    const va::EnkfGeo &g = a.geo;
    int lo = 1, hi = 1;
    if (nstim == 0) {
        std::vector<double> x0((size_t)a.T * M * D, 1.0), p((size_t)a.T * M * (NP ? NP : 1), 8.0);
        a.x0 = x0.data(); a.p = p.data();
        std::vector<int> nel((size_t)a.T * M * D, 0);
        switch (g.E) {
        case 1: cover<1>(a, nel); break;
        case 2: cover<2>(a, nel); break;
        case 3: cover<3>(a, nel); break;
        case 4: cover<4>(a, nel); break;
        case 5: cover<5>(a, nel); break;
        case 6: cover<6>(a, nel); break;
        case 7: cover<7>(a, nel); break;
        case 8: cover<8>(a, nel); break;
        default: printf("NO %d %d E=%d outside 1..8\n", D, M, g.E); return;
        }
        lo = hi = nel[0];
        for (int v : nel) { lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
    }
    printf("OK %d %d %d %d %d %d %zu %ld %d %d\n", D, M, g.threads, g.E, g.wave, g.pitch, g.lds_bytes, g.grid, lo, hi);
}

int main(int argc, char **argv)
{
    if (argc == 7 && !strcmp(argv[1], "plan")) { plan_line(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6])); return 0; }
    if (argc == 13 && !strcmp(argv[1], "args")) {
        const long T = atol(argv[2]);
        const int M = atoi(argv[3]), NP = atoi(argv[4]), NQ = atoi(argv[5]), L = atoi(argv[6]);
        std::vector<int> est((size_t)(NQ > 0 ? NQ : 1));
        for (int q = 0; q < NQ; ++q) est[q] = q;
        if (!strcmp(argv[11], "out")) est.back() = NP;
        if (!strcmp(argv[11], "neg")) est[0] = -1;
        if (!strcmp(argv[11], "rep") && NQ > 1) est[NQ - 1] = est[0];
        std::vector<double> ov((size_t)(L > 0 ? L : 1), 0.25);
        if (!strcmp(argv[12], "zero")) ov.back() = 0.0;
        if (!strcmp(argv[12], "neg")) ov[0] = -0.25;
        if (!strcmp(argv[12], "nan")) ov[ov.size() / 2] = std::numeric_limits<double>::quiet_NaN();
        if (!strcmp(argv[12], "inf")) ov[0] = std::numeric_limits<double>::infinity();
        char why[192] = "";
        const bool ok = va::enkf_check_args(T, M, NP, NQ, L, atoi(argv[7]), atoi(argv[8]), atoi(argv[9]), strcmp(argv[11], "null") ? est.data() : nullptr,
                                            strcmp(argv[12], "null") ? ov.data() : nullptr, atof(argv[10]), why, sizeof why);
        printf(ok ? "OK\n" : "NO %s\n", why);
        return 0;
    }
    if (argc != 14 || strcmp(argv[1], "run")) return 2;
    va::EnkfArgs a = {};
    a.D = atoi(argv[2]); a.T = atoi(argv[3]); a.M = atoi(argv[4]); a.NQ = atoi(argv[5]); a.n_obs = atoi(argv[6]); a.obs_every = atoi(argv[7]);
    a.substeps = atoi(argv[8]); a.dt = atof(argv[9]); a.t0 = atof(argv[10]); a.inflation = atof(argv[11]);
    a.NP = va::RhsL96::NP; a.nstim = 0; a.stim = nullptr; a.L = (a.D + 1) / 2;
    const int NV = a.D + a.NQ;
    std::vector<double> x0((size_t)a.T * a.M * a.D), p((size_t)a.T * a.M), Y((size_t)a.T * a.n_obs * a.L), ov((size_t)a.L);
    std::vector<int> est(1, 0), lidx((size_t)a.L);
    for (int j = 0; j < a.L; ++j) lidx[j] = 2 * j;
    FILE *fh = fopen(argv[12], "rb");
    if (!fh) return 4;
    for (std::vector<double> *v : {&x0, &p, &Y, &ov})
        if (v->size() && fread(v->data(), sizeof(double), v->size(), fh) != v->size()) return 5;
    fclose(fh);
    char why[192] = "";
    if (!va::enkf_check_args(a.T, a.M, a.NP, a.NQ, a.L, a.n_obs, a.obs_every, a.substeps, est.data(), ov.data(), a.inflation, why, sizeof why)) {
        fprintf(stderr, "bad arguments: %s\n", why);
        return 3;
    }
    if (!va::plan_enkf(a.D, a.T, a.M, a.NP, a.NQ, a.nstim, a.geo)) { fprintf(stderr, "refused: %s\n", a.geo.why); return 3; }
    const size_t ns = (size_t)a.T * a.n_obs * NV;
    std::vector<double> mf(ns, -1.0), sf(ns, -1.0), ma(ns, -1.0), sa(ns, -1.0), x_end(x0.size(), -1.0), p_end(p.size(), -1.0), stat((size_t)a.T);
    std::vector<int> status((size_t)a.T, -1);
    a.x0 = x0.data(); a.p = p.data(); a.Y = Y.data(); a.obs_var = ov.data(); a.est = est.data(); a.Lidx = lidx.data();
    a.mean_f = mf.data(); a.sd_f = sf.data(); a.mean_a = ma.data(); a.sd_a = sa.data(); a.x_end = x_end.data(); a.p_end = p_end.data();
    a.status = status.data();
    va::enkf_host<va::RhsL96>(a);
    for (int t = 0; t < a.T; ++t) stat[t] = (double)status[t];
    fh = fopen(argv[13], "wb");
    if (!fh) return 6;
    for (const std::vector<double> *v : {&mf, &sf, &ma, &sa, &x_end, &p_end, &stat})
        if (fwrite(v->data(), sizeof(double), v->size(), fh) != v->size()) return 7;
    fclose(fh);
    printf("%d %d %d %d %zu %ld\n", a.geo.threads, a.geo.E, a.geo.wave, a.geo.pitch, a.geo.lds_bytes, a.geo.grid);
    return 0;
}
