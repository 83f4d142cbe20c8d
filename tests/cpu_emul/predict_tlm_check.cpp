// predict_tlm_check.cpp -- CPU check of the tangent-linear RK4 predictor (csrc/va_predict_tlm.h, csrc/va_predict_tlm_geo.h: the
// headers the kernel and the host include).  Test infrastructure only (tests/test_predict_tlm_cpu.py).
//   predict_tlm_check geo nvec D0 D1        -> per D in [D0, D1]: "OK D RW chunk nchunks threads E wave lds_bytes grid dxmin dxmax
//        outmin outmax nom" | "NO D reason", planned for T = 3, NP = 1: how many lanes predict_tlm_load gives every
//        (trajectory, direction, column) and every (trajectory, column) of the nominal output (1 and 1 when right), and whether
//        every workgroup carries the nominal columns of its live trajectories exactly once (nom = 1)
//   predict_tlm_check traj D T nvec n_steps substeps every dt in out -> Lorenz-96 through predict_tlm_host and spread_host (the
//        kernels' phases, lane by lane): `in` holds T*D start values, T forcings, T*nvec*(D+1) directions as text; `out`
//        receives out, dX, var, cov as raw doubles; a last argument "nocov" leaves cov out (wide states: T n_out D D doubles)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "va_predict_tlm.h"

template <int E>
static void cover(const va::PredictTlmArgs &a, std::vector<int> &ndx, std::vector<int> &nout, int *nom_ok)
{
    std::vector<double> mem(va::predict_tlm_lds_doubles(a.geo.RW, a.geo.chunk, a.D, a.NP, a.nstim) + 1, 0.0);
    const va::PredictTlmLds l = va::predict_tlm_lds(a, mem.data());
    for (long wg = 0; wg < a.geo.grid; ++wg) {
        const va::PredictTlmWork w = va::predict_tlm_work(a, wg);
        long live = (long)a.T - w.group * a.geo.RW;
        if (live > a.geo.RW) live = a.geo.RW;
        std::vector<int> nom((size_t)a.geo.RW * a.D, 0);
        for (int tid = 0; tid < a.geo.threads; ++tid) {
            va::PredictTlmLane<E> L;
            va::predict_tlm_load<E>(a, l, wg, tid, L);
            for (int e = 0; e < E; ++e) {
                const va::PredictTlmElem &el = L.el[e];
                if (el.kind == 2) ++ndx[el.g - a.dX];
                if (el.kind == 1) {
                    ++nom[(size_t)(el.noff / ((a.geo.chunk + 1) * a.D)) * a.D + el.col];
                    if (el.g) ++nout[el.g - a.out];
                }
            }
        }
        for (size_t k = 0; k < nom.size(); ++k)
            if (nom[k] != ((long)(k / a.D) < live ? 1 : 0)) *nom_ok = 0;
    }
}

int main(int argc, char **argv)
{
    if (argc == 5 && !strcmp(argv[1], "geo")) {
        const int nvec = atoi(argv[2]);
        for (int D = atoi(argv[3]); D <= atoi(argv[4]); ++D) {
            va::PredictTlmArgs a;
            a.T = 3; a.D = D; a.NP = 1; a.NPest = 1; a.nvec = nvec; a.nstim = 0; a.n_steps = 1; a.substeps = 1; a.every = 1; a.n_out = 1;
            a.t0 = 0.0; a.dt = 0.025; a.stim = nullptr;
            if (!va::plan_predict_tlm(D, a.T, nvec, a.NP, 0, a.geo)) { printf("NO %d %s\n", D, a.geo.why); continue; }
            const va::PredictTlmGeo &g = a.geo;
            std::vector<double> x0((size_t)a.T * D, 1.0), p(a.T, 8.0), V0((size_t)a.T * nvec * (D + 1), 0.5), out((size_t)a.T * D), dX((size_t)a.T * nvec * D);
            const int pidx = 0;
            a.x0 = x0.data(); a.p = p.data(); a.V0 = V0.data(); a.Pidx = &pidx; a.out = out.data(); a.dX = dX.data();
            std::vector<int> ndx(dX.size(), 0), nout(out.size(), 0);
            int nom_ok = 1;
            switch (g.E) {
            case 1: cover<1>(a, ndx, nout, &nom_ok); break;
            case 2: cover<2>(a, ndx, nout, &nom_ok); break;
            case 3: cover<3>(a, ndx, nout, &nom_ok); break;
            case 4: cover<4>(a, ndx, nout, &nom_ok); break;
            case 5: cover<5>(a, ndx, nout, &nom_ok); break;
            case 6: cover<6>(a, ndx, nout, &nom_ok); break;
            case 7: cover<7>(a, ndx, nout, &nom_ok); break;
            case 8: cover<8>(a, ndx, nout, &nom_ok); break;
            default: printf("NO %d E=%d outside 1..8\n", D, g.E); continue;
            }
            int lo = ndx[0], hi = ndx[0], olo = nout[0], ohi = nout[0];
            for (int v : ndx) { lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
            for (int v : nout) { olo = v < olo ? v : olo; ohi = v > ohi ? v : ohi; }
            printf("OK %d %d %d %d %d %d %d %zu %ld %d %d %d %d %d\n", D, g.RW, g.chunk, g.nchunks, g.threads, g.E, g.wave, g.lds_bytes, g.grid,
                   lo, hi, olo, ohi, nom_ok);
        }
        return 0;
    }
    const bool nocov = argc == 12 && !strcmp(argv[11], "nocov");
    if ((argc != 11 && !nocov) || strcmp(argv[1], "traj")) return 2;
    va::PredictTlmArgs a;
    a.D = atoi(argv[2]); a.T = atoi(argv[3]); a.nvec = atoi(argv[4]); a.n_steps = atoi(argv[5]); a.substeps = atoi(argv[6]);
    a.every = atoi(argv[7]); a.dt = atof(argv[8]); a.t0 = 0.0; a.NP = va::RhsL96::NP; a.NPest = 1; a.nstim = 0; a.stim = nullptr;
    a.n_out = a.n_steps / a.every + 1;
    if (!va::plan_predict_tlm(a.D, a.T, a.nvec, a.NP, a.nstim, a.geo)) { fprintf(stderr, "refused: %s\n", a.geo.why); return 3; }
    const size_t row = (size_t)a.n_out * a.D;
    std::vector<double> x0((size_t)a.T * a.D), p((size_t)a.T), V0((size_t)a.T * a.nvec * (a.D + 1)), out(a.T * row, -1.0),
        dX(a.T * a.nvec * row, -1.0), var(a.T * row, -1.0), cov(nocov ? 0 : a.T * row * a.D, -1.0);
    FILE *fh = fopen(argv[9], "r");
    if (!fh) return 4;
    for (double &v : x0) if (fscanf(fh, "%lf", &v) != 1) return 5;
    for (double &v : p) if (fscanf(fh, "%lf", &v) != 1) return 5;
    for (double &v : V0) if (fscanf(fh, "%lf", &v) != 1) return 5;
    fclose(fh);
    const int pidx = 0;
    a.x0 = x0.data(); a.p = p.data(); a.V0 = V0.data(); a.Pidx = &pidx; a.out = out.data(); a.dX = dX.data();
    va::predict_tlm_host<va::RhsL96>(a);
    va::SpreadArgs sa;
    sa.dX = dX.data(); sa.var = var.data(); sa.cov = nocov ? nullptr : cov.data(); sa.T = a.T; sa.nvec = a.nvec; sa.n_out = a.n_out; sa.D = a.D;
    va::spread_host(sa);
    fh = fopen(argv[10], "wb");
    if (!fh) return 6;
    for (const std::vector<double> *v : {&out, &dX, &var, &cov})
        if (fwrite(v->data(), sizeof(double), v->size(), fh) != v->size()) return 7;
    fclose(fh);
    printf("%d %d %d %d %d %d %zu %ld\n", a.geo.RW, a.geo.chunk, a.geo.nchunks, a.geo.threads, a.geo.E, a.geo.wave, a.geo.lds_bytes, a.geo.grid);
    return 0;
}
