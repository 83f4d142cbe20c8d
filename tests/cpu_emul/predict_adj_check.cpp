// predict_adj_check.cpp -- CPU check of the adjoint RK4 predictor (csrc/va_predict_adj.h, csrc/va_predict_adj_geo.h: the headers
// the kernel and the host include).  Test infrastructure only (tests/test_predict_adj_cpu.py).
//   predict_adj_check geo ncot NP D0 D1      -> per D in [D0, D1]: "OK D RW chunk nchunks threads E wave lds_bytes grid gxmin gxmax
//        outmin outmax nom" | "NO D reason", planned for T = 3 and NP parameters: how many lanes predict_adj_load gives every
//        (trajectory, cotangent set, column) of gx0 and every (trajectory, column) of the nominal output (1 and 1 when right),
//        and whether every workgroup carries the nominal columns of its live trajectories exactly once with checkpoints of
//        their own inside the checkpoint buffer (nom = 1)
//   predict_adj_check traj D T ncot n_steps substeps every dt mode in out -> Lorenz-96 through predict_adj_host (the kernel's
//        phases, lane by lane): `in` holds T*D start values, T forcings, then mode 0: T*ncot*n_out*D cotangents; mode 1 / 2:
//        L, the L observed columns, L weights and T*n_out*L (1) or n_out*L (2: shared) observations, as text; `out` receives
//        out, gx0, gp, cost (T values, zeros in mode 0) as raw doubles
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "va_predict_adj.h"

template <int E>
static void cover(const va::PredictAdjArgs &a, size_t nck, std::vector<int> &ngx, std::vector<int> &nout, int *nom_ok)
{
    std::vector<double> mem(va::predict_adj_lds_doubles(a.geo.RW, a.geo.chunk, a.D, a.NP, a.nstim) + 1, 0.0);
    const va::PredictAdjLds l = va::predict_adj_lds(a, mem.data());
    std::vector<int> ck(nck, 0);
    for (long wg = 0; wg < a.geo.grid; ++wg) {
        const va::PredictAdjWork w = va::predict_adj_work(a, wg);
        long live = (long)a.T - w.group * a.geo.RW;
        if (live > a.geo.RW) live = a.geo.RW;
        std::vector<int> nom((size_t)a.geo.RW * a.D, 0);
        for (int tid = 0; tid < a.geo.threads; ++tid) {
            va::PredictAdjLane<E> L;
            va::predict_adj_load<E>(a, l, wg, tid, L);
            for (int e = 0; e < E; ++e) {
                const va::PredictAdjElem &el = L.el[e];
                if (el.kind == 2) ++ngx[el.o - a.gx0];
                if (el.kind == 1) {
                    ++nom[(size_t)(el.noff / a.D) * a.D + el.col];
                    if (el.o) ++nout[el.o - a.out];
                    const size_t at = (size_t)(el.ck - a.ckpt);
                    if (at + (size_t)(va::predict_adj_q(a) - 1) * a.D >= nck || ck[at]++) *nom_ok = 0;
                }
            }
        }
        for (size_t k = 0; k < nom.size(); ++k)
            if (nom[k] != ((long)(k / a.D) < live ? 1 : 0)) *nom_ok = 0;
    }
}

int main(int argc, char **argv)
{
    if (argc == 6 && !strcmp(argv[1], "geo")) {
        const int ncot = atoi(argv[2]), NP = atoi(argv[3]);
        for (int D = atoi(argv[4]); D <= atoi(argv[5]); ++D) {
            va::PredictAdjArgs a{};
            a.T = 3; a.D = D; a.NP = NP; a.NPest = NP ? 1 : 0; a.ncot = ncot; a.n_steps = 2; a.substeps = 1; a.every = 1; a.n_out = 3;
            a.dt = 0.025;
            if (!va::plan_predict_adj(D, a.T, ncot, a.NP, 0, a.geo)) { printf("NO %d %s\n", D, a.geo.why); continue; }
            const va::PredictAdjGeo &g = a.geo;
            const size_t nck = va::predict_adj_ckpt_doubles(g, D, va::predict_adj_q(a));
            std::vector<double> x0((size_t)a.T * D, 1.0), p((size_t)a.T * (NP ? NP : 1), 8.0), G((size_t)a.T * ncot * a.n_out * D, 0.5),
                out((size_t)a.T * a.n_out * D), gx0((size_t)a.T * ncot * D), gp((size_t)a.T * ncot), ckpt(nck);
            const int pidx = 0;
            a.x0 = x0.data(); a.p = p.data(); a.G = G.data(); a.Pidx = &pidx; a.out = out.data(); a.gx0 = gx0.data(); a.gp = gp.data();
            a.ckpt = ckpt.data();
            std::vector<int> ngx(gx0.size(), 0), nout(out.size(), 0);
            int nom_ok = 1;
            switch (g.E) {
            case 1: cover<1>(a, nck, ngx, nout, &nom_ok); break;
            case 2: cover<2>(a, nck, ngx, nout, &nom_ok); break;
            case 3: cover<3>(a, nck, ngx, nout, &nom_ok); break;
            case 4: cover<4>(a, nck, ngx, nout, &nom_ok); break;
            case 5: cover<5>(a, nck, ngx, nout, &nom_ok); break;
            case 6: cover<6>(a, nck, ngx, nout, &nom_ok); break;
            case 7: cover<7>(a, nck, ngx, nout, &nom_ok); break;
            case 8: cover<8>(a, nck, ngx, nout, &nom_ok); break;
            default: printf("NO %d E=%d outside 1..8\n", D, g.E); continue;
            }
            // (row 0 of every output column: the rows below it follow at the pitch D)
            int lo = ngx[0], hi = ngx[0], olo = nout[0], ohi = nout[0];
            for (int v : ngx) { lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
            for (int t = 0; t < a.T; ++t)
                for (int i = 0; i < D; ++i) { const int v = nout[(size_t)t * a.n_out * D + i]; olo = v < olo ? v : olo; ohi = v > ohi ? v : ohi; }
            printf("OK %d %d %d %d %d %d %d %zu %ld %d %d %d %d %d\n", D, g.RW, g.chunk, g.nchunks, g.threads, g.E, g.wave, g.lds_bytes, g.grid,
                   lo, hi, olo, ohi, nom_ok);
        }
        return 0;
    }
    if (argc != 12 || strcmp(argv[1], "traj")) return 2;
    va::PredictAdjArgs a{};
    a.D = atoi(argv[2]); a.T = atoi(argv[3]); a.ncot = atoi(argv[4]); a.n_steps = atoi(argv[5]); a.substeps = atoi(argv[6]);
    a.every = atoi(argv[7]); a.dt = atof(argv[8]); a.t0 = 0.0; a.NP = va::RhsL96::NP; a.NPest = 1; a.nstim = 0; a.stim = nullptr;
    const int mode = atoi(argv[9]);
    a.n_out = a.n_steps / a.every + 1;
    if (mode != 0 && a.ncot != 1) return 2;
    if (!va::plan_predict_adj(a.D, a.T, a.ncot, a.NP, a.nstim, a.geo)) { fprintf(stderr, "refused: %s\n", a.geo.why); return 3; }
    const size_t row = (size_t)a.n_out * a.D;
    std::vector<double> x0((size_t)a.T * a.D), p((size_t)a.T), G, Y, w, out(a.T * row, -1.0), gx0((size_t)a.T * a.ncot * a.D, -1.0),
        gp((size_t)a.T * a.ncot, -1.0), cost(a.T, 0.0), ckpt(va::predict_adj_ckpt_doubles(a.geo, a.D, va::predict_adj_q(a)), -1.0);
    std::vector<int> lidx;
    FILE *fh = fopen(argv[10], "r");
    if (!fh) return 4;
    for (double &v : x0) if (fscanf(fh, "%lf", &v) != 1) return 5;
    for (double &v : p) if (fscanf(fh, "%lf", &v) != 1) return 5;
    if (mode == 0) {
        G.resize((size_t)a.T * a.ncot * row);
        for (double &v : G) if (fscanf(fh, "%lf", &v) != 1) return 5;
        a.G = G.data();
    } else {
        if (fscanf(fh, "%d", &a.L) != 1 || a.L < 0 || a.L > a.D) return 5;
        lidx.resize(a.L); w.resize(a.L);
        for (int &v : lidx) if (fscanf(fh, "%d", &v) != 1) return 5;
        for (double &v : w) if (fscanf(fh, "%lf", &v) != 1) return 5;
        Y.resize((size_t)(mode == 1 ? a.T : 1) * a.n_out * a.L);
        for (double &v : Y) if (fscanf(fh, "%lf", &v) != 1) return 5;
        a.Y = Y.data(); a.w = w.data(); a.Lidx = lidx.data(); a.y_stride = mode == 1 ? (size_t)a.n_out * a.L : 0;
    }
    fclose(fh);
    const int pidx = 0;
    a.x0 = x0.data(); a.p = p.data(); a.Pidx = &pidx; a.out = out.data(); a.gx0 = gx0.data(); a.gp = gp.data(); a.cost = cost.data();
    a.ckpt = ckpt.data();
    va::predict_adj_host<va::RhsL96>(a);
    fh = fopen(argv[11], "wb");
    if (!fh) return 6;
    for (const std::vector<double> *v : {&out, &gx0, &gp, &cost})
        if (fwrite(v->data(), sizeof(double), v->size(), fh) != v->size()) return 7;
    fclose(fh);
    printf("%d %d %d %d %d %d %zu %ld\n", a.geo.RW, a.geo.chunk, a.geo.nchunks, a.geo.threads, a.geo.E, a.geo.wave, a.geo.lds_bytes, a.geo.grid);
    return 0;
}
