// lyap_check.cpp -- CPU check of the Lyapunov-spectrum kernel (csrc/va_lyap.h, csrc/va_lyap_geo.h: the headers the kernel and
// the host include).  Test infrastructure only (tests/test_lyap_cpu.py).
//   lyap_check geo D1                       -> per D in [1, D1] and K in [1, D]: "OK D K RW threads E wave pitch lds_bytes grid
//        emin emax dmin dmax" | "NO D K reason", planned for T = 3, NP = 1: how many lanes lyap_load gives every (trajectory,
//        slot, column) and how many every (trajectory, tangent)'s dot products (1 and 1 when right)
//   lyap_check plan D K NP nstim            -> "OK ..." | "NO D K reason" for one case
//   lyap_check args T D K n_steps substeps qr_every n_skip gain   (gain: none | ok | neg | nan | inf) -> "OK" | "NO reason"
//   lyap_check traj D T K n_steps substeps qr_every n_skip dt t0 q0 gain in out -> Lorenz-96 through lyap_host (the kernel's
//        phases, lane by lane): `in` holds T*D start values, T forcings, then T*K*D tangents (q0 = 1) and T*D gains (gain = 1) as
//        raw doubles; `out` receives logsum, x_end, Q_end, trace, status (as doubles) as raw doubles
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "va_lyap.h"

template <int E>
static void cover(const va::LyapArgs &a, std::vector<int> &nel, std::vector<int> &ndot)
{
    std::vector<double> mem(va::lyap_lds_doubles(a.geo.RW, a.K, a.D, a.NP, a.nstim) + 1, 0.0);
    const va::LyapLds l = va::lyap_lds(a, mem.data());
    for (long wg = 0; wg < a.geo.grid; ++wg)
        for (int tid = 0; tid < a.geo.threads; ++tid) {
            va::LyapLane<E> L;
            va::lyap_load<E>(a, l, wg, tid, L);
            for (int e = 0; e < E; ++e) {
                const va::LyapElem &el = L.el[e];
                if (el.kind) ++nel[((size_t)el.traj * (a.K + 1) + (el.kind == 1 ? 0 : el.k + 1)) * a.D + el.col];
            }
            if (L.dk >= 0) ++ndot[(size_t)L.dtraj * a.K + L.dk];
        }
}

static void plan_line(int D, int K, int NP, int nstim, bool count)
{
    va::LyapArgs a = {};
    a.T = 3; a.D = D; a.NP = NP; a.K = K; a.nstim = nstim; a.n_steps = 1; a.substeps = 1; a.qr_every = 1; a.n_skip = 0; a.t0 = 0.0; a.dt = 0.025;
    if (!va::plan_lyap(D, a.T, K, NP, nstim, a.geo)) { printf("NO %d %d %s\n", D, K, a.geo.why); return; }
    const va::LyapGeo &g = a.geo;
    int lo = 1, hi = 1, dlo = 1, dhi = 1;
    if (count) {
        std::vector<double> x0((size_t)a.T * D, 1.0), p((size_t)a.T * (NP ? NP : 1), 8.0);
        a.x0 = x0.data(); a.p = p.data();
        std::vector<int> nel((size_t)a.T * (K + 1) * D, 0), ndot((size_t)a.T * K, 0);
        switch (g.E) {
        case 1: cover<1>(a, nel, ndot); break;
        case 2: cover<2>(a, nel, ndot); break;
        case 3: cover<3>(a, nel, ndot); break;
        case 4: cover<4>(a, nel, ndot); break;
        case 5: cover<5>(a, nel, ndot); break;
        case 6: cover<6>(a, nel, ndot); break;
        case 7: cover<7>(a, nel, ndot); break;
        case 8: cover<8>(a, nel, ndot); break;
        default: printf("NO %d %d E=%d outside 1..8\n", D, K, g.E); return;
        }
        lo = hi = nel[0]; dlo = dhi = ndot[0];
        for (int v : nel) { lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
        for (int v : ndot) { dlo = v < dlo ? v : dlo; dhi = v > dhi ? v : dhi; }
    }
    printf("OK %d %d %d %d %d %d %d %zu %ld %d %d %d %d\n", D, K, g.RW, g.threads, g.E, g.wave, g.pitch, g.lds_bytes, g.grid, lo, hi, dlo, dhi);
}

int main(int argc, char **argv)
{
    if (argc == 3 && !strcmp(argv[1], "geo")) {
        for (int D = 1; D <= atoi(argv[2]); ++D)
            for (int K = 1; K <= D; ++K) plan_line(D, K, 1, 0, true);
        return 0;
    }
    if (argc == 6 && !strcmp(argv[1], "plan")) { plan_line(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), false); return 0; }
    if (argc == 10 && !strcmp(argv[1], "args")) {
        const long T = atol(argv[2]);
        const int D = atoi(argv[3]);
        std::vector<double> g((size_t)(T > 0 ? T : 1) * (D > 0 ? D : 1), 0.5);
        const bool none = !strcmp(argv[9], "none");
        if (!strcmp(argv[9], "neg")) g.back() = -1e-300;
        if (!strcmp(argv[9], "nan")) g[g.size() / 2] = std::numeric_limits<double>::quiet_NaN();
        if (!strcmp(argv[9], "inf")) g[0] = std::numeric_limits<double>::infinity();
        char why[192] = "";
        const bool ok = va::lyap_check_args(T, D, atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), atoi(argv[7]), atoi(argv[8]), none ? nullptr : g.data(),
                                            why, sizeof why);
        printf(ok ? "OK\n" : "NO %s\n", why);
        return 0;
    }
    if (argc != 15 || strcmp(argv[1], "traj")) return 2;
    va::LyapArgs a = {};
    a.D = atoi(argv[2]); a.T = atoi(argv[3]); a.K = atoi(argv[4]); a.n_steps = atoi(argv[5]); a.substeps = atoi(argv[6]); a.qr_every = atoi(argv[7]);
    a.n_skip = atoi(argv[8]); a.dt = atof(argv[9]); a.t0 = atof(argv[10]); a.NP = va::RhsL96::NP; a.nstim = 0; a.stim = nullptr;
    const bool has_q0 = atoi(argv[11]) != 0, has_gain = atoi(argv[12]) != 0;
    std::vector<double> x0((size_t)a.T * a.D), p((size_t)a.T), Q0(has_q0 ? (size_t)a.T * a.K * a.D : 0), gain(has_gain ? (size_t)a.T * a.D : 0);
    FILE *fh = fopen(argv[13], "rb");
    if (!fh) return 4;
    for (std::vector<double> *v : {&x0, &p, &Q0, &gain})
        if (v->size() && fread(v->data(), sizeof(double), v->size(), fh) != v->size()) return 5;
    fclose(fh);
    char why[192] = "";
    if (!va::lyap_check_args(a.T, a.D, a.K, a.n_steps, a.substeps, a.qr_every, a.n_skip, has_gain ? gain.data() : nullptr, why, sizeof why)) {
        fprintf(stderr, "bad arguments: %s\n", why);
        return 3;
    }
    if (!va::plan_lyap(a.D, a.T, a.K, a.NP, a.nstim, a.geo)) { fprintf(stderr, "refused: %s\n", a.geo.why); return 3; }
    const int n_qr = a.n_steps / a.qr_every;
    std::vector<double> logsum((size_t)a.T * a.K, -1.0), x_end((size_t)a.T * a.D, -1.0), Q_end((size_t)a.T * a.K * a.D, -1.0),
        trace((size_t)a.T * n_qr * a.K, -1.0), stat((size_t)a.T);
    std::vector<int> status((size_t)a.T, -1);
    a.x0 = x0.data(); a.p = p.data(); a.Q0 = has_q0 ? Q0.data() : nullptr; a.coupling = has_gain ? gain.data() : nullptr;
    a.logsum = logsum.data(); a.x_end = x_end.data(); a.Q_end = Q_end.data(); a.trace = trace.data(); a.status = status.data();
    va::lyap_host<va::RhsL96>(a);
    for (int t = 0; t < a.T; ++t) stat[t] = (double)status[t];
    fh = fopen(argv[14], "wb");
    if (!fh) return 6;
    for (const std::vector<double> *v : {&logsum, &x_end, &Q_end, &trace, &stat})
        if (fwrite(v->data(), sizeof(double), v->size(), fh) != v->size()) return 7;
    fclose(fh);
    printf("%d %d %d %d %d %zu %ld\n", a.geo.RW, a.geo.threads, a.geo.E, a.geo.wave, a.geo.pitch, a.geo.lds_bytes, a.geo.grid);
    return 0;
}
