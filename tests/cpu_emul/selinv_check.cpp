// selinv_check.cpp -- CPU check of the block-tridiagonal selected inverse (csrc/va_selinv.h, csrc/va_selinv_geo.h: the headers
// the kernels and the host include).  Test infrastructure only (tests/test_selinv_cpu.py, tests/_selinv_ref.py).
//   selinv_check geo W K NPe [W K NPe ...]  -> per shape: "OK W K NPe Wp NPp snk_global lds_bytes ws_doubles" | "NO W K NPe reason"
//   selinv_check run file       -> selinv_host (the kernel's phases, thread by thread) on: npts K W NPe want(4 flags: Skk Snk Spk
//                                  Spp) | Dk | Bk | Pk | Hpp;  prints status[npts], logdet[npts], then the requested outputs
//   selinv_check blocks file    -> hblocks_host on: N D hb NPe npts | HV;  prints Dk, Bk, Pk, Hpp
//   selinv_check laplace file   -> blocks -> selinv_host -> unpack_one on the same input;  prints status, logdet, var_x, cov_xx,
//                                  cov_px, cov_pp
// Numbers go out as %.17g, one per line (round-trip exact); NaN as "nan".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "va_selinv.h"

static FILE *fh;
static double num() { double v; if (fscanf(fh, "%lf", &v) != 1) { fprintf(stderr, "short input\n"); exit(5); } return v; }
static void fill(std::vector<double> &a, size_t n) { a.resize(n); for (double &v : a) v = num(); }
static void out(const std::vector<double> &a) { for (double v : a) printf("%.17g\n", v); }

int main(int argc, char **argv)
{
    if (argc >= 5 && !strcmp(argv[1], "geo")) {
        for (int i = 2; i + 2 < argc; i += 3) {
            const int W = atoi(argv[i]), K = atoi(argv[i + 1]), NPe = atoi(argv[i + 2]);
            va::SelinvGeo g;
            if (!va::plan_selinv(W, K, NPe, 3, g)) { printf("NO %d %d %d %s\n", W, K, NPe, g.why); continue; }
            printf("OK %d %d %d %d %d %d %zu %zu\n", W, K, NPe, g.Wp, g.NPp, g.snk_global, g.lds_bytes, g.ws_doubles);
        }
        return 0;
    }
    if (argc != 3) return 2;
    fh = fopen(argv[2], "r");
    if (!fh) return 4;
    const bool run = !strcmp(argv[1], "run"), blocks = !strcmp(argv[1], "blocks"), laplace = !strcmp(argv[1], "laplace");
    if (!run && !blocks && !laplace) return 2;

    va::SelinvArgs a;
    memset((void *)&a, 0, sizeof a);
    std::vector<double> Dk, Bk, Pk, Hpp, HV;
    int want[4] = {1, 0, 1, 1};
    int npts, K, W, NPe;
    va::HblocksGeo h = {};
    if (run) {
        npts = (int)num(); K = (int)num(); W = (int)num(); NPe = (int)num();
        for (int &w : want) w = (int)num();
        fill(Dk, (size_t)npts * K * W * W); fill(Bk, (size_t)npts * (K - 1) * W * W);
        fill(Pk, (size_t)npts * K * NPe * W); fill(Hpp, (size_t)npts * NPe * NPe);
    } else {
        h.N = (int)num(); h.D = (int)num(); h.hb = (int)num(); h.NPe = (int)num(); npts = (int)num();
        h.ld = (long)h.N * h.D + h.NPe;
        K = va::hblocks_K(h); W = va::hblocks_W(h); NPe = h.NPe;
        fill(HV, (size_t)npts * va::hblocks_nvec(h) * h.ld);
        Dk.assign((size_t)npts * K * W * W, -777.0); Bk.assign((size_t)npts * (K - 1) * W * W, -777.0);
        Pk.assign((size_t)npts * K * NPe * W, -777.0); Hpp.assign((size_t)npts * NPe * NPe, -777.0);
        va::HblocksArgs b;
        b.h = h; b.HV = HV.data(); b.Dk = Dk.data(); b.Bk = Bk.data(); b.Pk = Pk.data(); b.Hpp = Hpp.data(); b.npts = npts;
        va::hblocks_host(b);
        if (blocks) { out(Dk); out(Bk); out(Pk); out(Hpp); return 0; }
    }
    fclose(fh);
    if (!va::plan_selinv(W, K, NPe, npts, a.g)) { fprintf(stderr, "refused: %s\n", a.g.why); return 3; }
    std::vector<double> Skk((size_t)npts * K * W * W, -777.0), Snk((size_t)npts * (K - 1) * W * W, -777.0),
        Spk((size_t)npts * K * NPe * W, -777.0), Spp((size_t)npts * NPe * NPe, -777.0), logdet(npts, -777.0),
        ws((size_t)npts * a.g.ws_doubles, -777.0);
    std::vector<int> status(npts, -777);
    a.Dk = Dk.data(); a.Bk = Bk.data(); a.Pk = Pk.data(); a.Hpp = Hpp.data();
    a.Skk = want[0] ? Skk.data() : nullptr; a.Snk = want[1] ? Snk.data() : nullptr;
    a.Spk = want[2] ? Spk.data() : nullptr; a.Spp = want[3] ? Spp.data() : nullptr;
    a.logdet = logdet.data(); a.status = status.data(); a.ws = ws.data(); a.npts = npts;
    va::selinv_host(a);
    for (int s : status) printf("%d\n", s);
    out(logdet);
    if (run) {
        if (want[0]) out(Skk);
        if (want[1]) out(Snk);
        if (want[2]) out(Spk);
        if (want[3]) out(Spp);
        return 0;
    }
    const size_t ND = (size_t)h.N * h.D;
    std::vector<double> var_x(npts * ND, -777.0), cov_xx(npts * ND * h.D, -777.0), cov_px(npts * NPe * ND, -777.0);
    va::UnpackArgs u;
    u.h = h; u.Skk = Skk.data(); u.Spk = Spk.data(); u.var_x = var_x.data(); u.cov_xx = cov_xx.data(); u.cov_px = cov_px.data(); u.npts = npts;
    for (long pt = 0; pt < npts; ++pt)
        for (long e = 0; e < va::unpack_per_point(h); ++e) va::unpack_one(u, pt, e);
    out(var_x); out(cov_xx); out(cov_px); out(Spp);
    return 0;
}
