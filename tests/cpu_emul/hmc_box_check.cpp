// hmc_box_check.cpp -- CPU check of the box sampler (csrc/va_hmc_box.h, csrc/va_hmc_geo.h: the headers the kernels and the host
// include).  Test infrastructure only (tests/test_hmc_box_cpu.py).  Build with -ffp-contract=off.
//   hmc_box_check map in out      -> `in` (text): n, then n rows "lo hi z" (inf / -inf: no bound); `out` raw doubles: x, dx, dlj,
//                                    lj [n] each, by hmc_box_kinds and hmc_box_map
//   hmc_box_check inv in out      -> the same rows with x in place of z; `out` raw doubles z [n] by hmc_box_inverse
//   hmc_box_check args case       -> the box sampler's own checks on a named bad (or good) argument set: "rc reason"
//   hmc_box_check chain in out    -> hmc_check's 6-variable quadratic through hmc_host_box; `in` as hmc_check's, with lo[6] and
//        hi[6] between x0 and the noise (x0 is in x: checked, inverted on the host); `out` raw doubles: z_trace, x_trace, p_trace
//        [n_iter][B][6], mean, var [B][6], A, dH, accepted [B][n_iter], kept
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "va_hmc_box.h"

using namespace va;

static const int NQ = 6;

struct Quad {
    double d[NQ], o[NQ - 1];
    // g_i = (o_{i-1} x_{i-1} + d_i x_i) + o_i x_{i+1};  A = 1/2 sum_i x_i g_i in index order
    double eval(const double *x, double *g) const
    {
        double A = 0.0;
        for (int i = 0; i < NQ; ++i) {
            double v = d[i] * x[i];
            if (i > 0) v = o[i - 1] * x[i - 1] + v;
            if (i < NQ - 1) v = v + o[i] * x[i + 1];
            g[i] = v;
            A = A + x[i] * v;
        }
        return 0.5 * A;
    }
};

static int run_args(const char *name)
{
    const long n = 4, B = 2;
    double lo[4] = {-1.0, -HUGE_VAL, 0.5, -HUGE_VAL}, hi[4] = {1.0, 2.0, HUGE_VAL, HUGE_VAL};
    double X[8] = {0.0, 1.0, 1.0, 7.0, 0.5, -3.0, 2.5, -7.0}, Z[8] = {0, 1, 2, 3, 4, 5, 6, 7};
    int32_t kind[4];
    char why[256] = "";
    bool use_z = false;
    if (!strcmp(name, "good")) {}
    else if (!strcmp(name, "good_z")) use_z = true;
    else if (!strcmp(name, "lo_eq_hi")) lo[0] = 1.0;
    else if (!strcmp(name, "lo_gt_hi")) { lo[2] = 3.0; hi[2] = 2.0; }
    else if (!strcmp(name, "lo_nan")) lo[1] = NAN;
    else if (!strcmp(name, "on_lower")) X[6] = 0.5;
    else if (!strcmp(name, "on_upper")) X[1] = 2.0;
    else if (!strcmp(name, "outside")) X[4] = 1.5;
    else if (!strcmp(name, "start_nan")) X[3] = NAN;
    else if (!strcmp(name, "z_inf")) { use_z = true; Z[5] = INFINITY; }
    else if (!strcmp(name, "no_bounds")) for (int i = 0; i < 4; ++i) { lo[i] = -HUGE_VAL; hi[i] = HUGE_VAL; }
    else return 2;
    const long nb = hmc_box_kinds(n, lo, hi, kind, why, sizeof why);
    if (nb < 0) { printf("1 %s\n", why); return 0; }
    if (nb == 0) { printf("4 %s\n", why); return 0; }
    const int rc = use_z ? hmc_box_check_z(n, B, n, Z, why, sizeof why) : hmc_box_check_start(n, B, n, X, lo, hi, why, sizeof why);
    printf("%d %s kinds %d %d %d %d\n", rc, why, kind[0], kind[1], kind[2], kind[3]);
    return 0;
}

static int run_table(const char *in, const char *out, bool inverse)
{
    FILE *fh = fopen(in, "r");
    if (!fh) return 4;
    long n;
    if (fscanf(fh, "%ld", &n) != 1 || n < 1) return 5;
    std::vector<double> lo(n), hi(n), v(n);
    for (long i = 0; i < n; ++i)
        if (fscanf(fh, "%lf %lf %lf", &lo[i], &hi[i], &v[i]) != 3) return 5;
    fclose(fh);
    std::vector<int32_t> kind(n);
    char why[256];
    if (hmc_box_kinds(n, lo.data(), hi.data(), kind.data(), why, sizeof why) < 0) { fprintf(stderr, "refused: %s\n", why); return 3; }
    std::vector<double> r((inverse ? 1 : 4) * (size_t)n);
    for (long i = 0; i < n; ++i) {
        if (inverse) r[i] = hmc_box_inverse(kind[i], lo[i], hi[i], v[i]);
        else hmc_box_map(kind[i], lo[i], hi[i], v[i], &r[i], &r[n + i], &r[2 * n + i], &r[3 * n + i]);
    }
    fh = fopen(out, "wb");
    if (!fh) return 6;
    if (fwrite(r.data(), sizeof(double), r.size(), fh) != r.size()) return 7;
    fclose(fh);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 3 && !strcmp(argv[1], "args")) return run_args(argv[2]);
    if (argc == 4 && !strcmp(argv[1], "map")) return run_table(argv[2], argv[3], false);
    if (argc == 4 && !strcmp(argv[1], "inv")) return run_table(argv[2], argv[3], true);
    if (argc != 4 || strcmp(argv[1], "chain")) return 2;
    FILE *fh = fopen(argv[2], "r");
    if (!fh) return 4;
    int B, n_iter, n_leap, thin, nan_it, use_noise, minv_kind, n_keep;
    double jitter;
    unsigned long long seed;
    if (fscanf(fh, "%d %d %d %d %lf %d %d %llu %d %d", &B, &n_iter, &n_leap, &thin, &jitter, &nan_it, &use_noise, &seed, &minv_kind, &n_keep) != 10) return 5;
    const long n = NQ;
    const size_t nm = minv_kind == 2 ? (size_t)B * n : (size_t)n;
    std::vector<double> eps(B), minv(nm, 1.0), sminv(nm, 1.0), x((size_t)B * n), lo(n), hi(n), noise(use_noise ? (size_t)n_iter * B * (n + 2) : 0);
    std::vector<int64_t> keep(n_keep);
    Quad q;
    for (double &v : eps) if (fscanf(fh, "%lf", &v) != 1) return 5;
    if (minv_kind) for (double &v : minv) if (fscanf(fh, "%lf", &v) != 1) return 5;
    for (int64_t &v : keep) { long long t; if (fscanf(fh, "%lld", &t) != 1) return 5; v = t; }
    for (double &v : q.d) if (fscanf(fh, "%lf", &v) != 1) return 5;
    for (double &v : q.o) if (fscanf(fh, "%lf", &v) != 1) return 5;
    for (double &v : x) if (fscanf(fh, "%lf", &v) != 1) return 5;
    for (double &v : lo) if (fscanf(fh, "%lf", &v) != 1) return 5;
    for (double &v : hi) if (fscanf(fh, "%lf", &v) != 1) return 5;
    for (double &v : noise) if (fscanf(fh, "%lf", &v) != 1) return 5;
    fclose(fh);
    for (size_t i = 0; i < nm; ++i) sminv[i] = sqrt(minv[i]);
    char why[256];
    if (hmc_check_args(n, B, n_iter, n_leap, thin, eps.data(), jitter, minv_kind ? minv.data() : nullptr, (long)nm, keep.data(), n_keep, why, sizeof why)) {
        fprintf(stderr, "refused: %s\n", why);
        return 3;
    }
    std::vector<int32_t> kind(n);
    // (all-free bounds are let through here: the test of kind 0 against hmc_host wants them)
    if (hmc_box_kinds(n, lo.data(), hi.data(), kind.data(), why, sizeof why) < 0 || hmc_box_check_start(n, B, n, x.data(), lo.data(), hi.data(), why, sizeof why)) {
        fprintf(stderr, "refused: %s\n", why);
        return 3;
    }
    HmcBoxArgs a = {};
    HmcArgs &h = a.h;
    if (!plan_hmc(n, B, h.geo, why, sizeof why)) return 3;
    const size_t nv = (size_t)B * n, nt = (size_t)B * n_iter, nk = (size_t)B * (n_iter / thin) * n_keep;
    std::vector<double> z(nv), zs(nv), g(nv), p(nv, 0.0), xs(nv), gs(nv), A_eval(B), A_cur(2 * B), part(2 * (size_t)h.geo.grid), lpart(2 * (size_t)h.geo.grid),
        mean(nv, 0.0), m2(nv, 0.0), A_trace(nt), dH(nt), kept(nk + 1), zt((size_t)n_iter * nv), xt((size_t)n_iter * nv), pt((size_t)n_iter * nv);
    std::vector<int32_t> accepted(nt);
    for (size_t k = 0; k < nv; ++k) {
        const long i = (long)(k % n);
        double dx, dlj, lj;
        z[k] = hmc_box_inverse(kind[i], lo[i], hi[i], x[k]);
        hmc_box_map(kind[i], lo[i], hi[i], z[k], &x[k], &dx, &dlj, &lj);
    }
    h.x = x.data(); h.g = g.data(); h.p = p.data(); h.xs = xs.data(); h.gs = gs.data(); h.minv = minv.data(); h.sminv = sminv.data();
    h.minv_stride = minv_kind == 2 ? n : 0; h.eps = eps.data(); h.jitter = jitter; h.noise = use_noise ? noise.data() : nullptr;
    h.k0 = (uint32_t)seed; h.k1 = (uint32_t)(seed >> 32); h.A_eval = A_eval.data(); h.A_cur = A_cur.data(); h.part = part.data();
    h.mean = mean.data(); h.m2 = m2.data(); h.A_trace = A_trace.data(); h.dH = dH.data(); h.accepted = accepted.data(); h.kept = kept.data();
    h.keep_idx = keep.data(); h.n_keep = n_keep; h.ld = n; h.n_var = n; h.B = B; h.n_iter = n_iter; h.thin = thin;
    a.z = z.data(); a.zs = zs.data(); a.kind = kind.data(); a.lo = lo.data(); a.hi = hi.data(); a.lpart = lpart.data();
    int cur_it = -1;
    auto eval = [&]() {
        for (int b = 0; b < B; ++b) {
            A_eval[b] = q.eval(&x[(size_t)b * n], &g[(size_t)b * n]);
            if (nan_it >= 0 && cur_it == nan_it) g[(size_t)b * n + 2] = NAN;
        }
    };
    eval();
    for (int b = 0; b < B; ++b) A_cur[b] = A_eval[b];
    cur_it = 0;
    hmc_host_box(a, n_leap, eval, [&](int it) {
        memcpy(&zt[(size_t)it * nv], z.data(), sizeof(double) * nv);
        memcpy(&xt[(size_t)it * nv], x.data(), sizeof(double) * nv);
        memcpy(&pt[(size_t)it * nv], p.data(), sizeof(double) * nv);
        cur_it = it + 1;
    });
    std::vector<double> var(nv), accd(nt);
    for (size_t i = 0; i < nv; ++i) var[i] = n_iter > 1 ? m2[i] / (double)(n_iter - 1) : 0.0;
    for (size_t i = 0; i < nt; ++i) accd[i] = accepted[i];
    kept.resize(nk);
    fh = fopen(argv[3], "wb");
    if (!fh) return 6;
    for (const std::vector<double> *v : {&zt, &xt, &pt, &mean, &var, &A_trace, &dH, &accd, &kept})
        if (v->size() && fwrite(v->data(), sizeof(double), v->size(), fh) != v->size()) return 7;
    fclose(fh);
    printf("%ld %ld %d\n", h.geo.nwg, h.geo.grid, h.geo.threads);
    return 0;
}
