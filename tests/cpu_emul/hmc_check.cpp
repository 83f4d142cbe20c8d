// hmc_check.cpp -- CPU check of the Hamiltonian Monte Carlo sampler (csrc/va_hmc.h, csrc/va_hmc_geo.h: the headers the kernels
// and the host include).  Test infrastructure only (tests/test_hmc_cpu.py).  Build with -ffp-contract=off.
//   hmc_check words seed chain it n      -> the generator's words, (n + 1) lines of 4 hex words (elements, then the extra stream)
//   hmc_check normals seed chain it n    -> the n normals and the two uniforms hmc_normal / hmc_uniforms draw, one %.17g per line
//   hmc_check bm w0 w1                   -> "u01(w0) u01(w1) box_muller(w0, w1)"
//   hmc_check geo n_var B               -> "OK nwg grid threads lo hi" (how often the lanes visit every (chain, element):
//                                           1 and 1 when right) | "NO reason"
//   hmc_check draws seed it n_var B      -> per (chain, element) in lane order of the geometry: "b i w0 w1" as the lanes draw them
//   hmc_check args case                  -> hmc_check_args on a named bad (or good) argument set: "rc reason"
//   hmc_check chain in out               -> the 6-variable quadratic (tridiagonal H) through hmc_host; `in` (text): B n_iter
//        n_leap thin jitter nan_it use_noise seed minv_kind n_keep, then eps[B], minv, keep_idx, diag[6], off[5], x0[B*6],
//        noise; `out` raw doubles: x_trace, p_trace [n_iter][B][6], mean, var [B][6], A, dH, accepted [B][n_iter], kept
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "va_hmc.h"

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
    const long n_var = 6, B = 2;
    double eps[2] = {0.1, 0.2}, minv[12];
    for (double &v : minv) v = 1.5;
    int64_t keep[2] = {0, 5};
    int n_iter = 3, n_leap = 2, thin = 1;
    double jitter = 0.1;
    const double *mp = minv;
    long minv_n = 6, n_keep = 2;
    if (!strcmp(name, "good")) {}
    else if (!strcmp(name, "good_per_chain")) minv_n = 12;
    else if (!strcmp(name, "good_no_minv")) mp = nullptr;
    else if (!strcmp(name, "n_iter")) n_iter = 0;
    else if (!strcmp(name, "n_leap")) n_leap = 0;
    else if (!strcmp(name, "thin")) thin = 0;
    else if (!strcmp(name, "eps_zero")) eps[1] = 0.0;
    else if (!strcmp(name, "eps_neg")) eps[0] = -0.1;
    else if (!strcmp(name, "eps_nan")) eps[0] = NAN;
    else if (!strcmp(name, "eps_inf")) eps[1] = INFINITY;
    else if (!strcmp(name, "minv_zero")) minv[3] = 0.0;
    else if (!strcmp(name, "minv_nan")) minv[5] = NAN;
    else if (!strcmp(name, "minv_inf")) minv[0] = INFINITY;
    else if (!strcmp(name, "minv_size")) minv_n = 7;
    else if (!strcmp(name, "jitter_one")) jitter = 1.0;
    else if (!strcmp(name, "jitter_neg")) jitter = -0.01;
    else if (!strcmp(name, "jitter_nan")) jitter = NAN;
    else if (!strcmp(name, "keep_high")) keep[1] = 6;
    else if (!strcmp(name, "keep_neg")) keep[0] = -1;
    else return 2;
    char why[192] = "";
    const int rc = hmc_check_args(n_var, B, n_iter, n_leap, thin, eps, jitter, mp, minv_n, keep, n_keep, why, sizeof why);
    printf("%d %s\n", rc, why);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 6 && !strcmp(argv[1], "words")) {
        const unsigned long long seed = strtoull(argv[2], nullptr, 0);
        const uint32_t chain = (uint32_t)atol(argv[3]), it = (uint32_t)atol(argv[4]);
        const long n = atol(argv[5]);
        for (long i = 0; i <= n; ++i) {
            uint32_t w[4];
            if (i < n) hmc_philox((uint32_t)seed, (uint32_t)(seed >> 32), chain, it, (uint32_t)i, 0u, w);
            else hmc_philox((uint32_t)seed, (uint32_t)(seed >> 32), chain, it, 0u, 1u, w);
            printf("%08x %08x %08x %08x\n", w[0], w[1], w[2], w[3]);
        }
        return 0;
    }
    if (argc == 6 && !strcmp(argv[1], "normals")) {
        // what the phases draw through hmc_normal / hmc_uniforms (no explicit noise): n normals, then the two uniforms
        const unsigned long long seed = strtoull(argv[2], nullptr, 0);
        HmcArgs a = {};
        a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.n_var = atol(argv[5]); a.B = atoi(argv[3]) + 1;
        const int b = atoi(argv[3]), it = atoi(argv[4]);
        for (long i = 0; i < a.n_var; ++i) printf("%.17g\n", hmc_normal(a, b, it, i));
        double u_acc, u_jit;
        hmc_uniforms(a, b, it, u_acc, u_jit);
        printf("%.17g\n%.17g\n", u_acc, u_jit);
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "bm")) {
        const uint32_t w0 = (uint32_t)strtoul(argv[2], nullptr, 0), w1 = (uint32_t)strtoul(argv[3], nullptr, 0);
        printf("%.17g %.17g %.17g\n", hmc_u01(w0), hmc_u01(w1), hmc_box_muller(w0, w1));
        return 0;
    }
    if (argc == 4 && !strcmp(argv[1], "geo")) {
        const long n_var = atol(argv[2]), B = atol(argv[3]);
        HmcGeo g;
        char gwhy[96];
        if (!plan_hmc(n_var, B, g, gwhy, sizeof gwhy)) { printf("NO %s\n", gwhy); return 0; }
        std::vector<int> cnt((size_t)B * n_var, 0);
        for (long wg = 0; wg < g.grid; ++wg)
            for (int t = 0; t < g.threads; ++t)
                for (int e = 0; e < HMC_EPT; ++e) {
                    const long i = hmc_element(n_var, wg % g.nwg, t, e);
                    if (i >= 0) ++cnt[(size_t)(wg / g.nwg) * n_var + i];
                }
        int lo = cnt[0], hi = cnt[0];
        for (int v : cnt) { lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
        printf("OK %ld %ld %d %d %d\n", g.nwg, g.grid, g.threads, lo, hi);
        return 0;
    }
    if (argc == 6 && !strcmp(argv[1], "draws")) {
        const unsigned long long seed = strtoull(argv[2], nullptr, 0);
        HmcArgs a = {};
        a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.it = atoi(argv[3]); a.n_var = atol(argv[4]); a.B = atoi(argv[5]);
        char gwhy[96];
        if (!plan_hmc(a.n_var, a.B, a.geo, gwhy, sizeof gwhy)) return 3;
        for (long wg = 0; wg < a.geo.grid; ++wg)
            for (int t = 0; t < a.geo.threads; ++t)
                for (int e = 0; e < HMC_EPT; ++e) {
                    const long i = hmc_element(a.n_var, wg % a.geo.nwg, t, e);
                    if (i < 0) continue;
                    uint32_t w[4];
                    hmc_philox(a.k0, a.k1, a.chain0 + (uint32_t)(wg / a.geo.nwg), (uint32_t)a.it, (uint32_t)i, 0u, w);
                    printf("%ld %ld %08x %08x\n", wg / a.geo.nwg, i, w[0], w[1]);
                }
        return 0;
    }
    if (argc == 3 && !strcmp(argv[1], "args")) return run_args(argv[2]);
    if (argc != 4 || strcmp(argv[1], "chain")) return 2;
    FILE *fh = fopen(argv[2], "r");
    if (!fh) return 4;
    int B, n_iter, n_leap, thin, nan_it, use_noise, minv_kind, n_keep;
    double jitter;
    unsigned long long seed;
    if (fscanf(fh, "%d %d %d %d %lf %d %d %llu %d %d", &B, &n_iter, &n_leap, &thin, &jitter, &nan_it, &use_noise, &seed, &minv_kind, &n_keep) != 10) return 5;
    const long n = NQ;
    const size_t nm = minv_kind == 2 ? (size_t)B * n : (size_t)n;
    std::vector<double> eps(B), minv(nm, 1.0), sminv(nm, 1.0), x((size_t)B * n), noise(use_noise ? (size_t)n_iter * B * (n + 2) : 0);
    std::vector<int64_t> keep(n_keep);
    Quad q;
    for (double &v : eps) if (fscanf(fh, "%lf", &v) != 1) return 5;
    if (minv_kind) for (double &v : minv) if (fscanf(fh, "%lf", &v) != 1) return 5;
    for (int64_t &v : keep) { long long t; if (fscanf(fh, "%lld", &t) != 1) return 5; v = t; }
    for (double &v : q.d) if (fscanf(fh, "%lf", &v) != 1) return 5;
    for (double &v : q.o) if (fscanf(fh, "%lf", &v) != 1) return 5;
    for (double &v : x) if (fscanf(fh, "%lf", &v) != 1) return 5;
    for (double &v : noise) if (fscanf(fh, "%lf", &v) != 1) return 5;
    fclose(fh);
    for (size_t i = 0; i < nm; ++i) sminv[i] = sqrt(minv[i]);
    char why[192];
    if (hmc_check_args(n, B, n_iter, n_leap, thin, eps.data(), jitter, minv_kind ? minv.data() : nullptr, (long)nm, keep.data(), n_keep, why, sizeof why)) {
        fprintf(stderr, "refused: %s\n", why);
        return 3;
    }
    HmcArgs a = {};
    if (!plan_hmc(n, B, a.geo, why, sizeof why)) return 3;
    const size_t nv = (size_t)B * n, nt = (size_t)B * n_iter, nk = (size_t)B * (n_iter / thin) * n_keep;
    std::vector<double> g(nv), p(nv, 0.0), xs(nv), gs(nv), A_eval(B), A_cur(2 * B), part(2 * (size_t)a.geo.grid), mean(nv, 0.0), m2(nv, 0.0),
        A_trace(nt), dH(nt), kept(nk + 1), xt((size_t)n_iter * nv), pt((size_t)n_iter * nv);
    std::vector<int32_t> accepted(nt);
    a.x = x.data(); a.g = g.data(); a.p = p.data(); a.xs = xs.data(); a.gs = gs.data(); a.minv = minv.data(); a.sminv = sminv.data();
    a.minv_stride = minv_kind == 2 ? n : 0; a.eps = eps.data(); a.jitter = jitter; a.noise = use_noise ? noise.data() : nullptr;
    a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.A_eval = A_eval.data(); a.A_cur = A_cur.data(); a.part = part.data();
    a.mean = mean.data(); a.m2 = m2.data(); a.A_trace = A_trace.data(); a.dH = dH.data(); a.accepted = accepted.data(); a.kept = kept.data();
    a.keep_idx = keep.data(); a.n_keep = n_keep; a.ld = n; a.n_var = n; a.B = B; a.n_iter = n_iter; a.thin = thin;
    int cur_it = 0;
    auto eval = [&]() {
        for (int b = 0; b < B; ++b) {
            A_eval[b] = q.eval(&x[(size_t)b * n], &g[(size_t)b * n]);
            if (nan_it >= 0 && cur_it == nan_it) g[(size_t)b * n + 2] = NAN;        // an injected NaN gradient entry during iteration nan_it
        }
    };
    cur_it = -1;
    eval();
    for (int b = 0; b < B; ++b) A_cur[b] = A_eval[b];
    cur_it = 0;
    hmc_host(a, n_leap, eval, [&](int it) {
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
    for (const std::vector<double> *v : {&xt, &pt, &mean, &var, &A_trace, &dH, &accd, &kept})
        if (v->size() && fwrite(v->data(), sizeof(double), v->size(), fh) != v->size()) return 7;
    fclose(fh);
    printf("%ld %ld %d\n", a.geo.nwg, a.geo.grid, a.geo.threads);
    return 0;
}
