// va_nnet_geo.h -- the launch plan of the feed-forward-network action as plain host C++: the checks of a network
// descriptor, the layer tables, the job tables of the three product kernels in the order their workgroups meet the 8
// XCDs, and which of the small / tiled / fused paths the handle takes.  Integer arithmetic on the descriptor and the
// device's CU count, nothing else.  Included by the device image (va_nnet.h: the constants and NnetTile are shared with
// the kernels), by the host (va_capi.hip) and by the CPU check of the plans (tests/cpu_emul/nnet_plan_check.cpp,
// tests/test_nnet_geometry.py against tests/golden/nnet_plans.txt).  No HIP header.
#pragma once
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/varanneal_amd.h"

namespace va {

enum { NNET_SIGMOID = 0, NNET_TANH = 1, NNET_LINEAR = 2, NNET_RELU = 3, NNET_SOFTPLUS = 4,
       NNET_USER = 1000 };   // >= NNET_USER: a generated activation module (va_act_load_module)

constexpr int NN_TILE = 64;      // workgroup output tile: 2 x 2 waves, each 2 x 2 MFMA blocks of 16x16
constexpr int NN_KC = 32;        // K elements staged in LDS per step
constexpr int NN_THREADS = 256;
constexpr int NN_PACK = 8;       // elements per thread of the trial-point kernel (k_nnet_pack)

// layers up to NN_FB_W wide: the forward product and the state-gradient product of every transition in ONE kernel
// (k_nnet_fb, va_nnet_kernels.h): a workgroup marches a block of NN_FB_R examples through the layers
#ifndef NN_FB_ROWS
#define NN_FB_ROWS 32
#endif
#ifndef NN_FB_THR
#define NN_FB_THR 256
#endif
// NN_FB_THREADS / 64 waves share the NN_FB_W / 16 column blocks of a layer; NN_FB_WGS workgroups per CU (their LDS: two
// operand images of NN_FB_R rows)
constexpr int NN_FB_R = NN_FB_ROWS, NN_FB_W = 128, NN_FB_THREADS = NN_FB_THR, NN_FB_PITCH = NN_FB_W + 2;
constexpr int NN_FB_WGS = NN_FB_R == 32 ? 2 : 1;
constexpr int NN_FB_LAYERS = 64; // most layers its per-layer table in LDS holds
constexpr int NN_FB_PF = 8;      // k-steps the B fragments of its products are requested ahead
// k-steps a fragment table holds per column block for a product over K: whole groups of NN_FB_PF, one group of zeros behind
constexpr int nn_fb_steps(int K) { return (((K + 3) / 4 + NN_FB_PF - 1) / NN_FB_PF) * NN_FB_PF + NN_FB_PF; }

constexpr int NN_SMALL = 32;         // widest layer / most examples the single-kernel path handles
constexpr int NN_ROWS_DIRECT = 64;   // partial rows per seed the line-search kernel reduces itself
constexpr int NN_RED_ROWS = 32;      // rows left by k_nnet_rows when there are more
// one workgroup's job: rows [r0, r0+64) x columns [c0, c0+64) of a layer's product
// (layer metadata rides in the entry so a workgroup needs ONE dependent load before its data)
struct NnetTile { int layer, r0, c0, chunk, sn, sn1, offn, offn1, woff, boff, pad0, pad1; };

// Everything va_nnet_problem_create decides about a network before it touches the device: what it copies into NnetDev
// and uploads.
struct NnetPlan {
    std::vector<int> s, off;         // [NL] layer widths, [NL+1] offsets inside one example
    std::vector<int> woff, boff;     // [NL-1] offsets of W_n and b_n in P
    std::vector<int> lin, lout;      // [s[0]], [s[NL-1]] -> observed index or -1
    std::vector<int> pmap;           // [NP] -> index among the estimated parameters or -1
    std::vector<NnetTile> t1, t2, t3;      // job tables: one entry per NN_TILE x NN_TILE output tile
    int mch = 0, nmch = 0;           // examples per chunk of the weight-gradient product, chunks
    int n0 = 0, n1 = 0, n2 = 0, n3 = 0, n4 = 0, nraw = 0;      // as NnetDev (va_nnet.h)
    int small = 0;
    std::vector<int> wfoff;          // [2 (NL-1)] fragment offsets of the two products of every transition
    int wfsz = 0, nfb = 0;
    bool fb_ok = false;              // the layers fit k_nnet_fb (its buffers are allocated; va_problem_tune may switch it on)
    int fused = 0, fb_slots = 0;
    bool fold_rows = false;          // more than NN_ROWS_DIRECT partial rows: k_nnet_rows leaves NN_RED_ROWS
    int nprow = 0;
    int NDnet = 0;
    long long nvar = 0;
};

namespace nnet_geo_detail {

inline int refuse(const char **why, int code, const char *fmt, ...)
{
    static thread_local char buf[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (why) *why = buf;
    return code;
}

// Order of the jobs: workgroup i of a launch runs on XCD i % 8, each with an L2 of its own.  The jobs that read the
// same operand rows (the column tiles of one row block; the four tiles of one example chunk) are placed 8 apart --
// eight such families at a time, member by member -- so that they meet in ONE L2 and the rows come from HBM once
inline void place(std::vector<NnetTile> &out, std::vector<std::vector<NnetTile>> &fam)
{
    size_t f0 = 0;
    while (f0 < fam.size()) {
        const size_t nf = std::min<size_t>(8, fam.size() - f0);
        size_t width = 0;
        for (size_t f = 0; f < nf; ++f) width = std::max(width, fam[f0 + f].size());
        bool uniform = nf == 8;
        for (size_t f = 0; f < nf; ++f) uniform = uniform && fam[f0 + f].size() == width;
        if (uniform)
            for (size_t k = 0; k < width; ++k)
                for (size_t f = 0; f < nf; ++f) out.push_back(fam[f0 + f][k]);
        else
            for (size_t f = 0; f < nf; ++f) out.insert(out.end(), fam[f0 + f].begin(), fam[f0 + f].end());
        f0 += nf;
    }
    fam.clear();
}

// the checks of the descriptor, and the tables they fill on the way: s, off, woff, boff, lin, lout, pmap, NDnet, nvar
inline int check_desc(const va_nnet_desc *d, NnetPlan &p, const char **why)
{
    const int NL = d->n_layers;
    p.s.assign(d->structure, d->structure + NL); p.off.assign(NL + 1, 0); p.woff.assign(NL - 1, 0); p.boff.assign(NL - 1, 0);
    const std::vector<int> &s = p.s;
    long long np = 0;
    for (int n = 0; n < NL; ++n) {
        if (s[n] < 1) return refuse(why, VA_EINVAL, "structure[%d]=%d", n, s[n]);
        p.off[n + 1] = p.off[n] + s[n];
    }
    for (int n = 0; n < NL - 1; ++n) { p.woff[n] = (int)np; np += (long long)s[n + 1] * s[n]; p.boff[n] = (int)np; np += s[n + 1]; }
    if (np != d->NP) return refuse(why, VA_EINVAL, "NP=%d but the structure holds %lld weights and biases (va_nnet.py:194-207)", d->NP, np);
    if (d->NPest < 0 || d->NPest > d->NP || !d->P || (d->NPest > 0 && !d->Pidx)) return refuse(why, VA_EINVAL, "bad NPest/P/Pidx");
    if (d->L_in < 0 || d->L_out < 0 || (d->L_in > 0 && (!d->Lidx_in || !d->data_in)) || (d->L_out > 0 && (!d->Lidx_out || !d->data_out)))
        return refuse(why, VA_EINVAL, "observed-neuron arrays missing");
    if (d->L_in + d->L_out < 1) return refuse(why, VA_EINVAL, "no observed neurons: the measurement error divides by Ltot*M (va_nnet.py:173)");
    p.NDnet = p.off[NL];
    p.nvar = (long long)p.NDnet * d->M + d->NPest;
    if (p.nvar > 2000000000LL) return refuse(why, VA_EUNSUPPORTED, "n_var=%lld does not fit 32-bit indexing", p.nvar);
    p.lin.assign(s[0], -1); p.lout.assign(s[NL - 1], -1); p.pmap.assign(d->NP, -1);
    for (int l = 0; l < d->L_in; ++l) {
        if (d->Lidx_in[l] < 0 || d->Lidx_in[l] >= s[0]) return refuse(why, VA_EINVAL, "Lidx_in[%d]=%d outside the input layer", l, d->Lidx_in[l]);
        p.lin[d->Lidx_in[l]] = l;
    }
    for (int l = 0; l < d->L_out; ++l) {
        if (d->Lidx_out[l] < 0 || d->Lidx_out[l] >= s[NL - 1]) return refuse(why, VA_EINVAL, "Lidx_out[%d]=%d outside the output layer", l, d->Lidx_out[l]);
        p.lout[d->Lidx_out[l]] = l;
    }
    for (int k = 0; k < d->NPest; ++k) {
        if (d->Pidx[k] < 0 || d->Pidx[k] >= d->NP) return refuse(why, VA_EINVAL, "Pidx[%d]=%d outside [0,NP)", k, d->Pidx[k]);
        if (p.pmap[d->Pidx[k]] >= 0) return refuse(why, VA_EINVAL, "Pidx[%d]=%d listed twice", k, d->Pidx[k]);
        p.pmap[d->Pidx[k]] = k;
    }
    return VA_OK;
}

// job tables of the three product kernels, in the order of place()
inline void fill_jobs(const va_nnet_desc *d, NnetPlan &p)
{
    const int NL = d->n_layers;
    const std::vector<int> &s = p.s;
    auto tile = [&](int n, int r0, int c0, int c) {
        NnetTile t;
        memset(&t, 0, sizeof t);
        t.layer = n; t.r0 = r0; t.c0 = c0; t.chunk = c; t.sn = s[n]; t.offn = p.off[n];
        if (n < NL - 1) { t.sn1 = s[n + 1]; t.offn1 = p.off[n + 1]; t.woff = p.woff[n]; t.boff = p.boff[n]; }
        return t;
    };
    std::vector<std::vector<NnetTile>> fam;
    for (int n = 0; n < NL - 1; ++n) {
        for (int m0 = 0; m0 < d->M; m0 += NN_TILE) {
            fam.emplace_back();
            for (int i0 = 0; i0 < s[n + 1]; i0 += NN_TILE) fam.back().push_back(tile(n, m0, i0, 0));
        }
        place(p.t1, fam);
    }
    for (int n = 0; n < NL; ++n) {
        for (int m0 = 0; m0 < d->M; m0 += NN_TILE) {
            fam.emplace_back();
            for (int j0 = 0; j0 < s[n]; j0 += NN_TILE) fam.back().push_back(tile(n, m0, j0, 0));
        }
        place(p.t2, fam);
    }
    for (int n = 0; n < NL - 1; ++n) {
        for (int c = 0; c < p.nmch; ++c) {
            fam.emplace_back();
            for (int i0 = 0; i0 < s[n + 1]; i0 += NN_TILE)
                for (int j0 = 0; j0 < s[n]; j0 += NN_TILE) fam.back().push_back(tile(n, i0, j0, c));
        }
        place(p.t3, fam);
    }
}

}  // namespace nnet_geo_detail

// The plan of a network problem on a device of ncu compute units.  VA_OK, or the code of the first check the descriptor
// fails, with *why the message (valid until this thread's next refusal).  The caller has checked struct_size, batch,
// n_layers, M, structure != NULL and the activation id.
inline int plan_nnet(const va_nnet_desc *d, int ncu, NnetPlan &p, const char **why)
{
    p = NnetPlan();
    if (int rc = nnet_geo_detail::check_desc(d, p, why)) return rc;
    const int NL = d->n_layers;
    const std::vector<int> &s = p.s;
    // examples per chunk of the weight-gradient product: 256, doubled while the launch keeps >= 6 workgroups per CU
    // (each chunk writes a partial of the whole parameter gradient that k_nnet_pred reads back)
    p.mch = d->M <= 256 ? ((d->M + NN_KC - 1) / NN_KC) * NN_KC : 256;
    {
        long long tiles = 0;
        for (int n = 0; n < NL - 1; ++n) tiles += (long long)((s[n + 1] + NN_TILE - 1) / NN_TILE) * ((s[n] + NN_TILE - 1) / NN_TILE);
        while (p.mch * 2 <= d->M && tiles * d->batch * ((d->M + 2 * p.mch - 1) / (2 * p.mch)) >= 6LL * ncu) p.mch *= 2;
    }
    p.nmch = (d->M + p.mch - 1) / p.mch;
    nnet_geo_detail::fill_jobs(d, p);
    p.n1 = (int)p.t1.size(); p.n2 = (int)p.t2.size(); p.n3 = (int)p.t3.size();
    p.n4 = (d->NP + NN_THREADS - 1) / NN_THREADS;
    p.n0 = (p.NDnet * d->M + d->NP + NN_THREADS * NN_PACK - 1) / (NN_THREADS * NN_PACK);
    p.nraw = p.n1 + p.n2 + p.n4;
    int widest = 0;
    for (int n = 0; n < NL; ++n) widest = s[n] > widest ? s[n] : widest;
    // small networks: one workgroup per layer does the whole evaluation (k_nnet_small)
    {
        const int w = widest > d->M ? widest : d->M;
        p.small = (w <= NN_SMALL && NL <= NN_ROWS_DIRECT) ? (w <= 16 ? 16 : 32) : 0;
    }
    if (p.small) p.nraw = NL;
    // layers up to NN_FB_W wide with scalar measurement weights: forward and state-gradient products in one kernel
    // (k_nnet_fb); its workgroups write the first nfb of the n1 + n2 rows, k_nnet_wfrag zeroes the others
    p.wfoff.assign(2 * (NL - 1), 0);
    // fragment tables of the two products of every transition: NN_FB_W / 16 column blocks of nn_fb_steps(K) k-steps
    for (int n = 0; n < NL - 1; ++n) { p.wfoff[n] = p.wfsz; p.wfsz += (NN_FB_W / 16) * nn_fb_steps(s[n]) * 64; }
    for (int n = 0; n < NL - 1; ++n) { p.wfoff[NL - 1 + n] = p.wfsz; p.wfsz += (NN_FB_W / 16) * nn_fb_steps(s[n + 1]) * 64; }
    p.nfb = (d->M + NN_FB_R - 1) / NN_FB_R;
    p.fb_ok = !p.small && widest <= NN_FB_W && NL <= NN_FB_LAYERS && !d->rm_in_matrix && p.nfb <= p.n1 + p.n2 &&
              (long long)p.NDnet * d->M < (1LL << 31);
    p.fb_slots = ncu * NN_FB_WGS;
    // on when its blocks of NN_FB_R examples fill the chip at least once (a workgroup walks ALL layers of its block:
    // with few blocks the separate kernels, one workgroup per layer and tile, have more in flight); va_problem_tune
    // switches it either way (c5x, 1024 workgroups: 637 against 709 us per evaluation, profiles/r04_nnet_fused.txt)
    // (not for softplus -- log1p / exp / expm1 spill 28 registers there: 830 against 809 us -- nor, unasked, for a generated
    // activation, whose register needs nobody has looked at)
    p.fused = p.fb_ok && (long long)p.nfb * d->batch >= p.fb_slots && d->activation != NNET_SOFTPLUS && d->activation < NNET_USER;
    p.fold_rows = p.nraw > NN_ROWS_DIRECT;      // k_ls sums the rows with one wave: keep them few
    p.nprow = p.fold_rows ? NN_RED_ROWS : p.nraw;
    return VA_OK;
}

}  // namespace va
