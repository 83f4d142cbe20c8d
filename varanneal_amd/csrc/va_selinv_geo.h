// va_selinv_geo.h -- geometry of the block-tridiagonal selected inverse k_selinv and of the block builder k_hblocks
// (va_selinv.h), as plain host C++: shared by the launchers (va_blocktri_selinv, va_laplace), by the host run of the
// kernel's phases and by the CPU check that records it (tests/cpu_emul/selinv_check.cpp, tests/test_selinv_cpu.py).
//
// One point = K diagonal blocks of width W (hb time rows of D states each), the K - 1 blocks under them, a border of NPe
// parameter rows and the parameter block.  One workgroup owns one point and keeps in LDS, at an odd row pitch:
//     big[0..3]   W x W blocks      forward: S -> C_k | B_k -> E_k;   backward: Sigma_{k+1,k+1} -> Sigma_kk | C_k -> E_k -> Ge
//                                   | C_k^-1 | Sigma_{k+1,k}
//     brd[0..2]   NPe x W blocks    forward: F_{k-1} | P_k -> R -> F_k;   backward: Sigma_{p,k+1} | F_k -> Gf | Sigma_{p,k}
//     spp         NPe x NPe         S_p -> Sigma_pp
//     piv         max(W, NPe)       the pivots of the block being factored, BEFORE their square roots (see lower_gram)
// Where the four W x W blocks do not fit beside the border (W > 56 with 32 parameters), Sigma_{k+1,k} is the one that stays
// in global memory: it is written once and read once per step, every other block is read W times.
#pragma once
#include <stddef.h>

#include "va_core.h"

namespace va {

constexpr int SELINV_THREADS = 256;                   // 4 waves per workgroup
constexpr int SELINV_MAX_W = 64;                      // widest block: D <= 64, or D <= 32 with Simpson-Hermite
constexpr int SELINV_MAX_NPE = 32;                    // most estimated parameters in the border
constexpr size_t SELINV_LDS_CAP = 160 * 1024;         // a CU's whole LDS (the opt-in of va_device.h)
constexpr size_t LAPLACE_WORKSPACE_BYTES = (size_t)1 << 30;      // va_laplace: the device buffers of one chunk of points stay under this

struct SelinvGeo {
    int W = 0, K = 0, NPe = 0;
    int Wp = 0, NPp = 0;          // odd row pitches of the LDS images (doubles): conflict-free column walks of 8-byte words
    int snk_global = 0;           // 1: Sigma_{k+1,k} of the current step lives in the point's workspace, not in LDS
    size_t piv = 0;               // doubles of the pivot vector (max(W, NPe), rounded up to even: the images stay 16-byte aligned)
    size_t big = 0, brd = 0;      // doubles of one W x W image (at least NPe x NPp: the parameter stage borrows them) / one border image
    size_t lds_doubles = 0, lds_bytes = 0;
    size_t ws_doubles = 0;        // per point, global: C_k, E_k, F_k and the pivots of every block (+ one Sigma_{k+1,k} when snk_global)
    long grid = 0;                // workgroups: one per point
    const char *why = "";         // the refusal, when plan_selinv returns false
};

constexpr int SELINV_HDR = 2;     // doubles in front of the images: [0] the running log-determinant

inline bool plan_selinv(int W, int K, int NPe, long npts, SelinvGeo &g)
{
    g = SelinvGeo();
    if (W < 1 || K < 1 || NPe < 0 || npts < 1) { g.why = "bad sizes"; return false; }
    if (W > SELINV_MAX_W) { g.why = "block wider than 64 (D <= 64, or D <= 32 with SimpsonHermite): one workgroup cannot hold its blocks in LDS"; return false; }
    if (NPe > SELINV_MAX_NPE) { g.why = "more than 32 estimated parameters in the border"; return false; }
    if (npts > 2147483647L) { g.why = "more points than one launch takes"; return false; }
    g.W = W; g.K = K; g.NPe = NPe;
    g.Wp = W | 1; g.NPp = NPe | 1;
    const size_t ww = (size_t)W * g.Wp, pp = (size_t)NPe * g.NPp;
    g.big = ww > pp ? ww : pp;
    g.brd = (size_t)NPe * g.Wp;
    g.piv = ((size_t)(W > NPe ? W : NPe) + 1) & ~(size_t)1;
    const size_t rest = SELINV_HDR + g.piv + 3 * g.brd + pp, cap = SELINV_LDS_CAP / sizeof(double);
    g.snk_global = (rest + 4 * g.big > cap) ? 1 : 0;
    g.lds_doubles = rest + (size_t)(g.snk_global ? 3 : 4) * g.big;
    if (g.lds_doubles > cap) { g.why = "blocks do not fit 160 KiB of LDS"; return false; }      // (not reached within the two limits)
    g.lds_bytes = sizeof(double) * g.lds_doubles;
    g.ws_doubles = (size_t)(2 * K - 1 + g.snk_global) * W * W + (size_t)K * NPe * W + (size_t)K * W;
    g.grid = npts;
    return true;
}

// ---------------------------------------------------------------- k_hblocks: where an entry of the blocks comes from
// The coloured products HV [nvec = (2 hb + 1) D + NPe][ld] of one point (va_ode.Annealer._hessian_blocks): direction c has
// ones at the path entries (n, j) with (n mod (2 hb + 1)) D + j == c, direction (2 hb + 1) D + e is the unit vector of
// parameter e.  Entry H[i, j] with i <= j is read from the product of column j's colour, and mirrored.
struct HblocksGeo { int N, D, hb, NPe; long ld; };

constexpr long HB_ZERO = -1, HB_ONE = -2;
VA_HD int hblocks_W(const HblocksGeo &h) { return h.hb * h.D; }
VA_HD int hblocks_K(const HblocksGeo &h) { return (h.N + h.hb - 1) / h.hb; }
VA_HD int hblocks_nvec(const HblocksGeo &h) { return (2 * h.hb + 1) * h.D + h.NPe; }
// path entry (bi, bj) of the padded K W x K W matrix -> offset into the point's HV (vector * ld + row), HB_ZERO or HB_ONE
VA_HD long hblocks_src(const HblocksGeo &h, long bi, long bj)
{
    const long ND = (long)h.N * h.D;
    if (bi >= ND || bj >= ND) return bi == bj ? HB_ONE : HB_ZERO;            // the padding of the last block: identity
    if (bi > bj) { const long t = bi; bi = bj; bj = t; }                     // upper triangle, mirrored
    const long ni = bi / h.D, nj = bj / h.D;
    if (nj - ni > h.hb) return HB_ZERO;                                      // (that product row holds another column of the colour)
    const long colour = (nj % (2 * h.hb + 1)) * h.D + (bj - nj * h.D);
    return colour * h.ld + bi;
}
// border entry (parameter e, padded path column bj)
VA_HD long hblocks_src_border(const HblocksGeo &h, int e, long bj)
{
    if (bj >= (long)h.N * h.D) return HB_ZERO;
    return ((long)(2 * h.hb + 1) * h.D + e) * h.ld + bj;
}
// parameter block entry (e, f): one of the two that are averaged
VA_HD long hblocks_src_pp(const HblocksGeo &h, int e, int f)
{
    return ((long)(2 * h.hb + 1) * h.D + e) * h.ld + (long)h.N * h.D + f;
}

// va_laplace: doubles of device memory one point takes (directions, products, partial parameter rows, blocks, factor,
// selected blocks, unpacked results), and the points of a chunk that stay under LAPLACE_WORKSPACE_BYTES (0: not even one)
inline size_t laplace_point_doubles(const HblocksGeo &h, const SelinvGeo &g, int NP, int hvp_ntiles)
{
    const size_t nvec = (size_t)hblocks_nvec(h), W = g.W, K = g.K, NPe = g.NPe, ND = (size_t)h.N * h.D;
    const size_t blocks = (2 * K - 1) * W * W + K * NPe * W + NPe * NPe;
    const size_t sel = K * W * W + K * NPe * W + NPe * NPe + 2;                       // Skk, Spk, Spp, logdet, status
    const size_t unp = ND + ND * h.D + NPe * ND;                                      // var_x, cov_xx, cov_px
    return 2 * nvec * (size_t)h.ld + nvec * hvp_ntiles * (NP > 0 ? NP : 1) + (size_t)h.ld + NP + blocks + g.ws_doubles + sel + unp;
}
inline long laplace_chunk_points(size_t point_doubles, long npts)
{
    const size_t fit = LAPLACE_WORKSPACE_BYTES / (sizeof(double) * point_doubles);
    return (long)(fit < (size_t)npts ? fit : (size_t)npts);
}

}  // namespace va
