// lds_check.cpp -- CPU view of the evaluation kernels' LDS sizes: the plan of csrc/va_eval_geo.h put through the
// per-family size functions the launchers use (eval_flat_lds_bytes, eval3_lds_bytes, eval4_lds_bytes, eval5_lds_bytes,
// persist_lds_doubles).  Host side only: compile with hipcc -x hip --cuda-host-only -I varanneal_amd/csrc.
// Reads one problem per line from stdin, plan_check.cpp's 20 integers and three more:
//     D N_model batch disc rm_kind rf_kind merr_nskip L tile_rows eval_kernel bounds tdp rhs lin ne ghost xl xr gl gr NP NPest m
// and prints
//     emode T ntiles maxr | lds <bytes of a plain launch> <bytes of a line-search launch> | e5 nslot nslot_ls warr xdpp | seed G T <bytes>
// (seed: k_seed's slices with 256 / batch workgroups per seed at most; 0 0 0 when the ladder does not fit).
// Test infrastructure only: the case table of tests/test_gpu_lds_optin.py was made with it.
#include <cstdio>
#include <cstring>
#include <vector>

#include "va_eval_geo.h"
#include "va_eval3.h"
#include "va_eval4.h"
#include "va_eval5.h"
#include "va_eval_flat.h"
#include "va_persist.h"

int main()
{
    char line[512];
    static double one = 1.0;
    while (fgets(line, sizeof line, stdin)) {
        if (line[0] == '#' || line[0] == '\n') continue;
        int v[23];
        int n = 0, pos = 0, adv = 0;
        while (n < 23 && sscanf(line + pos, "%d%n", &v[n], &adv) == 1) { pos += adv; ++n; }
        if (n != 23) { fprintf(stderr, "bad line: %s", line); return 2; }
        va_problem_desc d;
        memset(&d, 0, sizeof d);
        d.struct_size = (int32_t)sizeof d;
        d.D = v[0]; d.N_model = v[1]; d.batch = v[2]; d.disc = v[3]; d.rm_kind = v[4]; d.rf_kind = v[5];
        d.merr_nskip = v[6]; d.L = v[7]; d.tile_rows = v[8]; d.eval_kernel = v[9];
        d.N_data = (d.N_model - 1) / d.merr_nskip + 1;
        if (v[10]) { d.lower = &one; d.upper = &one; }
        d.p_time_dependent = v[11]; d.rhs = v[12];
        std::vector<int32_t> lidx(d.L > 0 ? d.L : 1);
        for (int l = 0; l < d.L; ++l) lidx[l] = (int32_t)((long)l * d.D / d.L);
        d.Lidx = lidx.data();
        va::EvalForm f;
        f.lin = v[13]; f.ne = v[14]; f.ghost = v[15];
        f.has_reach5 = v[16] >= 0;
        for (int k = 0; k < 4; ++k) f.reach5[k] = f.has_reach5 ? v[16 + k] : 0;
        const int NP = v[20], NPest = v[21], m = v[22];
        const va::EvalPlan p = va::plan_eval(&d, f);
        va::Dev dv;
        memset(&dv, 0, sizeof dv);
        va::Dims &dm = dv.dm;                 // (as fill_dims, va_capi.hip: what the size functions read)
        dm.D = d.D; dm.N = d.N_model; dm.L = d.L; dm.disc = d.disc; dm.NP = NP; dm.NPt = NP; dm.NPest = NPest; dm.m = m;
        dm.tdp = d.p_time_dependent ? 1 : 0; dm.lin = f.lin;
        dm.emode = p.emode; dm.RY = p.RY; dm.NT = p.NT; dm.maxr = p.maxr; dm.T = p.T; dm.ntiles = p.ntiles; dm.ghost = p.ghost;
        dv.g4 = p.g4; dv.g5 = p.g5;
        size_t lds[2];
        for (int ls = 0; ls < 2; ++ls) {
            dv.lsrun = ls;
            lds[ls] = p.emode == 5 ? va::eval5_lds_bytes(dv) : p.emode == 4 ? va::eval4_lds_bytes(dv)
                    : p.emode == 3 ? va::eval3_lds_bytes(dm) : va::eval_flat_lds_bytes(dm);
        }
        int G = 0, T = 0;
        size_t seed = 0;
        const int maxG = 256 / d.batch;
        if (maxG >= 1 && va::persist_geometry(dm.N, dm.D, dm.L, NP, NPest, m, dm.disc, va::PZ_LDS_BYTES, maxG, 0, &G, &T))
            seed = 8 * va::persist_lds_doubles(T, dm.D, dm.L, NP, NPest, m, dm.disc == va::DISC_SH ? 2 : 1, G);
        else { G = 0; T = 0; }
        printf("%d %d %d %d | lds %zu %zu | e5 %d %d %d %d | seed %d %d %zu\n", p.emode, p.T, p.ntiles, p.maxr, lds[0], lds[1],
               p.g5.nslot, p.g5.nslot_ls, p.g5.warr, p.g5.xdpp, G, T, seed);
    }
    return 0;
}
