// plan_check.cpp -- CPU view of the evaluation kernels' chooser (csrc/va_eval_geo.h: the header the host includes).
// Reads one problem per line from stdin, 20 integers:
//     D N_model batch disc rm_kind rf_kind merr_nskip L tile_rows eval_kernel bounds tdp rhs lin ne ghost xl xr gl gr
// (Lidx: L columns spread evenly, l D / L; xl < 0: the form has no reaches) and prints every integer the chooser
// produces for it:
//     emode RY NT maxr T ntiles ghost | key kernel disc K W [| g4 <Geo4>] [| g5 <Geo5> | ys <ystrip>]
// Lines that start with '#' are skipped.  Test infrastructure only (tests/test_eval_geometry.py).
#include <cstdio>
#include <cstring>
#include <vector>

#include "va_eval_geo.h"

int main()
{
    char line[512];
    static double one = 1.0;
    while (fgets(line, sizeof line, stdin)) {
        if (line[0] == '#' || line[0] == '\n') continue;
        int v[20];
        int n = 0, pos = 0, adv = 0;
        while (n < 20 && sscanf(line + pos, "%d%n", &v[n], &adv) == 1) { pos += adv; ++n; }
        if (n != 20) { fprintf(stderr, "bad line: %s", line); return 2; }
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
        const va::EvalPlan p = va::plan_eval(&d, f);
        const va::VariantKey key = va::variant_key(p, &d);
        printf("%d %d %d %d %d %d %d | key %d %d %d %d", p.emode, p.RY, p.NT, p.maxr, p.T, p.ntiles, p.ghost,
               key.kernel, key.disc, key.K, key.W);
        if (p.emode == 4) {
            const va::Geo4 &g = p.g4;
            printf(" | g4 %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %u", g.D, g.K, g.RW, g.NW, g.SUB, g.T, g.P, g.PITCH, g.PP, g.KDP,
                   g.XP, g.XW, g.EW1, g.R2, g.WAVE, g.magic);
        }
        if (p.emode == 5) {
            const va::Geo5 &g = p.g5;
            printf(" | g5 %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d | ys", g.D, g.NS, g.CW, g.NSG, g.WPG, g.GL, g.XL,
                   g.PR, g.NACT, g.PW, g.PL, g.SEGL, g.NSEG, g.YPMAX, g.nslot, g.nslot_ls, g.ne, g.xdpp, g.LY, g.warr);
            for (int y : p.ystrip) printf(" %d", y);
        }
        printf("\n");
    }
    return 0;
}
