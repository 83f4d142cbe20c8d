// nnet_plan_check.cpp -- CPU view of the network action's launch plan (csrc/va_nnet_geo.h: the header the host includes).
// Reads one network per line from stdin, integers:
//     batch M ncu activation rm_matrix NPest_mode L_in L_out structure...
// (NP: what the structure holds; NPest_mode 0: no parameter estimated, 1: all, 2: every third; Lidx_in / Lidx_out: L
// neurons spread evenly over the layer, l s / L) and prints every integer of the NnetPlan:
//     NL NDnet nvar mch nmch n0 n1 n2 n3 n4 nraw small wfsz nfb fb_ok fused fb_slots fold_rows nprow
//     | tab <FNV-1a of s off woff boff lin lout pmap> | wf <wfoff> | t1 <table> | t2 <table> | t3 <table>
// a table of at most 64 tiles as its count and the 10 live fields of every tile, a larger one as its count, '#', and
// the FNV-1a hash of those fields.  A refused descriptor prints "refused <code> <message>".
// Lines that start with '#' are skipped.  Test infrastructure only (tests/test_nnet_geometry.py).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "va_nnet_geo.h"

namespace {

struct Fnv {
    uint64_t h = 1469598103934665603ull;
    void add(int v)
    {
        const uint32_t u = (uint32_t)v;
        for (int k = 0; k < 4; ++k) { h ^= (u >> (8 * k)) & 0xffu; h *= 1099511628211ull; }
    }
    void add(const std::vector<int> &v) { for (int x : v) add(x); }
};

void print_table(const char *name, const std::vector<va::NnetTile> &t)
{
    printf(" | %s %zu", name, t.size());
    Fnv f;
    for (const va::NnetTile &e : t) {
        const int v[10] = {e.layer, e.r0, e.c0, e.chunk, e.sn, e.sn1, e.offn, e.offn1, e.woff, e.boff};
        for (int x : v) {
            if (t.size() <= 64) printf(" %d", x);
            else f.add(x);
        }
    }
    if (t.size() > 64) printf(" # %016llx", (unsigned long long)f.h);
}

}  // namespace

int main()
{
    static char line[4096];
    static double one = 1.0;
    while (fgets(line, sizeof line, stdin)) {
        if (line[0] == '#' || line[0] == '\n') continue;
        std::vector<int> v;
        char *p = line, *end = nullptr;
        for (long x = strtol(p, &end, 10); end != p; x = strtol(p, &end, 10)) { v.push_back((int)x); p = end; }
        if (v.size() < 10) { fprintf(stderr, "bad line: %s", line); return 2; }
        std::vector<int32_t> s(v.begin() + 8, v.end());
        va_nnet_desc d;
        memset(&d, 0, sizeof d);
        d.struct_size = (int32_t)sizeof d;
        d.batch = v[0]; d.M = v[1]; d.activation = v[3]; d.L_in = v[6]; d.L_out = v[7];
        const int ncu = v[2], npest_mode = v[5];
        d.n_layers = (int32_t)s.size(); d.structure = s.data();
        long long np = 0;
        for (size_t n = 0; n + 1 < s.size(); ++n) np += (long long)s[n + 1] * s[n] + s[n + 1];
        d.NP = (int32_t)np;
        std::vector<int32_t> pidx, li(d.L_in > 0 ? d.L_in : 1), lo(d.L_out > 0 ? d.L_out : 1);
        for (int k = 0; k < d.NP; k += npest_mode == 2 ? 3 : 1)
            if (npest_mode) pidx.push_back(k);
        d.NPest = (int32_t)pidx.size(); d.Pidx = pidx.data(); d.P = &one;
        for (int l = 0; l < d.L_in; ++l) li[l] = (int32_t)((long)l * s.front() / d.L_in);
        for (int l = 0; l < d.L_out; ++l) lo[l] = (int32_t)((long)l * s.back() / d.L_out);
        d.Lidx_in = li.data(); d.Lidx_out = lo.data(); d.data_in = &one; d.data_out = &one;
        if (v[4]) { d.rm_in_matrix = &one; d.rm_out_matrix = &one; }
        va::NnetPlan pl;
        const char *why = "";
        if (const int rc = va::plan_nnet(&d, ncu, pl, &why)) { printf("refused %d %s\n", rc, why); continue; }
        printf("%d %d %lld %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", d.n_layers, pl.NDnet, pl.nvar, pl.mch, pl.nmch,
               pl.n0, pl.n1, pl.n2, pl.n3, pl.n4, pl.nraw, pl.small, pl.wfsz, pl.nfb, (int)pl.fb_ok, pl.fused, pl.fb_slots,
               (int)pl.fold_rows, pl.nprow);
        Fnv tab;
        tab.add(pl.s); tab.add(pl.off); tab.add(pl.woff); tab.add(pl.boff); tab.add(pl.lin); tab.add(pl.lout); tab.add(pl.pmap);
        printf(" | tab %016llx | wf", (unsigned long long)tab.h);
        for (int x : pl.wfoff) printf(" %d", x);
        print_table("t1", pl.t1); print_table("t2", pl.t2); print_table("t3", pl.t3);
        printf("\n");
    }
    return 0;
}
