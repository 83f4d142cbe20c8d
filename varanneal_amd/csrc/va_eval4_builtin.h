// va_eval4_builtin.h -- the built-in Lorenz-96's instantiations of k_eval4 at ONE workgroup width G (row groups per
// workgroup, va_eval4.h): every run length, D = 20 as a constant or D in a register, the three weight forms, the four
// discretisations.  The evaluation kernels take minutes to compile, so every width is a translation unit of its own:
// va_kernels.hip (G = 1), va_eval4_g2.hip, va_eval4_g3.hip.
#pragma once
#include "va_eval4.h"

namespace va {

template <class RHS, int K, int DC, int WS, int G>
static void eval4_rhs(const Dev &dv, EvalOp &op)
{
    with_disc(dv.dm.disc, [&](auto disc) { eval4_op<RHS, decltype(disc)::value, K, DC, WS, G>(dv, op); });
}

// D = 20 (examples/Lorenz96_D20, BASELINE configs 1-3) is compiled with D as a constant; scalar RM /
// RF0 with data at every model time (the same configs) run the variant without weight registers
template <class RHS, int K, int G>
static void eval4_d(const Dev &dv, EvalOp &op)
{
    const bool sw = !dv.pp.rm_arr && !dv.pp.rf0_arr, ws = sw && dv.dm.nskip == 1;
    if (dv.dm.D == 20) {
        if (ws) eval4_rhs<RHS, K, 20, 1, G>(dv, op);
        else if (sw) eval4_rhs<RHS, K, 20, 2, G>(dv, op);        // scalar weights, data at every nskip-th row
        else eval4_rhs<RHS, K, 20, 0, G>(dv, op);
    } else { if (ws) eval4_rhs<RHS, K, 0, 1, G>(dv, op); else eval4_rhs<RHS, K, 0, 0, G>(dv, op); }
}

// (a width the run length's registers do not hold -- G = 3 at runs of 8 or 12 rows -- has no kernel: eval4_op says so in op.err)
template <int G>
static void eval4_builtin(const Dev &dv, EvalOp &op)
{
    switch (dv.dm.maxr) {
    case 4: eval4_d<RhsL96s, 4, G>(dv, op); break;
    case 5: eval4_d<RhsL96s, 5, G>(dv, op); break;
    case 6: eval4_d<RhsL96s, 6, G>(dv, op); break;
    case 7: eval4_d<RhsL96s, 7, G>(dv, op); break;
    // runs of 12 rows at two row groups per CU (D = 20, scalar weights, data at every row or every nskip-th: Simpson-Hermite at
    // the C3 shape in ONE round of resident workgroups, see plan_eval4 in va_eval_geo.h)
    case 12: if (dv.dm.nskip == 1) eval4_rhs<RhsL96s, 12, 20, 1, G>(dv, op); else eval4_rhs<RhsL96s, 12, 20, 2, G>(dv, op); break;
    default: eval4_d<RhsL96s, 8, G>(dv, op); break;
    }
}

}  // namespace va
