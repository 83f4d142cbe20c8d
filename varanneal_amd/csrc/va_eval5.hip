// va_eval5.hip -- instantiations of the streaming evaluation kernel (va_eval5.h) for the built-in Lorenz-96
// (examples/Lorenz96_D20/Lorenz96_anneal.py:15-16 at the widths of BASELINE config 4).  A translation unit of
// its own so that the library's units compile side by side.
#include "va_device.h"
#include "va_eval5.h"

namespace va {

size_t eval5_lds(const Dev &dv) { return eval5_lds_bytes(dv); }

// D = 200 (BASELINE config 4) is compiled with the column geometry as constants
void eval5_builtin(const Dev &dv, EvalOp &op)
{
    with_disc(dv.dm.disc, [&](auto disc) {
        if (dv.dm.D == 200) eval5_op<RhsL96s, decltype(disc)::value, 200>(dv, op);
        else eval5_op<RhsL96s, decltype(disc)::value, 0>(dv, op);
    });
}

}  // namespace va
