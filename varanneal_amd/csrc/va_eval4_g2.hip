// va_eval4_g2.hip -- the built-in right-hand side on k_eval4 with two row groups (eight waves) per workgroup.
#include <hip/hip_runtime.h>

#include "va_device.h"
#include "va_eval4_builtin.h"

namespace va {

void eval4_builtin_g2(const Dev &dv, EvalOp &op) { eval4_builtin<2>(dv, op); }

}  // namespace va
