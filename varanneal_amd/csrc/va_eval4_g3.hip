// va_eval4_g3.hip -- the built-in right-hand side on k_eval4 with three row groups (twelve waves) per workgroup.
#include <hip/hip_runtime.h>

#include "va_device.h"
#include "va_eval4_builtin.h"

namespace va {

void eval4_builtin_g3(const Dev &dv, EvalOp &op) { eval4_builtin<3>(dv, op); }

}  // namespace va
