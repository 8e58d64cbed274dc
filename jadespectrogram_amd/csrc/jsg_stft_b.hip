// Translation unit B of the STFT kernels: the two 4096-point variants (JSG_STFT_VARIANTS, unit B; default machine scheduler: see jsg_stft_a.hip).
#ifndef JSG_X_B_SCALAR_TWIDDLE   // (variant builds: A/B of the scalar form in this unit)
#define JSG_TWIDDLE_CONST_VGPR 1   // see mul_w_q1
#endif
#include "jsg_stft_kernel.h"

namespace jsg {
#define JSG_IN_UNIT_A(...)
#define JSG_IN_UNIT_B(...) __VA_ARGS__
JSG_STFT_VARIANTS(JSG_DEFINE_VARIANT)
hipError_t touch_module_b() { return preload_code_object(reinterpret_cast<const void*>(&stft_db_kernel<Cfg4096, 3>)); }
}  // namespace jsg
