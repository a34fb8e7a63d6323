// dladmm_fused_rs.hip -- path 5, the small-batch row-split forward with one workgroup per 16
// batch columns (dladmm_fused_rs_kernel.h, MEM = 1): its instantiations and dispatch.  The ELZ
// entry / exit modes (a.elz) are instantiated for V4 / V5 / V7.
#include "dladmm_fused_rs_kernel.h"

namespace dladmm {

// every variant at the 256 x 512 shape (the plan admits V2 / V3 only under
// DLADMM_F_ROWSPLIT_ROWP: dladmm_capi.hip use_rowsplit)
bool rs_supports(int shape, int variant) {
  return shape == 2 && variant >= DLADMM_V1_LENA && variant <= DLADMM_V7_SCALAR_V1E;
}

hipError_t launch_fused_rs(int shape, int variant, const FusedArgs& a, int grid, hipStream_t s) {
  if (shape != 2) return hipErrorInvalidValue;
  return with_variant_modes(variant, [&](auto EM_, auto PK_) {
    constexpr int EM = decltype(EM_)::value, PK = decltype(PK_)::value;
    if (!a.elz) return launch_fused_rs_as<EM, PK, false, 1>(a, grid, s);
    // V4, V5, V7
    if constexpr ((EM == EM_VVAR && PK != PK_ROW) || (EM == EM_V1 && PK == PK_S1))
      return launch_fused_rs_as<EM, PK, true, 1>(a, grid, s);
    return hipErrorInvalidValue;
  });
}

}  // namespace dladmm
