// dladmm_fused_bf16.hip -- instantiations of the bf16-operand fused forward
// (dladmm_fused_bf16_kernel.h, forward path 7) and the variant support query of the C ABI plan.
#include "dladmm_fused_bf16_kernel.h"

namespace dladmm {

bool bf16_fused_supports(int variant) {
  return variant == DLADMM_V4_SCALAR || variant == DLADMM_V5_TIED ||
         variant == DLADMM_V6_LASSO || variant == DLADMM_V1_LENA;
}

// the per-row models (PK_ROW instantiations): only under DLADMM_F_BF16_FUSED_ROWP
bool bf16_fused_supports_rows(int variant) {
  return variant == DLADMM_V2_LTHETA || variant == DLADMM_V3_FULL;
}

// Shapes 1 and 2, as the split-f16 kernel: the C ABI runs shape-0 problems on shape 1 (zero
// padding is exact).
hipError_t launch_fused_bf16_shape(int shape, int variant, const FusedArgs& a, int grid,
                                   hipStream_t s) {
  switch (shape) {
    case 1: return dispatch_bf16_variant<kShapeMP[1], kShapeNP[1]>(variant, a, grid, s);
    case 2: return dispatch_bf16_variant<kShapeMP[2], kShapeNP[2]>(variant, a, grid, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace dladmm
