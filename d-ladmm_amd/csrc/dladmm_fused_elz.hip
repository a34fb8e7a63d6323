// dladmm_fused_elz.hip -- instantiations of the fused K-layer forward with the DLADMM_F_ELZ
// entry / exit modes (steps E, L, Z from an arbitrary triple: the newS safeguarded KM loop), for
// the scalar-parameter forms that loop uses: V4 / V5 (learned step) and V7 (classic step).  They
// are the saved-product form (the tail's P[K] and the steps' P[j] go through a.Po; a call without
// P stores to 0-record buffers).  The kernel template and its design notes: dladmm_fused_kernel.h.
#include "dladmm_fused_kernel.h"

namespace dladmm {

template <int MP, int NP>
hipError_t dispatch_variant_elz(int variant, const FusedArgs& a, int grid, hipStream_t s) {
  switch (variant) {
    case DLADMM_V4_SCALAR:
      return launch_fused<MP, NP, EM_VVAR, PK_SCALAR, true, false, true>(a, grid, s);
    case DLADMM_V5_TIED: return launch_fused<MP, NP, EM_VVAR, PK_S1, true, false, true>(a, grid, s);
    case DLADMM_V7_SCALAR_V1E:
      return launch_fused<MP, NP, EM_V1, PK_S1, true, false, true>(a, grid, s);
  }
  return hipErrorInvalidValue;
}

hipError_t launch_fused_shape_elz(int shape, int variant, const FusedArgs& a, int grid,
                                  hipStream_t s) {
  if (!a.elz) return hipErrorInvalidValue;
  switch (shape) {
    case 0: return dispatch_variant_elz<kShapeMP[0], kShapeNP[0]>(variant, a, grid, s);
    case 1: return dispatch_variant_elz<kShapeMP[1], kShapeNP[1]>(variant, a, grid, s);
    case 2: return dispatch_variant_elz<kShapeMP[2], kShapeNP[2]>(variant, a, grid, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace dladmm
