// dladmm_reverse_rs.hip -- the small-batch row-split reverse sweep (dladmm_reverse_rs_kernel.h,
// bwd paths 2 and 3): its dispatch and the V1 / V4 / V5 / V6 instantiations.  V2 / V3 (per-row
// parameters) are instantiated in dladmm_reverse_rs_v2.hip / dladmm_reverse_rs_v3.hip.
#include "dladmm_reverse_rs_kernel.h"

namespace dladmm {

// a group's exchange buffer: the gU and gP blocks
size_t rev_xs_group_floats() { return (size_t)(kXsNB + kXsMB) * 64 * 4; }

hipError_t launch_reverse_xs(int shape, int variant, const RevArgs& a, hipStream_t s) {
  if (!reverse_rs_supports(shape, variant) || !a.xch || !a.xcnt) return hipErrorInvalidValue;
  const int grid = xs_grid(a.B);
  if (variant == DLADMM_V1_LENA) return launch_rrs_em<EM_V1, 4>(a, grid, s);
  if (variant == DLADMM_V2_LTHETA) return launch_rrs_v2(a, grid, 4, s);
  if (variant == DLADMM_V3_FULL) return launch_rrs_v3(a, grid, 4, s);
  if (variant == DLADMM_V6_LASSO) return launch_rrs_em<EM_LASSO, 4>(a, grid, s);
  return launch_rrs_em<EM_VVAR, 4>(a, grid, s);
}

// every variant at the 256 x 512 shape; V2 / V3 get here only after a row-split forward, which the
// plan gives them under DLADMM_F_ROWSPLIT_ROWP (dladmm_capi.hip use_rowsplit)
bool reverse_rs_supports(int shape, int variant) {
  return shape == 2 && variant >= DLADMM_V1_LENA && variant <= DLADMM_V6_LASSO;
}

hipError_t launch_reverse_rs(int shape, int variant, const RevArgs& a, int grid, hipStream_t s) {
  if (!reverse_rs_supports(shape, variant)) return hipErrorInvalidValue;
  if (variant == DLADMM_V1_LENA) return launch_rrs_em<EM_V1>(a, grid, s);
  if (variant == DLADMM_V2_LTHETA) return launch_rrs_v2(a, grid, 1, s);
  if (variant == DLADMM_V3_FULL) return launch_rrs_v3(a, grid, 1, s);
  if (variant == DLADMM_V6_LASSO) return launch_rrs_em<EM_LASSO>(a, grid, s);
  return launch_rrs_em<EM_VVAR>(a, grid, s);
}

}  // namespace dladmm
