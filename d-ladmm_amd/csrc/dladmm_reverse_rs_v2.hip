// dladmm_reverse_rs_v2.hip -- row-split reverse-sweep instantiations: V2 (main_syn_l1l1_ltheta.py),
// per-row parameters, E-step form EM_V1; one workgroup (bwd path 2) and four workgroups (bwd
// path 3) per 16 columns (dladmm_reverse_rs_kernel.h; dispatch: dladmm_reverse_rs.hip).
#include "dladmm_reverse_rs_kernel.h"

namespace dladmm {

hipError_t launch_rrs_v2(const RevArgs& a, int grid, int mem, hipStream_t s) {
  if (!a.rowp || !a.rpart) return hipErrorInvalidValue;
  return mem == 4 ? launch_rrs_em<EM_V1, 4, true>(a, grid, s)
                  : launch_rrs_em<EM_V1, 1, true>(a, grid, s);
}

}  // namespace dladmm
