// dladmm_reverse_rs_v3.hip -- row-split reverse-sweep instantiations: V3 (main_syn_l1l1_full.py),
// per-row parameters, E-step form EM_VVAR; one workgroup (bwd path 2) and four workgroups (bwd
// path 3) per 16 columns (dladmm_reverse_rs_kernel.h; dispatch: dladmm_reverse_rs.hip).
#include "dladmm_reverse_rs_kernel.h"

namespace dladmm {

hipError_t launch_rrs_v3(const RevArgs& a, int grid, int mem, hipStream_t s) {
  if (!a.rowp || !a.rpart) return hipErrorInvalidValue;
  return mem == 4 ? launch_rrs_em<EM_VVAR, 4, true>(a, grid, s)
                  : launch_rrs_em<EM_VVAR, 1, true>(a, grid, s);
}

}  // namespace dladmm
