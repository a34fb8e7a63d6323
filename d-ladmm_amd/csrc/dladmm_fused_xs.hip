// dladmm_fused_xs.hip -- path 6, the row-split forward for the SMALLEST batches with four
// workgroups (on four CUs) per 16 batch columns (dladmm_fused_rs_kernel.h, MEM = 4; the hand-off
// between the members: dladmm_group_xchg.h): its instantiations, grid and dispatch.
#include "dladmm_fused_rs_kernel.h"

namespace dladmm {

// the groups padded to whole stripes (GroupXchg's block -> (group, member) mapping)
int xs_grid(int64_t B) {
  const int64_t groups = (B + 15) / 16;
  return (int)(((groups + kXsStripe - 1) / kXsStripe) * kXsStripe * kXsMembers);
}

// a group's exchange buffer: the Z and Var blocks, then the objective partials [2][waves][16]
size_t xs_group_floats() { return (size_t)(kXsNB + kXsMB) * 64 * 4 + 2 * kXsWaves * 16; }

hipError_t launch_fused_xs(int shape, int variant, const FusedArgs& a, hipStream_t s) {
  if (shape != 2 || !a.xch || !a.xcnt || a.elz) return hipErrorInvalidValue;
  return with_variant_modes(variant, [&](auto EM_, auto PK_) {
    return launch_fused_rs_as<decltype(EM_)::value, decltype(PK_)::value, false, kXsMembers>(
        a, xs_grid(a.B), s);
  });
}

}  // namespace dladmm
