// dladmm_lskm_rowp_fused.h -- host-side contract between dladmm_lskm_rowp_f32 (dladmm_capi.hip)
// and the one-launch safeguarded LSKM forward of the per-row models V2 / V3
// (dladmm_lskm_rowp_fused.hip).
#pragma once

#include "dladmm_internal.h"

namespace dladmm {

struct LskmRowpArgs {
  int m, n, B, K;
  const float* X;  int64_t ldx;
  const float* Z0; int64_t ldz0;
  const float* E0; int64_t lde0;
  const float* L0; int64_t ldl0;
  const float* Ap;    // packed A             [MB/2][NB][2] fragments (pack order 2)
  const float* Atp;   // packed -A^T          [NB/2][MB][2]: the KM step's weight
  const float* Wp;    // packed -W_k       [K][NB/2][MB][2]
  const float* rowp; int64_t rstride;  // [K][8][rstride]: the learned layers' per-row table
  const float* km;    // [8]: the KM step (beta, ss2, theta_e, theta_z = ss1 alpha, s1 = ss1)
  float *Zo, *Eo, *Lo, *To; int64_t ldo;   // Z / E / L [K][.][ldo], T [K + 1][m][ldo]
  int* count;         // [K], zeroed before the launch
  float* mu_out;      // [B] or null: mu after the last layer
  float beta, c, thresh, param;            // thresh = (float)(1 - delta)
  int updater;
};
static_assert(sizeof(LskmRowpArgs) <= 2048, "kernel argument size");

// the 256 x 512 register shape only; grid = ceil(B / 16); variant: DLADMM_V2_LTHETA (EM_V1) or
// DLADMM_V3_FULL (EM_VVAR)
hipError_t launch_lskm_rowp_fused(int variant, const LskmRowpArgs& a, int grid, hipStream_t s);

}  // namespace dladmm
