// dladmm_lskm_news_fused.h -- host-side contract between dladmm_lskm_news_f32 (dladmm_capi.hip)
// and the one-launch safeguarded newS LSKM forward (dladmm_lskm_news_fused.hip).
#pragma once

#include "dladmm_internal.h"

namespace dladmm {

struct LskmNewsArgs {
  int m, n, B, K;
  const float* X;  int64_t ldx;
  const float* Z0; int64_t ldz0;
  const float* E0; int64_t lde0;
  const float* L0; int64_t ldl0;
  const float* Ap;    // packed A             [MB/2][NB][2] fragments (pack order 2)
  const float* Atp;   // packed -A^T          [NB/2][MB][2]: the KM step's weight
  const float* const* wtab;  // device [K]: layer k's packed -W [NB/2][MB][2] (entries may repeat)
  const float* scal;  // [K][8], unshifted: step k takes its E / L slots from row k - 1
  const float* km;    // [8]: the KM step (V7: beta, theta_e = ss2, theta_z = ss1 alpha, s1 = ss1)
  const float* inv_bs;  // device scalar 1 / (beta ss1)
  float *Zo, *Eo, *Lo; int64_t ldo;   // Z / E / L [K][.][ldo]
  int* count;         // [K], zeroed before the launch
  uint8_t* mask;      // [K][B] keep decisions, or null
  float* mu_out;      // [B] or null: mu after the last layer
  float thresh, param;                // thresh = (float)(1 - delta)
  int updater;
};
static_assert(sizeof(LskmNewsArgs) <= 2048, "kernel argument size");

// the 256 x 512 register shape only; grid = ceil(B / 16)
hipError_t launch_lskm_news_fused(const LskmNewsArgs& a, int grid, hipStream_t s);

}  // namespace dladmm
