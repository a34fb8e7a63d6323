// dladmm_lskm_lena_fused.h -- host-side contract between dladmm_lskm_lena_f32 (dladmm_capi.hip)
// and the one-launch safeguarded LSKM forward of the lena (V1) model
// (dladmm_lskm_lena_fused.hip).
#pragma once

#include "dladmm_internal.h"

namespace dladmm {

struct LskmLenaArgs {
  int m, n, B, K;
  const float* X;  int64_t ldx;
  const float* Z0; int64_t ldz0;
  const float* E0; int64_t lde0;
  const float* L0; int64_t ldl0;
  const float* Ap;    // packed A             [MB/2][NB][2] fragments (pack order 2)
  const float* Atp;   // packed -A^T          [NB/2][MB][2]: the KM step's weight
  const float* Wp;    // packed -W_k       [K][NB/2][MB][2]
  const float* const* b1t;  // device table [K]: beta1_k (m, B), row stride ldb
  const float* const* b2t;  // device table [K]: beta2_k
  int64_t ldb;
  const float* scal;  // [K][8]: the learned (V1) layers' uniform slots (theta_z, theta_e)
  const float* km;    // [8]: the KM step (beta = s1 = ss1, ss2 = theta_e, theta_z = ss1 alpha)
  float *Zo, *Eo, *Lo; int64_t ldo;        // Z / E / L [K][.][ldo]
  int* count;         // [K], zeroed before the launch
  float* mu_out;      // [B] or null: mu after the last layer
  float thresh, param;                     // thresh = (float)(1 - delta)
  int updater;
};
static_assert(sizeof(LskmLenaArgs) <= 2048, "kernel argument size");

// the 256 x 512 register shape only; grid = ceil(B / 16)
hipError_t launch_lskm_lena_fused(const LskmLenaArgs& a, int grid, hipStream_t s);

}  // namespace dladmm
