// dladmm_sl2.h -- host-side contract between dladmm_sl2_f32 (dladmm_capi.hip) and the fused S-L2
// training term: one classic KM step from the network's last state, its squared residual norm
// per column and the adjoint of that norm (dladmm_sl2.hip).
#pragma once

#include "dladmm_internal.h"

namespace dladmm {

struct Sl2Args {
  int m, n, B;
  const float* X;  int64_t ldx;
  const float* Z;  int64_t ldz;
  const float* E;  int64_t lde;
  const float* L;  int64_t ldl;
  const float* T;  int64_t ldt;
  const float* Ep; int64_t ldep;
  const float* Ap;    // packed A     [MB/2][NB][2] fragments (pack order 2)
  const float* Atp;   // packed -A^T  [NB/2][MB][2]
  const float* coef;  // device scalar w (the adjoint form only)
  double* colsum;     // [B]
  float *gZ, *gE, *gL, *gT, *gEp; int64_t ldg;   // the adjoint form; gEp may be null
  float beta, ss1, ss2, thz, c;
};

// the 256 x 512 register shape only; grid = ceil(B / 16); grad: also the five cotangents
hipError_t launch_sl2(const Sl2Args& a, bool grad, int grid, hipStream_t s);
// total[0] = colsum[0] + ... + colsum[B - 1] in a fixed order (one wave)
hipError_t launch_sl2_total(const double* colsum, int B, double* total, hipStream_t s);

}  // namespace dladmm
