// dladmm_fused_p0.hip -- the load-P0 form of the fused K-layer forward (inference form) and the
// kernel that produces P0 = A Z0.  The kernel template and its design notes:
// dladmm_fused_kernel.h (P0LOAD); the caller's contract: include/dladmm.h (DLADMM_F_P0_SAVE /
// DLADMM_F_P0_REUSE).
#include "dladmm_fused_kernel.h"

namespace dladmm {

// P0 [MP][ldp] = Ap Z0, bit-identical to what the compute form's prologue pass hands its rows:
// the same packed fragments, the same v_mfma_f32_16x16x4_f32 sequence per output element (kb
// ascending; sub-steps x, z on one accumulator, y, w on a second, one add: DLADMM_G2_CHAINS).
// One wave per 16 columns, runtime loops, Z0 re-read per output pair: slow (it runs once per
// cache fill), small.  Padded rows and columns are written too (exact zeros), so the whole
// region is defined.
__global__ __launch_bounds__(256) void p0_kernel(const float* Ap, const float* Z0, int64_t ldz0,
                                                  int n, int64_t B, float* P0, int64_t ldp,
                                                  int MB, int NB) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int j = lane & 15, g = lane >> 4;
  const int64_t col = (int64_t)blockIdx.x * kTileCols + w * 16 + j;
  const rsrc_t rz = mkrsrc(Z0, (uint32_t)(n * ldz0 * 4));
  const uint32_t oz = col < B ? (uint32_t)((col + (int64_t)(4 * g) * ldz0) * 4) : kOOB;
  const f32x4* ap = reinterpret_cast<const f32x4*>(Ap);
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  for (int p = 0; p < MB / 2; ++p) {
    f32x4 ca = zero4, cb = zero4;
#if DLADMM_G2_CHAINS == 2
    f32x4 ca2 = zero4, cb2 = zero4;
#endif
    for (int kb = 0; kb < NB; ++kb) {
      float z[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) z[r] = bload(rz, oz + (uint32_t)((16 * kb + r) * ldz0 * 4));
      const f32x4 wa = ap[((int64_t)(p * NB + kb) * 2 + 0) * 64 + lane];
      const f32x4 wb = ap[((int64_t)(p * NB + kb) * 2 + 1) * 64 + lane];
#if DLADMM_G2_CHAINS == 2
      ca = mfma4(wa.x, z[0], ca);
      cb = mfma4(wb.x, z[0], cb);
      ca2 = mfma4(wa.y, z[1], ca2);
      cb2 = mfma4(wb.y, z[1], cb2);
      ca = mfma4(wa.z, z[2], ca);
      cb = mfma4(wb.z, z[2], cb);
      ca2 = mfma4(wa.w, z[3], ca2);
      cb2 = mfma4(wb.w, z[3], cb2);
#else
      ca = mfma4(wa.x, z[0], ca);
      cb = mfma4(wb.x, z[0], cb);
      ca = mfma4(wa.y, z[1], ca);
      cb = mfma4(wb.y, z[1], cb);
      ca = mfma4(wa.z, z[2], ca);
      cb = mfma4(wb.z, z[2], cb);
      ca = mfma4(wa.w, z[3], ca);
      cb = mfma4(wb.w, z[3], cb);
#endif
    }
#if DLADMM_G2_CHAINS == 2
    const f32x4 qa = ca + ca2, qb = cb + cb2;
#else
    const f32x4 qa = ca, qb = cb;
#endif
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      P0[(int64_t)(16 * (2 * p) + 4 * g + r) * ldp + col] = qa[r];
      P0[(int64_t)(16 * (2 * p + 1) + 4 * g + r) * ldp + col] = qb[r];
    }
  }
}

hipError_t launch_p0_producer(int shape, const float* Ap, const float* Z0, int64_t ldz0, int n,
                              int64_t B, float* P0, int64_t ldp, int grid, hipStream_t s) {
  if (shape < 0 || shape >= kNumShapes || ldp < (int64_t)grid * kTileCols)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(p0_kernel, dim3(grid), dim3(256), 0, s, Ap, Z0, ldz0, n, B, P0, ldp,
                     kShapeMP[shape] / 16, kShapeNP[shape] / 16);
  return hipGetLastError();
}

// every instantiation of the load form fits its register budget (DESIGN: the census)
bool p0_supports(int shape, int variant) {
  return shape >= 0 && shape < kNumShapes && variant >= DLADMM_V1_LENA &&
         variant <= DLADMM_V6_LASSO;
}

template <int MP, int NP>
hipError_t dispatch_variant_p0(int variant, const FusedArgs& a, int grid, hipStream_t s) {
  switch (variant) {
    case DLADMM_V1_LENA: return launch_fused<MP, NP, EM_V1, PK_ELEM, false, true>(a, grid, s);
    case DLADMM_V2_LTHETA: return launch_fused<MP, NP, EM_V1, PK_ROW, false, true>(a, grid, s);
    case DLADMM_V3_FULL: return launch_fused<MP, NP, EM_VVAR, PK_ROW, false, true>(a, grid, s);
    case DLADMM_V4_SCALAR: return launch_fused<MP, NP, EM_VVAR, PK_SCALAR, false, true>(a, grid, s);
    case DLADMM_V5_TIED: return launch_fused<MP, NP, EM_VVAR, PK_S1, false, true>(a, grid, s);
    case DLADMM_V6_LASSO: return launch_fused<MP, NP, EM_LASSO, PK_SCALAR, false, true>(a, grid, s);
  }
  return hipErrorInvalidValue;
}

hipError_t launch_fused_shape_p0(int shape, int variant, const FusedArgs& a, int grid,
                                 hipStream_t s) {
  switch (shape) {
    case 0: return dispatch_variant_p0<kShapeMP[0], kShapeNP[0]>(variant, a, grid, s);
    case 1: return dispatch_variant_p0<kShapeMP[1], kShapeNP[1]>(variant, a, grid, s);
    case 2: return dispatch_variant_p0<kShapeMP[2], kShapeNP[2]>(variant, a, grid, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace dladmm
