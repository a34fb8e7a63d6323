// dladmm_step.h -- the per-element layer step and its adjoint, once, for the fused, row-split,
// split-f16 and per-layer forward kernels and the two reverse sweeps; the bit-for-bit tests
// between those paths hold because they all call the expressions below.  Values in, values out:
// loads, stores, pin_agpr, fences and ablation macros stay with the callers.  An operand a caller
// reads from a table only where it is used (a per-row threshold or step) comes as a callable, so
// the read stays there.  The only memory read here is the uniform per-layer scalar table.
// The two shrink forms (dladmm_common.h) differ in bits and both are kept: the E-step takes the
// form from its threshold's type, ShrinkP = the clamp form shrink_u (the fused kernels' scalar
// thresholds), float = the literal form shrink (their per-row ones; the per-layer epilogue
// throughout).  Not here: dladmm_backward.hip, which forms the shrink derivative as products with
// shrink_d, not as selects -- a different expression with different bits (0 * inf, signed zeros).
#pragma once

#include "dladmm_common.h"
#include "dladmm_internal.h"

namespace dladmm {

// ------------------------------------------------------------------------------ forward
// Uniform per-layer scalars of pass k (k = -1, the prologue: layer 0).  b1n = beta1 of the layer
// whose Var the G2 epilogue of layer k produces (k + 1, clamped).  PK_ROW: no table, all zero.
struct LayerP { float b1n, b2, b3, ss2, ss2b, s1; ShrinkP the, thz; };
// sp: the layer's row of the table; se: the row of the E / L half; sn: the row of b1n's layer
template <int EMODE, int PKIND>
__device__ __forceinline__ LayerP layer_params_at(cfloat_p sp, cfloat_p se, cfloat_p sn) {
  LayerP p{};
  if constexpr (PKIND != PK_ROW) {
    p.b2 = se[DLADMM_P_BETA2];
    // the scalar V1 form (V7) has no beta3: L = L + beta1 T, as everywhere in EM_V1
    p.b3 = (EMODE == EM_V1 && PKIND == PK_S1) ? se[DLADMM_P_BETA1] : se[DLADMM_P_BETA3];
    p.ss2 = se[DLADMM_P_SS2];
    p.ss2b = se[DLADMM_P_SS2B];
    p.the = shrink_params(se[DLADMM_P_THETA_E]);
    p.thz = shrink_params(sp[DLADMM_P_THETA_Z]);
    if constexpr (PKIND == PK_S1) p.s1 = sp[DLADMM_P_S1];
    p.b1n = sn[DLADMM_P_BETA1];
  }
  return p;
}
template <int EMODE, int PKIND>
__device__ __forceinline__ LayerP layer_params(const float* scal, int k, int K, int elz) {
  const int kk = k < 0 ? 0 : k;
  const int kn = k < 0 ? 0 : (k + 1 < K ? k + 1 : k);
  // DLADMM_F_ELZ: pass G2(k) is the E / L half of step k + 1, on that row's slots
  return layer_params_at<EMODE, PKIND>((cfloat_p)scal + kk * DLADMM_NSCALAR,
                                       (cfloat_p)scal + (elz ? kn : kk) * DLADMM_NSCALAR,
                                       (cfloat_p)scal + kn * DLADMM_NSCALAR);
}

// Z = S(U, theta_z), the clamp form also for per-row thresholds (shrink_params(row theta)): for
// theta < 0 it gives Z = 2U exactly where both relus are open, so the backward's masks read off
// the saved Z_k (|Z| < 2|theta|) are exact -- the literal form can round U within an ulp of
// -|theta| to Z = -2|theta| and drop a term there.
__device__ __forceinline__ float z_shrink(float u, ShrinkP thz) { return shrink_u(u, thz); }
// Z_k = S(Z_{k-1} + [s1] q, theta_z), q = -W_k Var (negated packed weights): the reference's
// Z - ss1*fc(Var) operation for operation, main_lena.py:86 / main_syn_l1l1_scalar_tied.py:114
// (s1: V5 only).  thz(): the layer's or the row's ShrinkP.
template <int PKIND, class THZ>
__device__ __forceinline__ float z_step(float zp, float q, float s1, THZ&& thz) {
  const float u = (PKIND == PK_S1) ? zp + s1 * q : zp + q;
  return z_shrink(u, thz());
}

__device__ __forceinline__ float e_shrink(float u, ShrinkP th) { return shrink_u(u, th); }
__device__ __forceinline__ float e_shrink(float u, float th) { return shrink(u, th); }

// E_k, L_k, T_{k+1} of one element from Pv = A Z_k, x = X and the state e0, l0, in the
// reference's operation order; Var_{k+1} = var(beta1_{k+1}), formed where the caller asks (after
// its stores: the schedules are register-tight).  pro (the prologue): E, L stay e0, l0 and
// T_0 = A Z0 + E0 - X (main_lena.py:70).  ss2(), the(): read where used; ss2b: EM_LASSO only.
struct StepOut {
  float e, l, t;
  // Var of the next layer: L + b1*T  (main_lena.py:85)
  __device__ __forceinline__ float var(float b1n) const { return l + b1n * t; }
};
template <int EMODE, class SS2, class THE>
__device__ __forceinline__ StepOut el_step(float Pv, float x, float e0, float l0, float b2,
                                           float b3, float ss2b, bool pro, SS2&& ss2, THE&& the) {
  StepOut o;
  float e;
  if constexpr (EMODE == EM_V1) {
    // E = S(X - A Z - b2*L, theta_e)                      main_lena.py:87
    const float u = (x - Pv) - b2 * l0;
    e = e_shrink(u, the());
  } else if constexpr (EMODE == EM_VVAR) {
    // VVar = L + b2*(A Z + E - X); E = S(E - ss2*VVar)    main_syn_l1l1_scalar.py:114-115
    const float vv = l0 + b2 * ((Pv + e0) - x);
    const float eh = e0 - ss2() * vv;
    e = e_shrink(eh, the());
  } else {
    // E = ss2_1*(X - A Z) - ss2_2*L                       main_syn_lasso_scalar.py:102-103
    e = ss2() * (x - Pv) - ss2b * l0;
  }
  e = pro ? e0 : e;
  const float t = (Pv + e) - x;                            // main_lena.py:70 / :88
  float l = l0 + b3 * t;                                   // main_lena.py:89 / scalar :118
  l = pro ? l0 : l;
  o.e = e;
  o.l = l;
  o.t = t;
  return o;
}

// ------------------------------------------------------------------------------ backward
// G2'(k) scalars: beta1 of BK3's layer k; BK1's layer j (the prologue: j = K - 1); cf = layer j's
// fit coefficient.  ROWP: row-table operands (all zero here but cf).  b1: 64-column sweep only.
struct LP2 { float b1k, b1, b2, b3, ss2, ss2b, the, cf; };
template <bool ROWP>
__device__ __forceinline__ LP2 load_lp2(const float* scal, const float* lcoef, int loss_kind, int k,
                                        int jl, int K) {
  cfloat_p sp = (cfloat_p)scal;
  LP2 p{};
  const int kk = k < K ? k : K - 1;
  const int jj = jl < 0 ? 0 : jl;
  p.cf = loss_kind ? ((cfloat_p)lcoef)[2 * jj + 1] : 0.f;
  if constexpr (ROWP) return p;
  p.b1k = sp[kk * DLADMM_NSCALAR + DLADMM_P_BETA1];
  p.b1 = sp[jj * DLADMM_NSCALAR + DLADMM_P_BETA1];
  p.b2 = sp[jj * DLADMM_NSCALAR + DLADMM_P_BETA2];
  p.b3 = sp[jj * DLADMM_NSCALAR + DLADMM_P_BETA3];
  p.ss2 = sp[jj * DLADMM_NSCALAR + DLADMM_P_SS2];
  p.ss2b = sp[jj * DLADMM_NSCALAR + DLADMM_P_SS2B];
  p.the = sp[jj * DLADMM_NSCALAR + DLADMM_P_THETA_E];
  return p;
}
// G1'(k): the Z-step's mask bound c from theta_z (0 for theta_z >= 0, else 2|theta_z|; ROWP: per
// row, from the row table) and cz_k
__device__ __forceinline__ float z_mask_bound(float th) { return th >= 0.f ? 0.f : -2.0f * th; }
struct LP1 { float c, cz; };
template <bool ROWP>
__device__ __forceinline__ LP1 load_lp1(const float* scal, const float* lcoef, int loss_kind,
                                        int k) {
  const float th = ROWP ? 0.f : ((cfloat_p)scal)[k * DLADMM_NSCALAR + DLADMM_P_THETA_Z];
  return LP1{z_mask_bound(th), loss_kind ? ((cfloat_p)lcoef)[2 * k] : 0.f};
}

// BK2 of one element: gZ = the complete incoming adjoint of Z_k (carried + cotangent + A^T gP_k),
// zk = the saved Z_k, c = z_mask_bound(theta_z).  gU = the adjoint of Z_{k-1}, pth = d/dtheta_z.
struct ZAdj { float gU, pth; };
__device__ __forceinline__ ZAdj z_adjoint(float gZ, float zk, float c, float cz) {
  // + d/dZ_k of cz_k sum|Z_k|: cz_k sgn(Z_k) is exact, so the fma is a mul + add
  const float sg = (zk > 0.f ? 1.f : 0.f) - (zk < 0.f ? 1.f : 0.f);
  const float gZt = __builtin_fmaf(cz, sg, gZ);
  // S'(U) = [U - th > 0] + [-U - th > 0] in {0, 1, 2}, from Z_k = S(U, th); gZt * S' as a sum of
  // selected gZt (exact), d/dth = [-U - th > 0] - [U - th > 0]
  const float ga = zk > -c ? gZt : 0.f, gb = zk < c ? gZt : 0.f;
  return ZAdj{ga + gb, gb - ga};
}

// BK1 of one element of layer j.  In: the adjoints aL, aT, aE of L_j, T_{j+1}, E_j; Pv = A Z_j,
// lp = L_{j-1}, ep = E_{j-1} (EM_VVAR), x = X; the layer's parameters (L-update coefficient: b1
// in EM_V1, else b3); ROWP: per-row theta_e, the forward's literal shrink form, else its clamp
// form; cf, lqm: the fit term's coefficient and L2 (~0) / L1 (0) select mask.  Out: gP (with the
// cf * dfit term), gEp, gLp = the adjoints of P_j, E_{j-1}, L_{j-1}; t = T_{j+1} recomputed; the
// partials p3 (L-update coefficient), p2 (beta2), pe (theta_e), ps2, ps2b.
struct ElAdj { float gP, gEp, gLp, t, p3, p2, pe, ps2, ps2b; };
template <int EMODE, bool ROWP>
__device__ __forceinline__ ElAdj el_adjoint(float aL, float aT, float aE, float Pv, float lp,
                                            float ep, float x, float b1, float b2, float b3,
                                            float ss2, float ss2b, float the, float cf,
                                            uint32_t lqm) {
  ElAdj o{};
  if constexpr (EMODE == EM_V1) {
    const float u = (x - Pv) - b2 * lp;               // main_lena.py:87
    // E_j as the forward formed it
    const float e = ROWP ? shrink(u, the) : shrink_u(u, shrink_params(the));
    o.t = (Pv + e) - x;
    const float gTn = aT + b1 * aL;                   // L_j = L_{j-1} + b1 T_{j+1} (:89)
    o.p3 = aL * o.t;
    const float gEt = aE + gTn;
    // shrink' = [u - th > 0] + [-u - th > 0]: gEt times it as a sum of selected gEt
    const float ga = (u - the) > 0.0f ? gEt : 0.f;
    const float gb = (-u - the) > 0.0f ? gEt : 0.f;
    const float gEh = ga + gb;
    o.pe = gb - ga;                                   // V2's per-row theta_e
    o.gP = gTn - gEh;
    o.p2 = -gEh * lp;
    o.gLp = aL - b2 * gEh;
  } else if constexpr (EMODE == EM_VVAR) {
    const float r0 = (Pv + ep) - x;
    const float vv = lp + b2 * r0;                    // main_syn_l1l1_scalar.py:114
    const float eh = ep - ss2 * vv;                   // :115
    const float e = ROWP ? shrink(eh, the) : shrink_u(eh, shrink_params(the));
    o.t = (Pv + e) - x;
    const float gTn = aT + b3 * aL;
    o.p3 = aL * o.t;
    const float gEt = aE + gTn;
    const float ga = (eh - the) > 0.0f ? gEt : 0.f;
    const float gb = (-eh - the) > 0.0f ? gEt : 0.f;
    const float gEh = ga + gb;
    o.pe = gb - ga;
    const float gVV = -ss2 * gEh;
    o.ps2 = -gEh * vv;
    o.gLp = aL + gVV;
    o.p2 = gVV * r0;
    o.gP = gTn + b2 * gVV;
    o.gEp = gEh + b2 * gVV;
  } else {
    const float e = ss2 * (x - Pv) - ss2b * lp;       // main_syn_lasso_scalar.py:102-103
    o.t = (Pv + e) - x;
    const float gTn = aT + b3 * aL;
    o.p3 = aL * o.t;
    const float gEt = aE + gTn;
    o.ps2 = gEt * (x - Pv);
    o.gP = gTn - ss2 * gEt;
    o.ps2b = -gEt * lp;
    o.gLp = aL - ss2b * gEt;
  }
  {  // d/dP of cf * fit (fit = sum|X - P|, torch sgn(0) = 0, or 0.5 sum (X - P)^2)
    const float res = x - Pv;
    const float sg = (res > 0.f ? 1.f : 0.f) - (res < 0.f ? 1.f : 0.f);
    // uniform select by bit mask (a per-row branch here splits the unrolled body)
    const float dfit = __builtin_bit_cast(
        float, (lqm & __builtin_bit_cast(uint32_t, res)) | (~lqm & __builtin_bit_cast(uint32_t, sg)));
    o.gP = o.gP - cf * dfit;
  }
  return o;
}
// Var of BK3's layer k from BK1's recomputed values: L_j + beta1_k T_{j+1}, the forward's own
// expression (l = L_{j-1} + c T_{j+1}, c = the L-update coefficient), so T is never loaded.
template <int EMODE>
__device__ __forceinline__ float var_k(float lp, float t, float b1, float b3, float b1k) {
  const float lcoef = EMODE == EM_V1 ? b1 : b3;
  const float lk = lp + lcoef * t;
  return lk + b1k * t;
}

}  // namespace dladmm
