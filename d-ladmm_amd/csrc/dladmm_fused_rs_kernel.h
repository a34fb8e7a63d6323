// dladmm_fused_rs_kernel.h -- the fused K-layer forward for SMALL batches: a group of 16 batch
// columns per MEM workgroups, the ROWS of every product split over the group's WPG = 4 MEM waves
// (the forward twin of dladmm_reverse_rs_kernel.h).
//
// The fused kernel (dladmm_fused_kernel.h) gives each wave 16 columns and ALL rows: a workgroup
// covers 64 columns, so a batch of B columns occupies ceil(B / 64) CUs and every layer costs one
// CU's time for both products over all rows (the KM ground truth of test_syn_l1l1_scalar.py:478,
// K = 2000 at B = 20 .. 1,000, ran at 67 us per step on 1-16 of the 256 CUs).
// Here wave v = 4 member + w of the group owns a 1 / WPG of the output rows of each product:
//   G1 (Z = S(Z - s1 W_k Var)): output blocks NB4 v .. of n (NP = 512), contraction over all m;
//   G2 (A Z_k and the E / L / T / Var updates): blocks MB4 v .. of m (MP = 256), over all n.
// MEM = 1 (path 5, dladmm_fused_rs.hip): one workgroup, 8 G1 and 4 G2 blocks per wave.  Its 4
//   SIMDs run every MFMA of both products, ~15 us of f32 MFMA cycles per layer whatever the batch.
// MEM = 4 (path 6, dladmm_fused_xs.hip): four workgroups on four CUs, one G1 pair and one G2
//   block (half of A pair v / 2) per wave, a quarter of path 5's MFMAs per SIMD: for batches
//   (20 columns: main_lena.py:155) that leave nearly every CU idle.
// Each product's B operand (Var, then Z_k) is the group's whole column state, so the waves
// exchange it once per product: through LDS and a barrier, or between the members through the
// group's exchange buffer (dladmm_group_xchg.h).  The weight fragments come straight from L2 by
// buffer loads, a few steps ahead, with compiler-counted waits (no LDS ring).
//
// Arithmetic is the fused kernel's, operation for operation: the same packed -W_k / A fragments
// (pack order 2), G1 one fma chain per output block over k in order, G2 two chains (k sub-steps
// x, z and y, w) summed once, the same elementwise expressions -- so the outputs are the fused
// kernel's bit for bit (tests/test_gpu_rowsplit.py), the saved products P_k = A Z_k of a
// training forward too.  The fused per-column objective is the same sum in another order (each
// wave sums its rows, then the WPG partials in wave order): equal to fp32 rounding.
// Scope: every variant at the 256 x 512 register shape, fp32; the plan (dladmm_capi.hip) picks
// it for batches that leave most CUs idle on the fused kernel.  V2 / V3 (per-row parameters,
// PK_ROW) run it under DLADMM_F_ROWSPLIT_ROWP: a wave reads the row-table entries of its own
// rows with each output pair (the 16 lanes of a row on one address), the fused kernel's PK_ROW
// expressions (Z the clamp form of shrink, E the literal one; tests/test_gpu_rowsplit_rowp.py).
#pragma once
#include "dladmm_group_xchg.h"
#include "dladmm_step.h"

#ifndef RS_PF
#define RS_PF 4  // path 5's weight-fragment read-ahead (MFMA steps) per wave: 2, 4 and 8 time the
                 // same (profiles/r06_rowsplit_ab.json) -- each CU fetches the whole weight pair
                 // per step for its 16 columns (1 MiB at 256 x 512), ~45 GB/s per CU at 22 us/step
#endif
#ifndef XS_PF
#define XS_PF 8  // path 6's: its waves wait on the weight stream rather than on their MFMAs
#endif

namespace dladmm {

// ELZ: the DLADMM_F_ELZ entry / exit modes (a.elz = 1, or 2 with the tail), a compile-time
// parameter as in the fused kernel: instantiated for V4 / V5 / V7 on path 5, and every
// instantiation without it is instruction for instruction what it was.
template <int MP, int NP, int EMODE, int PKIND, bool ELZ, int MEM>
__global__ __launch_bounds__(256, 1) void fused_rs_kernel(const FusedArgs a) {
  static_assert(!(ELZ && MEM > 1), "the ELZ modes run on path 5 only");
  constexpr int MB = MP / 16, NB = NP / 16;
  constexpr int WPG = kWaves * MEM;                  // waves per 16-column group
  constexpr int NB4 = NB / WPG, MB4 = MB / WPG;      // output blocks per wave
  static_assert(NB4 % 2 == 0 && (MB4 % 2 == 0 || MB4 == 1),
                "G1 whole pairs; G2 pairs or one block");
  constexpr int HP = MB4 >= 2 ? 2 : 1;               // G2 blocks per output step group
  constexpr int S1 = (NB4 / 2) * MB, S2 = (MB4 / HP) * NB;  // MFMA steps of a wave's G1 / G2
  constexpr int PF = MEM > 1 ? XS_PF : RS_PF;        // weight-fragment read-ahead
  constexpr bool kElem = PKIND == PK_ELEM;  // V1: per-sample betas (m, B) of every layer
  constexpr bool kRow = PKIND == PK_ROW;    // V2 / V3: per-row parameters [K][8][rstride]
  __shared__ f32x4 zx[NB * 64];  // Z_k of the 16 columns, block b at zx[b * 64 + lane]
  __shared__ f32x4 vx[MB * 64];  // Var
  __shared__ float red[kWaves][2][16];  // path 5: per-wave column partials of the fused objective

  GroupXchg<MEM> X;
  const int grp = X.grp, mem = X.mem;
  if (MEM > 1 && grp * 16 >= a.B) return;   // a padding group: every member leaves
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int v = mem * kWaves + w;           // wave of the group
  const int g = lane >> 4;
  const int64_t col = (int64_t)grp * 16 + (lane & 15);
  const bool cv = col < a.B;
  const int m = a.m, n = a.n, K = a.K;
  const bool lossz = a.loss_kind != 0;
  const bool lasso = __builtin_amdgcn_readfirstlane(a.loss_kind) == DLADMM_LOSS_LASSO;
  auto lane_off = [&](int64_t ld) -> uint32_t {
    return cv ? (uint32_t)((col + (int64_t)(4 * g) * ld) * 4) : kOOB;
  };
  const int elz = ELZ ? __builtin_amdgcn_readfirstlane(a.elz) : 0;
  const int b1o = v * NB4, b2o = v * MB4;  // first output block of this wave in G1 / G2

  // path 6, the group's exchange buffer: Z blocks [NB][64] f32x4, Var blocks [MB][64], then the
  // objective partials [2][WPG waves][16 columns]
  f32x4* xz = (f32x4*)(MEM > 1 ? a.xch + (int64_t)grp * a.xstride : nullptr);
  const rsrc_t rxz = mkrsrc((const float*)xz, MEM > 1 ? (uint32_t)(NB * 64 * 16) : 0u);
  const rsrc_t rxv = mkrsrc((const float*)(xz + NB * 64), MEM > 1 ? (uint32_t)(MB * 64 * 16) : 0u);
  const rsrc_t rxl = mkrsrc((const float*)(xz + (NB + MB) * 64),
                            MEM > 1 ? (uint32_t)(2 * WPG * 16 * 4) : 0u);
  X.join(a.xcnt);

  float Zr[NB4][4], Er[MB4][4], Lr[MB4][4], Xr[MB4][4];
  {
    const rsrc_t rz = mkrsrc(a.Z0, (uint32_t)(n * a.ldz0 * 4));
    const rsrc_t re = mkrsrc(a.E0, (uint32_t)(m * a.lde0 * 4));
    const rsrc_t rl = mkrsrc(a.L0, (uint32_t)(m * a.ldl0 * 4));
    const rsrc_t rx = mkrsrc(a.X, (uint32_t)(m * a.ldx * 4));
    const uint32_t oz = lane_off(a.ldz0), oe = lane_off(a.lde0), ol = lane_off(a.ldl0),
                   ox = lane_off(a.ldx);
    // Z0 into LDS (an input: no hand-off): path 6, every block of the group, a quarter per wave;
    // path 5, each wave its own blocks.  This wave's blocks into registers
    if constexpr (MEM > 1) {
      for (int b = w; b < NB; b += kWaves) {
        f32x4 zv;
#pragma unroll
        for (int r = 0; r < 4; ++r) zv[r] = bload(rz, oz + (uint32_t)((16 * b + r) * a.ldz0 * 4));
        zx[b * 64 + lane] = zv;
      }
    }
#pragma unroll
    for (int b = 0; b < NB4; ++b) {
      f32x4 zv;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        Zr[b][r] = bload(rz, oz + (uint32_t)((16 * (b1o + b) + r) * a.ldz0 * 4));
        zv[r] = Zr[b][r];
      }
      if constexpr (MEM == 1) zx[(b1o + b) * 64 + lane] = zv;
    }
#pragma unroll
    for (int b = 0; b < MB4; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint32_t ro = (uint32_t)(16 * (b2o + b) + r);
        Xr[b][r] = bload(rx, ox + ro * (uint32_t)(a.ldx * 4));
        Er[b][r] = bload(re, oe + ro * (uint32_t)(a.lde0 * 4));
        Lr[b][r] = bload(rl, ol + ro * (uint32_t)(a.ldl0 * 4));
      }
  }

  float regsum = 0.f, fit1 = 0.f, fit2 = 0.f;  // this wave's rows of the layer's objective
  // V1: per-element betas of the G2 epilogue rows (b3 = beta1_k, b2 = beta2_k, b1n = beta1_k+1),
  // loaded at the start of the pass (scalar-loaded layer pointers, as the fused kernel)
  float pb[kElem ? MB4 : 1][3][4];
  const uint32_t vb = lane_off(a.ldb);
  auto load_betas = [&](int k) {
    if constexpr (kElem) {
      typedef const float* const __attribute__((address_space(4)))* ctab_p;
      const ctab_p t1 = (ctab_p)a.b1t, t2 = (ctab_p)a.b2t;
      const int kk = k < 0 ? 0 : k, kn = k + 1 < K ? k + 1 : kk;
      const uint32_t eb = (uint32_t)(m * a.ldb * 4);
      const rsrc_t r1 = mkrsrc(k < 0 ? nullptr : t1[kk], k < 0 ? 0u : eb);
      const rsrc_t r2 = mkrsrc(k < 0 ? nullptr : t2[kk], k < 0 ? 0u : eb);
      const rsrc_t rn = mkrsrc(k + 1 < K ? t1[kn] : nullptr, k + 1 < K ? eb : 0u);
#pragma unroll
      for (int b = 0; b < MB4; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const uint32_t so = (uint32_t)(16 * (b2o + b) + r) * (uint32_t)(a.ldb * 4);
          pb[b][0][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r1, (int)vb, (int)so, 0));
          pb[b][1][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r2, (int)vb, (int)so, 0));
          pb[b][2][r] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rn, (int)vb, (int)so, 0));
        }
    }
  };
  // V2 / V3: view of `slot` of layer kk of the row table, bounded to the slot's rows (theta_z: n,
  // the others: m) -- the padded rows read 0, a finite parameter that meets their all-zero state
  // (the fused kernel's row_tab_load clamps the row instead; either way they stay zero).  Lane
  // offset: row 4 g of a block; the block and row go in the uniform offset
  const uint32_t vr = (uint32_t)(16 * g);
  auto row_view = [&](int kk, int slot) -> rsrc_t {
    const int lim = slot == DLADMM_P_THETA_Z ? n : m;
    return mkrsrc(kRow ? a.rowp + ((int64_t)kk * 8 + slot) * a.rstride : nullptr,
                  kRow ? (uint32_t)(lim * 4) : 0u);
  };
  auto row_ld = [&](rsrc_t r, int b, int rr) -> float {
    uint32_t o = (uint32_t)(64 * b);
    if constexpr (MEM == 1) asm volatile("" : "+s"(o));  // path 5: formed where it is used
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)vr, (int)(o + 4 * rr), 0));
  };
  // the layer's per-column objective (fused kernel: flush_loss): each wave's rows summed over its
  // lane groups and staged (path 5: LDS; path 6: the exchange buffer, handed off with the Var
  // blocks), then the WPG partials in wave order by the group's wave 0 after the hand-off
  auto stage_loss = [&]() {
    const float rs_ = col_sum(regsum), fs = col_sum(lasso ? fit2 : fit1);
    if (g == 0) {
      if constexpr (MEM == 1) {
        red[w][0][lane] = rs_;
        red[w][1][lane] = fs;
      } else {
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, rs_), rxl, (v * 16 + lane) * 4, 0, 16);
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, fs), rxl,
                                              ((WPG + v) * 16 + lane) * 4, 0, 16);
      }
    }
    regsum = fit1 = fit2 = 0.f;
  };
  auto flush_loss = [&](int k) {  // after the hand-off that follows stage_loss
    if (mem == 0 && w == 0 && g == 0) {
      auto part = [&](int t, int q) -> float {
        if constexpr (MEM == 1) return red[q][t][lane];
        else return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                        rxl, ((t * WPG + q) * 16 + lane) * 4, 0, 16));
      };
      float r0 = part(0, 0), f0 = part(1, 0);
#pragma unroll
      for (int q = 1; q < WPG; ++q) {
        r0 += part(0, q);
        f0 += part(1, q);
      }
      // every slot of the group, padding columns too (their sums are zero): the reduction
      // reads ldl = 16 * groups columns
      a.lossp[(int64_t)(2 * k + 0) * a.ldl + col] = X.fin(r0);
      a.lossp[(int64_t)(2 * k + 1) * a.ldl + col] = X.fin(lasso ? 0.5f * f0 : f0);
    }
  };

  const uint32_t vo = lane_off(a.ldo);
  const uint32_t ld4 = (uint32_t)(a.ldo * 4);
  const uint32_t zbytes = (uint32_t)(n * a.ldo * 4), mbytes = (uint32_t)(m * a.ldo * 4);
  const int64_t wl = (int64_t)MB * NB * kFrag;  // floats per packed weight
  const uint32_t vf = (uint32_t)(lane * 16);    // lane offset inside a 1-KiB fragment
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  auto frag = [&](rsrc_t r, int off) -> f32x4 {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)vf, off, 0));
  };
  // byte offset of row 16 b + r of a [rows][ldo] output (an opaque base, so the per-block values
  // are formed where they are used rather than all kept live across the layer loop)
  auto row_off = [&](int b, int r) -> uint32_t {
    uint32_t o = (uint32_t)(16 * b) * ld4;
    asm volatile("" : "+s"(o));
    return o + (uint32_t)r * ld4;
  };

  // The weight-fragment window: step s of a pass reads slot s % PF and refills it with step
  // s + PF.  Pack order 2 puts output pair P's k-block kb at fragments 2 (P KB + kb) + h, so a
  // wave's pairs are one contiguous run: its buffer view starts at its first pair and step s
  // reads fragments 2s, 2s + 1 (compile-time offsets).  G2 with one block per wave (HP = 1) reads
  // half b2o & 1 of A pair b2o / 2: fragment 2s of a view that starts at that half.
  // Path 5 opens a window per pass; path 6 has this one, whose first PF steps are fetched inside
  // the hand-off before the pass (pre1 / pre2)
  f32x4 xfa[MEM > 1 ? PF : 1], xfb[MEM > 1 ? PF : 1];
  auto fetch = [&](auto H2_, rsrc_t r, auto S_, f32x4* fa, f32x4* fb) {
    constexpr int s = decltype(S_)::value;
    fa[s % PF] = frag(r, 2 * s * 1024);
    if constexpr (decltype(H2_)::value) fb[s % PF] = frag(r, (2 * s + 1) * 1024);
  };
  auto prefetch = [&](auto H2_, auto NS_, rsrc_t r, f32x4* fa, f32x4* fb) {  // the first PF steps
    static_for<PF>([&](auto I_) {
      if constexpr (decltype(I_)::value < decltype(NS_)::value) fetch(H2_, r, I_, fa, fb);
    });
  };
  constexpr auto kS1 = std::integral_constant<int, S1>{};
  constexpr auto kS2 = std::integral_constant<int, S2>{};
  constexpr auto kH2 = std::integral_constant<bool, HP == 2>{};
  auto rw_of = [&](int k) -> rsrc_t {
    const float* wk = a.Wp + (int64_t)(k * a.wstep) * wl + (int64_t)(b1o / 2) * MB * 2 * kFrag;
    return mkrsrc(wk, (uint32_t)(S1 * 2 * kFrag * 4));
  };
  const rsrc_t ra =
      HP == 2 ? mkrsrc(a.Ap + (int64_t)(b2o / 2) * NB * 2 * kFrag, (uint32_t)(S2 * 2 * kFrag * 4))
              : mkrsrc(a.Ap + ((int64_t)(b2o >> 1) * NB * 2 + (b2o & 1)) * kFrag,
                       (uint32_t)((2 * S2 - 1) * kFrag * 4));
  auto pre1 = [&](int k) { prefetch(std::true_type{}, kS1, rw_of(k), xfa, xfb); };
  auto pre2 = [&]() { prefetch(kH2, kS2, ra, xfa, xfb); };  // A: the same every layer

  // G1(k): this wave's Z blocks; Var (all m rows) from vx
  auto g1_body = [&](int k, const LayerP& P, rsrc_t rzo, rsrc_t rw, f32x4* fa, f32x4* fb) {
    const rsrc_t rtz = row_view(k, DLADMM_P_THETA_Z);
    static_for<NB4 / 2>([&](auto P_) {
      constexpr int pp = decltype(P_)::value;
      f32x4 ca = zero4, cb = zero4;
      float tz[2][4];  // V2 / V3: theta_z of the pair's rows, in flight across its products
      if constexpr (kRow) {
#pragma unroll
        for (int h = 0; h < 2; ++h)
#pragma unroll
          for (int r = 0; r < 4; ++r) tz[h][r] = row_ld(rtz, b1o + 2 * pp + h, r);
      }
      static_for<MB>([&](auto J_) {
        constexpr int jb = decltype(J_)::value;
        constexpr int s = pp * MB + jb;
        const f32x4 vv = vx[jb * 64 + lane];
        const f32x4 wa = fa[s % PF], wb = fb[s % PF];
        if constexpr (s + PF < S1)
          fetch(std::true_type{}, rw, std::integral_constant<int, s + PF>{}, fa, fb);
        ca = mfma4(wa.x, vv[0], ca);
        cb = mfma4(wb.x, vv[0], cb);
        ca = mfma4(wa.y, vv[1], ca);
        cb = mfma4(wb.y, vv[1], cb);
        ca = mfma4(wa.z, vv[2], ca);
        cb = mfma4(wb.z, vv[2], cb);
        ca = mfma4(wa.w, vv[3], ca);
        cb = mfma4(wb.w, vv[3], cb);
      });
      // the Z-step (z_step, dladmm_step.h)
      static_for<2>([&](auto H_) {
        constexpr int h = decltype(H_)::value;
        constexpr int lb = 2 * pp + h;
        const f32x4 q = h ? cb : ca;
        f32x4 zv;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float z = z_step<PKIND>(Zr[lb][r], q[r], P.s1, [&]() -> ShrinkP {
            if constexpr (kRow) return shrink_params(tz[h][r]);
            else return P.thz;
          });
          Zr[lb][r] = z;
          zv[r] = z;
          bstore_s(rzo, vo, row_off(b1o + lb, r), X.fin(z));
          regsum += fabsf(z);
        }
        if constexpr (MEM == 1) zx[(b1o + lb) * 64 + lane] = zv;
        else X.xstore(rxz, b1o + lb, lane, zv);
      });
    });
  };
  auto g1_pass = [&](int k, const LayerP& P, rsrc_t rzo) {
    const rsrc_t rw = rw_of(k);
    if constexpr (MEM == 1) {
      f32x4 fa[PF], fb[PF];
      prefetch(std::true_type{}, kS1, rw, fa, fb);
      g1_body(k, P, rzo, rw, fa, fb);
    } else {
      g1_body(k, P, rzo, rw, xfa, xfb);
    }
  };

  // G2(k): A Z_k for this wave's E / L / T blocks; Z_k (all n rows) from zx.  PRO: the prologue
  // (T0 = A Z0 + E0 - X; E, L stay E0, L0)
  struct OutR { rsrc_t e, l, t, p; };
  auto g2_body = [&](auto PRO_, int k, const LayerP& P, const OutR& O, f32x4* fa, f32x4* fb) {
    // DLADMM_F_ELZ: the prologue pass runs the full epilogue (E / L half of step 0)
    const bool PRO = decltype(PRO_)::value && !elz;
    // V2 / V3: beta2, beta3, theta_e (and V3's ss2) of layer max(k, 0), beta1 of layer k + 1
    // (the prologue: layer 0; after the last layer it feeds a Var nothing reads: layer K - 1)
    const int rk = k < 0 ? 0 : k, rkn = k + 1 < K ? k + 1 : rk;
    const rsrc_t rb2 = row_view(rk, DLADMM_P_BETA2), rb3 = row_view(rk, DLADMM_P_BETA3);
    const rsrc_t rte = row_view(rk, DLADMM_P_THETA_E), rs2 = row_view(rk, DLADMM_P_SS2);
    const rsrc_t rb1n = row_view(rkn, DLADMM_P_BETA1);
    static_for<MB4 / HP>([&](auto P_) {
      constexpr int pp = decltype(P_)::value;
      f32x4 ca = zero4, cb = zero4, ca2 = zero4, cb2 = zero4;
      float rp[HP][5][4];  // the pair's row parameters, in flight across its products
      if constexpr (kRow) {
#pragma unroll
        for (int h = 0; h < HP; ++h)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int b = b2o + HP * pp + h;
            rp[h][0][r] = row_ld(rb3, b, r);
            rp[h][1][r] = row_ld(rb2, b, r);
            rp[h][2][r] = row_ld(rb1n, b, r);
            rp[h][3][r] = row_ld(rte, b, r);
            if constexpr (EMODE == EM_VVAR) rp[h][4][r] = row_ld(rs2, b, r);
          }
      }
      static_for<NB>([&](auto K_) {
        constexpr int kb = decltype(K_)::value;
        constexpr int s = pp * NB + kb;
        const f32x4 z = zx[kb * 64 + lane];
        const f32x4 wa = fa[s % PF], wb = fb[HP == 2 ? s % PF : 0];
        if constexpr (s + PF < S2) fetch(kH2, ra, std::integral_constant<int, s + PF>{}, fa, fb);
        ca = mfma4(wa.x, z[0], ca);
        if constexpr (HP == 2) cb = mfma4(wb.x, z[0], cb);
        ca2 = mfma4(wa.y, z[1], ca2);
        if constexpr (HP == 2) cb2 = mfma4(wb.y, z[1], cb2);
        ca = mfma4(wa.z, z[2], ca);
        if constexpr (HP == 2) cb = mfma4(wb.z, z[2], cb);
        ca2 = mfma4(wa.w, z[3], ca2);
        if constexpr (HP == 2) cb2 = mfma4(wb.w, z[3], cb2);
      });
      const f32x4 qa = ca + ca2, qb = cb + cb2;
      // el_step (dladmm_step.h); a per-row threshold (float): the literal shrink form
      static_for<HP>([&](auto H_) {
        constexpr int h = decltype(H_)::value;
        constexpr int lb = HP * pp + h;
        const f32x4 q = h ? qb : qa;
        f32x4 vv4;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float Pv = q[r], x = Xr[lb][r];
          const float l0 = Lr[lb][r], e0 = Er[lb][r];
          float b2 = P.b2, b3 = P.b3, b1n = P.b1n;
          if constexpr (kElem) {
            b3 = pb[lb][0][r];
            b2 = pb[lb][1][r];
            b1n = pb[lb][2][r];
          } else if constexpr (kRow) {
            b3 = rp[h][0][r];
            b2 = rp[h][1][r];
            b1n = rp[h][2][r];
          }
          const StepOut s = el_step<EMODE>(
              Pv, x, e0, l0, b2, b3, P.ss2b, PRO,
              [&] {
                if constexpr (kRow) return rp[h][4][r];
                else return P.ss2;
              },
              [&] {
                if constexpr (kRow) return rp[h][3][r];
                else return P.the;
              });
          const float e = s.e, l = s.l, t = s.t;
          Er[lb][r] = e;
          Lr[lb][r] = l;
          const uint32_t so = row_off(b2o + lb, r);
          bstore_s(O.e, vo, so, X.fin(e));
          bstore_s(O.l, vo, so, X.fin(l));
          bstore_s(O.t, vo, so, X.fin(t));
          bstore_s(O.p, vo, so, X.fin(Pv));  // training forwards: A Z_k for the backward
          const float res = x - Pv;
          fit1 += fabsf(res);                       // |X - A Z|
          fit2 = __builtin_fmaf(res, res, fit2);    // (X - A Z)^2
          vv4[r] = s.var(b1n);  // Var of the next layer
        }
        if constexpr (MEM == 1) vx[(b2o + lb) * 64 + lane] = vv4;
        else X.xstore(rxv, b2o + lb, lane, vv4);
      });
    });
  };
  auto g2_pass = [&](auto PRO_, int k, const LayerP& P, const OutR& O) {
    load_betas(k);
    if constexpr (MEM == 1) {
      f32x4 fa[PF], fb[PF];
      prefetch(kH2, kS2, ra, fa, fb);
      g2_body(PRO_, k, P, O, fa, fb);
    } else {
      g2_body(PRO_, k, P, O, xfa, xfb);
    }
  };

  constexpr auto kNB = std::integral_constant<int, NB>{};
  constexpr auto kMB = std::integral_constant<int, MB>{};
  const rsrc_t none = mkrsrc(nullptr, 0u);
  __syncthreads();  // Z0 is in zx
  {
    const rsrc_t t0 = mkrsrc(a.keep_all ? a.To : nullptr, (a.keep_all && a.To) ? mbytes : 0u);
    const OutR Op{elz ? mkrsrc(a.Eo, mbytes) : none, elz ? mkrsrc(a.Lo, mbytes) : none, t0,
                  elz ? mkrsrc(a.Po, a.Po ? mbytes : 0u) : none};
    if constexpr (MEM > 1) pre2();
    g2_pass(std::true_type{}, -1, layer_params<EMODE, PKIND>(a.scal, -1, K, elz), Op);
  }
  regsum = fit1 = fit2 = 0.f;  // the prologue's sums are not an objective
  X.handoff(rxv, vx, kMB, [&] {  // Var_0 complete
    if constexpr (MEM > 1) if (K > 0) pre1(0);
  });
  for (int k = 0; k < K; ++k) {
    const bool st = a.keep_all || k == K - 1;
    const int ko = a.keep_all ? k : 0;
    const LayerP P = layer_params<EMODE, PKIND>(a.scal, k, K, elz);
    g1_pass(k, P, mkrsrc(a.Zo + (int64_t)ko * n * a.ldo, st ? zbytes : 0u));
    X.handoff(rxz, zx, kNB, [&] {  // Z_k complete; every wave is done reading Var_k
      if constexpr (MEM > 1) pre2();
    });
    // DLADMM_F_ELZ (keep_all): the run ends with Z_{K-1}, or (tail) with a product pass that
    // stores only P[K]; the passes before it write slab k + 1 of E / L / P
    const bool zlast = elz && k == K - 1;
    if (zlast && elz == 1) break;
    const int ke = elz ? k + 1 : ko, kp = elz ? k + 1 : k;
    const bool sel = st && !zlast;
    const OutR O{mkrsrc(a.Eo + (int64_t)ke * m * a.ldo, sel ? mbytes : 0u),
                 mkrsrc(a.Lo + (int64_t)ke * m * a.ldo, sel ? mbytes : 0u),
                 mkrsrc(a.To ? a.To + (int64_t)(a.keep_all ? k + 1 : 0) * m * a.ldo : nullptr,
                        (a.To && sel) ? mbytes : 0u),
                 mkrsrc(a.Po && a.keep_all ? a.Po + (int64_t)kp * m * a.ldo : nullptr,
                        a.Po && a.keep_all ? mbytes : 0u)};
    g2_pass(std::false_type{}, k, P, O);
    if (lossz) stage_loss();
    X.handoff(rxv, vx, kMB, [&] {  // Var_{k+1} (and the layer's objective partials) complete;
                                   // every wave is done reading Z_k
      if constexpr (MEM > 1) if (k + 1 < K) pre1(k + 1);
    });
    if (lossz) flush_loss(k);
  }
}

template <int EM, int PK, bool ELZ, int MEM>
hipError_t launch_fused_rs_as(const FusedArgs& a, int grid, hipStream_t s) {
  hipLaunchKernelGGL((fused_rs_kernel<kShapeMP[2], kShapeNP[2], EM, PK, ELZ, MEM>), dim3(grid),
                     dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace dladmm
