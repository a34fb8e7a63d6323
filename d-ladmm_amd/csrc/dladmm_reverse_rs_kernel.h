// dladmm_reverse_rs_kernel.h -- the reverse-sweep backward for SMALL batches: one workgroup per 16
// batch columns, the ROWS of every product split over its 4 waves (the backward twin of
// dladmm_fused_rs_kernel.h, path 5).
//
// The reverse sweep (dladmm_reverse_kernel.h) gives each wave 16 columns and all rows, so the
// reference training loops' batches of 20 / 25 (main_lena.py:155, main_syn_l1l1_scalar.py -bs
// 25) ran the whole backward on one CU.  Here, per layer k = K-1 .. 0, wave w owns
//   G1'(k)  R = A^T gP_k      rows n: blocks 8w .. 8w+7, epilogue BK2(k) (gU_k, the adjoint of Z)
//   G2'(k)  gVar = M_k^T gU_k rows m: blocks 4w .. 4w+3, epilogue BK3(k) + BK1(k-1)
// and the B operands (gP_k, then gU_k: whole column states) go through LDS, one barrier per
// product.  The products are the reverse sweep's -- same packed A^T / M_k^T fragments, one fma
// chain per output block in k order -- and so are the elementwise expressions, in the same
// order: gU_k and Var_k (and with them every weight gradient) are that kernel's bit for bit.
// The parameter partials are per (layer, slot, wave) as there, but each wave's partial covers a
// quarter of the rows of 16 columns, so the parameter gradients agree to rounding
// (tests/test_gpu_rowsplit.py); V1's per-sample beta gradients are per-element stores, equal
// bit for bit.  ROWP (V2 / V3, per-row parameters; under DLADMM_F_ROWSPLIT_ROWP): the parameters
// are row-table operands of the epilogue rows and their gradients per-row partials, one entry
// per (layer, slot, row, 16-column group) -- the same 16 columns, hence the same row16_sum, as
// the 64-column sweep's wave of that index, reduced in the same fp64 order: the per-row
// gradients are that sweep's too (tests/test_gpu_rowsplit_rowp.py).
// Scope: V1 (EM_V1), V2 (EM_V1 + ROWP), V3 (EM_VVAR + ROWP), V4 / V5 (EM_VVAR) and V6 (EM_LASSO)
// at the 256 x 512 shape, with or without cotangents of Z and of E / L / T (the reference's
// torch-op losses over the returned states, main_lena.py:221-228).  The operands of a G2' output
// pair are loaded as the pair's products start, in flight across its 32 MFMA steps.
// Instantiated by dladmm_reverse_rs.hip (V1 / V4 / V5 / V6, and the dispatch) and
// dladmm_reverse_rs_v2.hip / _v3.hip (one translation unit each: the build stays parallel).
#pragma once
#include "dladmm_group_xchg.h"
#include "dladmm_step.h"

#ifndef RRS_PF
#define RRS_PF 4  // weight-fragment read-ahead (MFMA steps) per wave
#endif

namespace dladmm {

// MEM: workgroups per 16-column group.  1 = the one-workgroup form (bwd path 2); 4 = bwd path 3,
// after a path-6 forward: wave v = 4 member + w of the group's 16 owns G1' pair v and G2' block v
// (half of an M_k^T pair), and the B operands (gU_k, gP_k) go between the members through the
// group's exchange buffer once per product, by the forward's hand-off (dladmm_group_xchg.h: sc1
// stores, one agent-scope counter add per member, one bounded sc1 poll; NaN adjoints after a
// timeout)
template <int MP, int NP, int EMODE, bool GZ, bool COT, int MEM, bool ROWP = false>
__global__ __launch_bounds__(256, 1) void reverse_rs_kernel(const RevArgs a) {
  constexpr int MB = MP / 16, NB = NP / 16;
  constexpr int WPG = kWaves * MEM;                     // waves per 16-column group
  constexpr int NB4 = NB / WPG, MB4 = MB / WPG;         // output blocks per wave
  static_assert(NB4 % 2 == 0 && (MB4 % 2 == 0 || MB4 == 1), "G1' whole pairs; G2' pairs or one block");
  constexpr int HP = MB4 >= 2 ? 2 : 1;                  // G2' blocks per output step group
  constexpr int S1 = (NB4 / 2) * MB, S2 = (MB4 / HP) * NB;  // MFMA steps of a wave's G1' / G2'
  constexpr bool kAE = EMODE == EM_VVAR;  // the adjoint of E is carried through the workspace
  constexpr bool kV1 = EMODE == EM_V1 && !ROWP;  // V1: per-sample betas and their gradients
  static_assert(!ROWP || EMODE != EM_LASSO, "per-row parameters: V2 (EM_V1), V3 (EM_VVAR)");
  // weight-fragment read-ahead: deeper in the four-workgroup form, whose waves wait on the
  // weight stream rather than on their MFMAs (the forward's XS_PF)
  constexpr int PF = MEM > 1 ? 8 : RRS_PF;
  __shared__ f32x4 gpx[MB * 64];  // gP_k of the 16 columns (G1''s B operand)
  __shared__ f32x4 gux[NB * 64];  // gU_k (G2''s B operand)

  GroupXchg<MEM> X;
  const int grp = X.grp, mem = X.mem;
  if (MEM > 1 && grp * 16 >= a.B) return;   // a padding group: every member leaves
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int v = mem * kWaves + w;           // wave of the group
  const int g = lane >> 4;
  const int64_t col = (int64_t)grp * 16 + (lane & 15);
  const bool cv = col < a.B;
  const int m = a.m, K = a.K;
  const int cg = grp * WPG + v;  // partial slot of this wave (ROWP: per-row partials, slot grp)
  const uint32_t lqm = __builtin_amdgcn_readfirstlane(a.loss_kind) == DLADMM_LOSS_LASSO ? ~0u : 0u;
  const int64_t ldo = a.ldo, ml = (int64_t)m * ldo, zl = (int64_t)a.n * ldo;
  auto lane_off = [&](int64_t ld, bool ok) -> uint32_t {
    return ok ? (uint32_t)((col + (int64_t)(4 * g) * ld) * 4) : kOOB;
  };
  const uint32_t vo = lane_off(ldo, cv), vx = lane_off(a.ldx, cv), vw = lane_off(a.ldw, col < a.Bw);
  const uint32_t ldo4 = (uint32_t)(ldo * 4), ldw4 = (uint32_t)(a.ldw * 4);
  const uint32_t aeo = (uint32_t)(a.aer * a.ldw * 4), vas4 = (uint32_t)(a.vas * 4);
  const uint32_t mbytes = (uint32_t)(ml * 4);
  const int b1o = v * NB4, b2o = v * MB4;
  const rsrc_t none = mkrsrc(nullptr, 0u);
  // MEM = 4: the group's exchange buffer (gU blocks [NB][64] f32x4, then gP blocks [MB][64])
  const f32x4* xu = (const f32x4*)(MEM > 1 ? a.xch + (int64_t)grp * a.xstride : nullptr);
  const rsrc_t rxu = mkrsrc((const float*)xu, MEM > 1 ? (uint32_t)(NB * 64 * 16) : 0u);
  const rsrc_t rxp = mkrsrc((const float*)(xu + NB * 64), MEM > 1 ? (uint32_t)(MB * 64 * 16) : 0u);
  X.join(a.xcnt);
  // a wave-uniform (pointer, size) buffer view (readfirstlane: the selects stay in SGPRs)
  auto urs = [](const float* p, uint32_t bytes) -> rsrc_t {
    const uint64_t v = (uint64_t)p;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return mkrsrc((const float*)(((uint64_t)hi << 32) | lo), __builtin_amdgcn_readfirstlane(bytes));
  };
  typedef const float* const __attribute__((address_space(4)))* ctab_p;
  const ctab_p tab = (ctab_p)a.ptab;
  auto ld = [](rsrc_t r, uint32_t voff, uint32_t soff) -> float {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, (int)soff, 2));
  };
  auto row_off = [&](int b, int r, uint32_t ld4) -> uint32_t {  // opaque per-block base
    uint32_t o = (uint32_t)(16 * b) * ld4;
    asm volatile("" : "+s"(o));
    return o + (uint32_t)r * ld4;
  };

  // state of this wave's rows: the adjoint of Z (n rows: gU once BK2 formed it), the partial
  // adjoint of L_{k-1} (m rows), X
  float AZ[NB4][4], AL[MB4][4], Xr[MB4][4];
  {
    const rsrc_t rx = mkrsrc(a.X, (uint32_t)(m * a.ldx * 4));
#pragma unroll
    for (int b = 0; b < NB4; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) AZ[b][r] = 0.f;
#pragma unroll
    for (int b = 0; b < MB4; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        AL[b][r] = 0.f;
        Xr[b][r] = ld(rx, vx, row_off(b2o + b, r, (uint32_t)(a.ldx * 4)));
      }
  }
  float psz = 0.f, psb1 = 0.f, ps[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
  auto flush = [&](int layer, int slot, float v) {
    if constexpr (kV1 || ROWP) return;  // V1: per-sample betas (element gradients), fixed
                                        // thresholds; V2 / V3: per-row partials (pstore)
    const float s = wave_sum(v);
    if (lane == 0) a.part[((int64_t)layer * DLADMM_NSCALAR + slot) * a.ncg + cg] = X.fin(s);
  };
  auto flush_bk1 = [&](int j) {
    if constexpr (kV1 || ROWP) return;
    flush(j, DLADMM_P_BETA3, ps[0]);
    if constexpr (EMODE == EM_VVAR) {
      flush(j, DLADMM_P_BETA2, ps[1]);
      flush(j, DLADMM_P_THETA_E, ps[2]);
      flush(j, DLADMM_P_SS2, ps[3]);
    } else {
      flush(j, DLADMM_P_SS2, ps[3]);
      flush(j, DLADMM_P_SS2B, ps[4]);
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) ps[i] = 0.f;
  };

  // G2'(k) / G1'(k) scalars: load_lp2 / load_lp1 (dladmm_step.h)
  auto lp2 = [&](int k, int jl) { return load_lp2<ROWP>(a.scal, a.lcoef, a.loss_kind, k, jl, K); };
  auto lp1 = [&](int k) { return load_lp1<ROWP>(a.scal, a.lcoef, a.loss_kind, k); };

  // ROWP (the reverse sweep's row-table operands and per-row partials): the row table
  // [K][8][rstride] (lane: rows 4 g .. of a block, the 16 lanes of a row on one address; rows past
  // m / n read finite table entries -- or 0 past the table -- that meet zero adjoints) and the
  // per-row partials [K][8][RS][ncg], RS = max(MP, NP) rows, ncg = the 16-column groups: entry
  // grp of a row is the row16_sum of this group's 16 columns, written by the one wave of the group
  // that owns the row, so every entry the reduction reads (rows < m / n) is written once
  constexpr int RS = MP > NP ? MP : NP;
  const int64_t rst = ROWP ? a.rstride : 0;
  const rsrc_t rrow = ROWP ? mkrsrc(a.rowp, (uint32_t)(K * 8 * rst * 4)) : none;
  const uint32_t vr = (uint32_t)(16 * g);
  auto rbase = [&](int k, int slot) -> uint32_t {
    return __builtin_amdgcn_readfirstlane((uint32_t)(((int64_t)k * 8 + slot) * rst * 4));
  };
  const int64_t pslot = (int64_t)RS * a.ncg;   // floats per (layer, slot) of the partials
  auto rpart = [&](int k) -> rsrc_t {
    return urs(ROWP ? a.rpart + (int64_t)k * 8 * pslot : nullptr, ROWP ? (uint32_t)(8 * pslot * 4) : 0u);
  };
  const uint32_t vpr = (lane & 15) == 0 ? (uint32_t)(((int64_t)(4 * g) * a.ncg + grp) * 4) : kOOB;
  const uint32_t ldp4 = (uint32_t)(a.ncg * 4);
  // per-row partial of (slot, row 16 b + 4 g + r): the group's 16 columns summed, stored by lanes
  // l & 15 == 0; NaN after a timed-out hand-off, as every value formed from exchanged operands
  auto pstore = [&](rsrc_t rp, int slot, int b, int r, float v) {
    const uint32_t so = __builtin_amdgcn_readfirstlane((uint32_t)(slot * pslot * 4));
    bstore_s(rp, vpr, so + row_off(b, r, ldp4), X.fin(row16_sum(v)));
  };

  const uint32_t vf = (uint32_t)(lane * 16);
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  auto frag2 = [&](rsrc_t r, auto S_, f32x4& fa, f32x4& fb) {
    constexpr int s = decltype(S_)::value;
    fa = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)vf, 2 * s * 1024, 0));
    fb = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)vf, (2 * s + 1) * 1024, 0));
  };
  const int64_t wl = (int64_t)MB * NB * kFrag;  // floats per packed matrix
  // A^T [NB/2][MB][2] (G1': this wave's pairs from b1o / 2 on); M_k^T [K][MB/2][NB][2]
  const rsrc_t rat = mkrsrc(a.Atp + (int64_t)(b1o / 2) * MB * 2 * kFrag, (uint32_t)(S1 * 2 * kFrag * 4));

  // G1'(k): R = A^T gP_k for this wave's n blocks; BK2(k): gU_k = S'(U_k) (gZ + cz sgn Z_k + R)
  auto g1_pass = [&](int k) {
    const LP1 P1 = lp1(k);
    const rsrc_t rz = urs(a.Z + k * zl, (uint32_t)(zl * 4));
    const float* gzp = GZ ? tab[rev_tab_at(RT_GZ, K, k)] : nullptr;
    const rsrc_t rgz = GZ ? urs(gzp, gzp ? (uint32_t)(zl * 4) : 0u) : none;
    const rsrc_t rg = urs(a.GU + k * a.gus, (uint32_t)(NP * a.ldw * 4));
    float pz[NB4][4], pg[GZ ? NB4 : 1][4];
    float pt[ROWP ? NB4 : 1][4];  // ROWP: theta_z of this wave's rows
    const uint32_t rthz = ROWP ? rbase(k, DLADMM_P_THETA_Z) : 0u;
    const rsrc_t rpk1 = rpart(k);
#pragma unroll
    for (int b = 0; b < NB4; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint32_t so = row_off(b1o + b, r, ldo4);
        pz[b][r] = ld(rz, vo, so);
        if constexpr (GZ) pg[b][r] = ld(rgz, vo, so);
        if constexpr (ROWP) pt[b][r] = ld(rrow, vr, rthz + row_off(b1o + b, r, 4u));
      }
    f32x4 fa[PF], fb[PF];
    static_for<PF>([&](auto I_) {
      constexpr int i = decltype(I_)::value;
      if constexpr (i < S1) frag2(rat, I_, fa[i], fb[i]);
    });
    static_for<NB4 / 2>([&](auto P_) {
      constexpr int pp = decltype(P_)::value;
      f32x4 ca = zero4, cb = zero4;
      static_for<MB>([&](auto J_) {
        constexpr int jb = decltype(J_)::value;
        constexpr int s = pp * MB + jb;
        const f32x4 v = gpx[jb * 64 + lane];
        const f32x4 wa = fa[s % PF], wb = fb[s % PF];
        if constexpr (s + PF < S1)
          frag2(rat, std::integral_constant<int, s + PF>{}, fa[s % PF], fb[s % PF]);
        ca = mfma4(wa.x, v[0], ca);
        cb = mfma4(wb.x, v[0], cb);
        ca = mfma4(wa.y, v[1], ca);
        cb = mfma4(wb.y, v[1], cb);
        ca = mfma4(wa.z, v[2], ca);
        cb = mfma4(wb.z, v[2], cb);
        ca = mfma4(wa.w, v[3], ca);
        cb = mfma4(wb.w, v[3], cb);
      });
      static_for<2>([&](auto H_) {
        constexpr int h = decltype(H_)::value;
        constexpr int lb = 2 * pp + h;
        const f32x4 q = h ? cb : ca;
        f32x4 gu4;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float zk = pz[lb][r];
          // BK2 (z_adjoint, dladmm_step.h); theta_z's mask bound is per row under ROWP
          const float cth = ROWP ? z_mask_bound(pt[ROWP ? lb : 0][r]) : P1.c;
          const ZAdj za = z_adjoint(
              (GZ ? AZ[lb][r] + pg[GZ ? lb : 0][r] : AZ[lb][r]) + q[r], zk, cth, P1.cz);
          const float gU = za.gU;
          if constexpr (ROWP) pstore(rpk1, DLADMM_P_THETA_Z, b1o + lb, r, za.pth);
          else psz += za.pth;
          AZ[lb][r] = gU;
          gu4[r] = X.fin(gU);
          bstore_s(rg, vw, row_off(b1o + lb, r, ldw4), gu4[r]);
        }
        gux[(b1o + lb) * 64 + lane] = gu4;
        X.xstore(rxu, b1o + lb, lane, gu4);
      });
    });
    flush(k, DLADMM_P_THETA_Z, psz);
    psz = 0.f;
  };

  // G2'(k): gVar = M_k^T gU_k for this wave's m blocks.  MODE 0: BK3(k) + BK1(k-1) on layer
  // j = k - 1's saved state; 1: BK3 of layer 0 alone (T_0 in the P slot, L0); 2: the prologue,
  // BK1(K-1) with zero incoming adjoints (no product)
  auto g2_pass = [&](auto MODE_, int k) {
    constexpr int MODE = decltype(MODE_)::value;
    const int j = MODE == 2 ? K - 1 : k - 1;   // the BK1 layer
    const LP2 P = MODE == 2 ? lp2(K, K - 1) : (MODE == 1 ? lp2(0, -1) : lp2(k, k - 1));
    // operand views (the reverse sweep's res2 / res2_last)
    auto tview = [&](int t, int kk) -> rsrc_t {
      const float* p = tab[rev_tab_at(t, K, kk)];
      return urs(p, p ? mbytes : 0u);
    };
    rsrc_t oP, oL, oE = none;
    rsrc_t oB1K = none, oGB1K = none, oB1J = none, oB2J = none, oGB1J = none, oGB2J = none;
    rsrc_t oGE = none, oGL = none, oGT = none;
    if constexpr (MODE == 1) {
      oP = mkrsrc(a.T, mbytes);
      oL = urs(a.L0, mbytes);
      if constexpr (kV1) {
        oB1K = tview(RT_B1, 0);
        oGB1K = tview(RT_GB1, 0);
      }
    } else {
      oP = urs(a.P + j * ml, mbytes);
      oL = urs(j >= 1 ? a.L + (j - 1) * ml : a.L0, mbytes);
      if constexpr (kAE) oE = urs(j >= 1 ? a.E + (j - 1) * ml : a.E0, mbytes);
      if constexpr (kV1) {
        const bool bk3 = j + 1 < K;   // the prologue (j = K - 1) has no BK3
        oB1K = bk3 ? tview(RT_B1, j + 1) : none;
        oGB1K = bk3 ? tview(RT_GB1, j + 1) : none;
        oB1J = tview(RT_B1, j);
        oB2J = tview(RT_B2, j);
        oGB1J = tview(RT_GB1, j);
        oGB2J = tview(RT_GB2, j);
      }
      if constexpr (COT) {
        oGE = tview(RT_GE, j);
        oGL = tview(RT_GL, j);
        oGT = tview(RT_GT, j + 1);
      }
    }
    // ROWP: row-table offsets (the reverse sweep's res2 / res2_last) and the per-row partials of
    // BK3's layer (beta1) and BK1's layer j
    uint32_t rb1k = 0u, rb1j = 0u, rb2j = 0u, rthe = 0u, rb3j = 0u, rss2 = 0u;
    rsrc_t pPK = none, pPJ = none;
    if constexpr (ROWP) {
      if constexpr (MODE == 1) {
        pPK = rpart(0);
        rb1k = rbase(0, DLADMM_P_BETA1);
      } else {
        const bool bk3 = j + 1 < K;
        if constexpr (MODE == 0) pPK = rpart(j + 1);
        pPJ = rpart(j);
        rb1k = rbase(bk3 ? j + 1 : j, DLADMM_P_BETA1);
        rb1j = rbase(j, DLADMM_P_BETA1);
        rb2j = rbase(j, DLADMM_P_BETA2);
        rthe = rbase(j, DLADMM_P_THETA_E);
        rb3j = rbase(j, DLADMM_P_BETA3);
        rss2 = rbase(j, DLADMM_P_SS2);
      }
    }
    // Var_j's workspace block and the next layer's (which holds the adjoint of E_{j})
    const int jr = MODE == 1 ? 0 : j;
    const rsrc_t rv = urs(a.VAR + jr * a.vas, (uint32_t)((jr + 1 < K ? 2 : 1) * a.vas * 4));
    // operands of one pair of m blocks, loaded as the pair's products start (in flight during
    // its 32 MFMA steps)
    enum { O_P = 0, O_L = 1, O_E = 2, O_A = 3, O_B1K = 4, O_B1J = 5, O_B2J = 6, O_GB1 = 7,
           O_GE = 8, O_GL = 9, O_GT = 10,
           O_RB1K = 11, O_RB1J = 12, O_RB2J = 13, O_RTHE = 14, O_RB3J = 15, O_RSS2 = 16 };
    float op[2][17][4];
    auto load_pair = [&](int pp) {
#pragma unroll
      for (int h = 0; h < HP; ++h)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int b = HP * pp + h;
          const uint32_t so = row_off(b2o + b, r, ldo4);
          op[h][O_P][r] = ld(oP, vo, so);
          op[h][O_L][r] = ld(oL, vo, so);
          if constexpr (kAE) {
            op[h][O_E][r] = MODE == 1 ? 0.f : ld(oE, vo, so);
            op[h][O_A][r] = MODE == 0 ? ld(rv, vw, vas4 + aeo + row_off(b2o + b, r, ldw4)) : 0.f;
          }
          if constexpr (kV1) {
            op[h][O_B1K][r] = ld(oB1K, vo, so);
            op[h][O_B1J][r] = ld(oB1J, vo, so);
            op[h][O_B2J][r] = ld(oB2J, vo, so);
            op[h][O_GB1][r] = ld(oGB1K, vo, so);
          }
          if constexpr (COT) {
            op[h][O_GE][r] = ld(oGE, vo, so);
            op[h][O_GL][r] = ld(oGL, vo, so);
            op[h][O_GT][r] = ld(oGT, vo, so);
          }
          if constexpr (ROWP) {
            const uint32_t rs = row_off(b2o + b, r, 4u);
            op[h][O_RB1K][r] = ld(rrow, vr, rb1k + rs);
            if constexpr (MODE != 1) {
              op[h][O_RB1J][r] = ld(rrow, vr, rb1j + rs);
              op[h][O_RB2J][r] = ld(rrow, vr, rb2j + rs);
              op[h][O_RTHE][r] = ld(rrow, vr, rthe + rs);
              if constexpr (kAE) {
                op[h][O_RB3J][r] = ld(rrow, vr, rb3j + rs);
                op[h][O_RSS2][r] = ld(rrow, vr, rss2 + rs);
              }
            }
          }
        }
    };
    // M_k^T: HP = 2, this wave's pairs from b2o / 2 on (steps read fragments 2s, 2s + 1);
    // HP = 1, half b2o & 1 of pair b2o / 2 (fragments 2 (P NB + kb) + h0: step s at 2s)
    const rsrc_t rmt =
        MODE == 2 ? none
        : HP == 2 ? mkrsrc(a.Mtp + (int64_t)k * wl + (int64_t)(b2o / 2) * NB * 2 * kFrag,
                           (uint32_t)(S2 * 2 * kFrag * 4))
                  : mkrsrc(a.Mtp + (int64_t)k * wl + ((int64_t)(b2o >> 1) * NB * 2 + (b2o & 1)) * kFrag,
                           (uint32_t)((2 * S2 - 1) * kFrag * 4));
    f32x4 fa[PF], fb[HP == 2 ? PF : 1];
    auto fetch = [&](auto S_, int slot) {
      constexpr int st = decltype(S_)::value;
      if constexpr (HP == 2) {
        frag2(rmt, S_, fa[slot], fb[slot]);
      } else {
        fa[slot] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                                 rmt, (int)vf, 2 * st * 1024, 0));
      }
    };
    if constexpr (MODE != 2) {
      static_for<PF>([&](auto I_) {
        constexpr int i = decltype(I_)::value;
        if constexpr (i < S2) fetch(I_, i);
      });
    }
    static_for<MB4 / HP>([&](auto P_) {
      constexpr int pp = decltype(P_)::value;
      load_pair(pp);
      f32x4 qa4[2] = {zero4, zero4};
      if constexpr (MODE != 2) {
        f32x4 ca = zero4, cb = zero4;
        static_for<NB>([&](auto K_) {
          constexpr int kb = decltype(K_)::value;
          constexpr int s = pp * NB + kb;
          const f32x4 u = gux[kb * 64 + lane];
          const f32x4 wa = fa[s % PF];
          const f32x4 wb = fb[HP == 2 ? s % PF : 0];
          if constexpr (s + PF < S2)
            fetch(std::integral_constant<int, s + PF>{}, s % PF);
          ca = mfma4(wa.x, u[0], ca);
          if constexpr (HP == 2) cb = mfma4(wb.x, u[0], cb);
          ca = mfma4(wa.y, u[1], ca);
          if constexpr (HP == 2) cb = mfma4(wb.y, u[1], cb);
          ca = mfma4(wa.z, u[2], ca);
          if constexpr (HP == 2) cb = mfma4(wb.z, u[2], cb);
          ca = mfma4(wa.w, u[3], ca);
          if constexpr (HP == 2) cb = mfma4(wb.w, u[3], cb);
        });
        qa4[0] = ca;
        qa4[1] = cb;
      }
      // epilogue rows: BK3 / BK1 as in the 64-column sweep (el_adjoint, dladmm_step.h)
#pragma unroll
    for (int h = 0; h < HP; ++h) {
      const int lb = HP * pp + h;
      f32x4 gp4;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float gVar = qa4[h][r];
        const uint32_t sw = row_off(b2o + lb, r, ldw4);
        const uint32_t sb = row_off(b2o + lb, r, ldo4);
        const float b1k = kV1 ? op[h][O_B1K][r] : ROWP ? op[h][O_RB1K][r] : P.b1k;
        if constexpr (MODE == 1) {
          if constexpr (kV1) {
            // beta1_0's gradient: BK1(0)'s term + gVar T_0
            bstore_s(oGB1K, vo, sb, op[h][O_GB1][r] + gVar * op[h][O_P][r]);
          } else if constexpr (ROWP) {
            // beta1_0's per-row partial: gVar T_0
            pstore(pPK, DLADMM_P_BETA1, b2o + lb, r, gVar * op[h][O_P][r]);
          } else {
            psb1 += gVar * op[h][O_P][r];   // beta1_0's gradient: gVar T_0
          }
          // Var_0 = L0 + beta1_0 T_0, the forward's prologue expression
          bstore_s(rv, vw, sw, op[h][O_L][r] + b1k * op[h][O_P][r]);
          continue;
        }
        const float aLin = AL[lb][r] + gVar;  // complete adjoint of L_{k-1} (upstream aside)
        const float aTin = b1k * gVar;        // adjoint of T_k
        const float aL = COT ? aLin + op[h][O_GL][r] : aLin;
        const float aT = COT ? aTin + op[h][O_GT][r] : aTin;
        const float aE0 = MODE == 0 ? (kAE ? op[h][O_A][r] : 0.f) : 0.f;
        const float aE = COT ? aE0 + op[h][O_GE][r] : aE0;
        const float Pv = op[h][O_P][r], lp = op[h][O_L][r], x = Xr[lb][r];
        const float b1 = kV1 ? op[h][O_B1J][r] : ROWP ? op[h][O_RB1J][r] : 0.f;
        // per-row parameters of BK1's layer (ROWP), else the layer's scalars
        const float b2p = ROWP ? op[h][O_RB2J][r] : P.b2;
        const float b3p = (ROWP && kAE) ? op[h][O_RB3J][r] : P.b3;
        const float ss2p = (ROWP && kAE) ? op[h][O_RSS2][r] : P.ss2;
        const float thep = ROWP ? op[h][O_RTHE][r] : P.the;
        // BK1 of layer j (el_adjoint, dladmm_step.h); V1's beta2 is per sample
        const float b2 = (EMODE == EM_V1 && !ROWP) ? op[h][O_B2J][r] : b2p;
        const float ep = kAE ? op[h][O_E][r] : 0.f;
        const ElAdj ad = el_adjoint<EMODE, ROWP>(aL, aT, aE, Pv, lp, ep, x, b1, b2, b3p, ss2p,
                                                 P.ss2b, thep, P.cf, lqm);
        const float gP = ad.gP, gEp = ad.gEp, gLp = ad.gLp, t = ad.t;
        const float p3 = ad.p3, p2 = ad.p2, pe = ad.pe, ps2 = ad.ps2, ps2b = ad.ps2b;
        (void)gEp;
        if constexpr (kV1) {
          // beta1_k's gradient = BK1(k)'s term + gVar T_k; beta1_{k-1} gets BK1(k-1)'s term
          // aL T_k now and BK3(k-1)'s next pass; beta2_{k-1} complete
          bstore_s(MODE == 0 ? oGB1K : none, vo, sb, op[h][O_GB1][r] + gVar * t);
          bstore_s(oGB1J, vo, sb, p3);
          bstore_s(oGB2J, vo, sb, p2);
        } else if constexpr (ROWP) {
          // per-row partials: beta1 of layer k (BK3), then BK1(k-1)'s slots, as the reverse sweep
          // groups them (BK1's beta3 slot carries V2's beta1 L term)
          if constexpr (MODE == 0) pstore(pPK, DLADMM_P_BETA1, b2o + lb, r, gVar * t);
          pstore(pPJ, DLADMM_P_BETA3, b2o + lb, r, p3);
          pstore(pPJ, DLADMM_P_BETA2, b2o + lb, r, p2);
          pstore(pPJ, DLADMM_P_THETA_E, b2o + lb, r, pe);
          if constexpr (kAE) pstore(pPJ, DLADMM_P_SS2, b2o + lb, r, ps2);
        } else {
          if constexpr (MODE == 0) psb1 += gVar * t;  // beta1 of layer k: gVar * T_k
          ps[0] += p3; ps[1] += p2; ps[2] += pe; ps[3] += ps2; ps[4] += ps2b;
        }
        gp4[r] = X.fin(gP);
        AL[lb][r] = gLp;
        // Var of layer k: L_{k-1} + beta1_k T_k from the recomputed values (the prologue's,
        // layer K, runs past the workspace: dropped)
        const float vark = var_k<EMODE>(lp, t, b1, b3p, b1k);
        bstore_s(rv, vw, vas4 + sw, vark);
        if constexpr (kAE) bstore_s(rv, vw, sw + aeo, gEp);  // adjoint of E_{k-2}
      }
      if constexpr (MODE != 1) {
        gpx[(b2o + lb) * 64 + lane] = gp4;
        X.xstore(rxp, b2o + lb, lane, gp4);
      }
    }
    });
  };

  // prologue BK1(K-1), then per layer G1'(k), G2'(k)
  constexpr auto kNB = std::integral_constant<int, NB>{};
  constexpr auto kMB = std::integral_constant<int, MB>{};
  g2_pass(std::integral_constant<int, 2>{}, K);
  flush_bk1(K - 1);
  X.handoff(rxp, gpx, kMB);  // gP_{K-1} complete
  for (int k = K - 1; k >= 1; --k) {
    g1_pass(k);
    X.handoff(rxu, gux, kNB);  // gU_k complete; every wave is done reading gP_k
    g2_pass(std::integral_constant<int, 0>{}, k);
    flush(k, DLADMM_P_BETA1, psb1);
    psb1 = 0.f;
    flush_bk1(k - 1);
    X.handoff(rxp, gpx, kMB);  // gP_{k-1} complete; every wave is done reading gU_k
  }
  g1_pass(0);
  X.handoff(rxu, gux, kNB);
  g2_pass(std::integral_constant<int, 1>{}, 0);
  flush(0, DLADMM_P_BETA1, psb1);
}

template <int EM, bool GZ, bool COT, int MEM, bool ROWP>
hipError_t launch_rrs(const RevArgs& a, int grid, hipStream_t s) {
  hipLaunchKernelGGL((reverse_rs_kernel<kShapeMP[2], kShapeNP[2], EM, GZ, COT, MEM, ROWP>),
                     dim3(grid), dim3(256), 0, s, a);
  return hipGetLastError();
}
template <int EM, int MEM = 1, bool ROWP = false>
hipError_t launch_rrs_em(const RevArgs& a, int grid, hipStream_t s) {
  if (a.has_gz && a.has_cot) return launch_rrs<EM, true, true, MEM, ROWP>(a, grid, s);
  if (a.has_gz) return launch_rrs<EM, true, false, MEM, ROWP>(a, grid, s);
  if (a.has_cot) return launch_rrs<EM, false, true, MEM, ROWP>(a, grid, s);
  return launch_rrs<EM, false, false, MEM, ROWP>(a, grid, s);
}

// V2 / V3 (ROWP), instantiated in dladmm_reverse_rs_v2.hip / _v3.hip; mem: workgroups per
// 16-column group (1: bwd path 2, 4: bwd path 3)
hipError_t launch_rrs_v2(const RevArgs& a, int grid, int mem, hipStream_t s);
hipError_t launch_rrs_v3(const RevArgs& a, int grid, int mem, hipStream_t s);

}  // namespace dladmm
