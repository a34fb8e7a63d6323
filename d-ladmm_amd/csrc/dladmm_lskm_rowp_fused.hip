// dladmm_lskm_rowp_fused.hip -- the learned + safeguarded KM forward of the per-row models (V2:
// test_syn_l1l1_ltheta.py:160-244 and test_syn_gt_ltheta.py:127-212; V3: test_syn_l1l1_full.py:
// 172-292) as ONE launch at the 256 x 512 register shape, fp32.
//
// Geometry, LDS images, weight streams, the KM candidate formed in place, the fixed-order fp64
// norm with its E term and the stores are those of dladmm_lskm_fused.hip (read its header first):
// 256 threads keep 16 columns for every layer, wave w owns G1 output blocks 8w .. 8w + 7 and G2
// blocks 4w .. 4w + 3 in the C/D map of v_mfma_f32_16x16x4_f32, weight fragments come straight
// from L2 RS_PF steps ahead (pack order 2), B operands from LDS, one sched_barrier(0) per MFMA
// step.  What differs is where the learned step's parameters come from: every one of them is PER
// ROW -- beta1, beta2, beta3 (V2: beta1 again), V3's ss2 and theta_e over the m rows, theta_z over
// the n rows, [K][8][rstride] as dladmm_fwd_desc lays them out.
//
// A lane owns 16 E / L rows and 32 Z rows: 5 x 16 + 32 = 112 values of a V3 layer, far more than
// the body (three column states per lane) leaves registers for.  So a layer's table lives in LDS,
// 5 MP + NP floats (7 KiB), and the epilogues read it from there:
//   * the workgroup loads it cooperatively, thread t rows t (the five m-row slots) and t, t + 256
//     (theta_z): 7 dword buffer loads (V2: 6) from views bounded to m / n rows, so a padded row
//     reads 0 whatever the table's row stride (its state is all zero and stays so); after the
//     last layer the last layer's table is loaded again, unread;
//   * layer k + 1's loads are issued right after pass 2's closing barrier, ahead of pass 3's
//     fragment prefetch, and committed to LDS after pass 3's last epilogue: vmcnt retires in
//     order and every fragment load of pass 3 is younger, so the wait is free.  Passes 3 and 4
//     (the KM streams) read no per-row parameter, and pass 3's closing barrier publishes the
//     table -- two barriers before its first reader, the Var formation at the top of layer k + 1.
//     One buffer is enough: layer k's last reader (pass 2's epilogue) is behind pass 2's barrier;
//   * readers take a block's four rows 16 b + 4 g .. + 3 of a slot as one 16-byte LDS load (the
//     16 lanes of a lane group on one address: a broadcast), at the top of the block's epilogue.
//
// Layer k:
//   1. G1, W_k on v0 = Lc + beta1_k o Tc                   -> Zl (theta_z_k per row)    -> z0
//   2. G2, A on z0                                         -> El, Ll, Tl (el_step<EMODE>)
//        v1 = Ll + b Tl, v0 = Lc + b Tc (b = the KM beta);  issue layer k + 1's table
//   3. dual G1, the shared -A^T on v0 and v1               -> Zk (in place) -> z0, Zs -> z1
//        commit the table
//   4. dual G2, A on z0 and z1                             -> (Ek, Lk, Tk) in place; (Es, Ts)
//   then |[beta Ts ; c (Es - 2 El + Ep)]| per column, keep = |S| < (1 - delta) mu, the mu update,
//   the lane-local select, the non-temporal stores of the selected Z / E / L / T and one integer
//   atomic per workgroup.
//
// Every stored value goes through dladmm_step.h in the fused kernel's PK_ROW forms (Z: the clamp
// form shrink_u on shrink_params(theta_z[row]); E: the literal shrink on theta_e[row]) and the
// same fma chains as the multi-launch path (a one-layer V2 / V3 forward, two one-step V5
// forwards, safeguard_kernel), so the two agree bit for bit while the decisions agree
// (tests/test_gpu_rowp_lskm.py).
#include "dladmm_lskm_rowp_fused.h"

#include "dladmm_fused_rs_kernel.h"  // RS_PF; dladmm_step.h

namespace dladmm {

template <int MP, int NP, int EMODE>
__global__ __launch_bounds__(256, 1) void lskm_rowp_fused_kernel(const LskmRowpArgs a) {
  constexpr int MB = MP / 16, NB = NP / 16;
  constexpr int NB4 = NB / kWaves, MB4 = MB / kWaves;   // output blocks per wave
  static_assert(NB4 % 2 == 0 && MB4 % 2 == 0, "whole output pairs");
  static_assert(MP == 256 && NP == 2 * MP, "the table load: thread t, rows t and t + 256");
  constexpr int S1 = (NB4 / 2) * MB, S2 = (MB4 / 2) * NB;  // MFMA steps of a wave's G1 / G2
  constexpr int PF = RS_PF;
  constexpr bool kV3 = EMODE == EM_VVAR;
  // the layer's row table: slots beta1, beta2, beta3, ss2, theta_e (MP rows each), then theta_z
  enum { T_B1 = 0, T_B2 = 1, T_B3 = 2, T_SS2 = 3, T_THE = 4, T_THZ = 5 };
  __shared__ f32x4 zx[2][NB * 64];  // Z images of the 16 columns, block b at [b * 64 + lane]
  __shared__ f32x4 vx[2][MB * 64];  // Var images
  __shared__ f32x4 tab[(5 * MP + NP) / 4];
  __shared__ double red[2][kWaves][16];  // per-wave column partials: |S|^2, and mu_0's at k = 0

  const int grp = blockIdx.x;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4;
  const int64_t col = (int64_t)grp * 16 + (lane & 15);
  const bool cv = col < a.B;
  const int m = a.m, n = a.n, K = a.K;
  auto lane_off = [&](int64_t ld) -> uint32_t {
    return cv ? (uint32_t)((col + (int64_t)(4 * g) * ld) * 4) : kOOB;
  };
  const int b1o = w * NB4, b2o = w * MB4;  // first output block of this wave in G1 / G2

  // The table of layer k, this thread's rows: issue (registers), then commit (LDS).  Views
  // bounded to the slot's rows; after the last layer: layer K - 1 again (in range, unread).
  float tr[7];
  const uint32_t vt = threadIdx.x * 4u;
  auto tab_issue = [&](int k) {
    const float* lp = a.rowp + (int64_t)(k < K ? k : K - 1) * DLADMM_NSCALAR * a.rstride;
    auto ld = [&](int slot, int lim, uint32_t off) -> float {
      const rsrc_t r = mkrsrc(lp + slot * a.rstride, (uint32_t)(lim * 4));
      return __builtin_bit_cast(float,
                                __builtin_amdgcn_raw_buffer_load_b32(r, (int)vt, (int)off, 0));
    };
    tr[T_B1] = ld(DLADMM_P_BETA1, m, 0u);
    tr[T_B2] = ld(DLADMM_P_BETA2, m, 0u);
    tr[T_B3] = ld(DLADMM_P_BETA3, m, 0u);
    if constexpr (kV3) tr[T_SS2] = ld(DLADMM_P_SS2, m, 0u);
    tr[T_THE] = ld(DLADMM_P_THETA_E, m, 0u);
    tr[5] = ld(DLADMM_P_THETA_Z, n, 0u);
    tr[6] = ld(DLADMM_P_THETA_Z, n, (uint32_t)(MP * 4));
  };
  auto tab_commit = [&]() {
    float* t = (float*)tab;
    t[T_B1 * MP + threadIdx.x] = tr[T_B1];
    t[T_B2 * MP + threadIdx.x] = tr[T_B2];
    t[T_B3 * MP + threadIdx.x] = tr[T_B3];
    if constexpr (kV3) t[T_SS2 * MP + threadIdx.x] = tr[T_SS2];
    t[T_THE * MP + threadIdx.x] = tr[T_THE];
    t[T_THZ * MP + threadIdx.x] = tr[5];
    t[T_THZ * MP + MP + threadIdx.x] = tr[6];
  };
  // rows 16 b + 4 g .. + 3 of a slot (b: the block's index in the product's output)
  auto tab_rows = [&](int slot, int b) -> f32x4 { return tab[slot * (MP / 4) + 4 * b + g]; };
  tab_issue(0);

  float Zc[NB4][4], Ec[MB4][4], Lc[MB4][4], Tc[MB4][4], Xr[MB4][4];  // current state, X
  float Zl[NB4][4], El[MB4][4], Ll[MB4][4], Tl[MB4][4];              // L2O candidate
  {
    const rsrc_t rz = mkrsrc(a.Z0, (uint32_t)(n * a.ldz0 * 4));
    const rsrc_t re = mkrsrc(a.E0, (uint32_t)(m * a.lde0 * 4));
    const rsrc_t rl = mkrsrc(a.L0, (uint32_t)(m * a.ldl0 * 4));
    const rsrc_t rx = mkrsrc(a.X, (uint32_t)(m * a.ldx * 4));
    const uint32_t oz = lane_off(a.ldz0), oe = lane_off(a.lde0), ol = lane_off(a.ldl0),
                   ox = lane_off(a.ldx);
#pragma unroll
    for (int b = 0; b < NB4; ++b) {
      f32x4 zv;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        Zc[b][r] = bload(rz, oz + (uint32_t)((16 * (b1o + b) + r) * a.ldz0 * 4));
        zv[r] = Zc[b][r];
        pin_agpr(Zc[b][r]);
      }
      zx[0][(b1o + b) * 64 + lane] = zv;
    }
#pragma unroll
    for (int b = 0; b < MB4; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint32_t ro = (uint32_t)(16 * (b2o + b) + r);
        Xr[b][r] = bload(rx, ox + ro * (uint32_t)(a.ldx * 4));
        Ec[b][r] = bload(re, oe + ro * (uint32_t)(a.lde0 * 4));
        Lc[b][r] = bload(rl, ol + ro * (uint32_t)(a.ldl0 * 4));
      }
  }
  tab_commit();  // layer 0's table, published by the barrier below

  const uint32_t vo = lane_off(a.ldo);
  const uint32_t ld4 = (uint32_t)(a.ldo * 4);
  const uint32_t zbytes = (uint32_t)(n * a.ldo * 4), mbytes = (uint32_t)(m * a.ldo * 4);
  const int64_t wl = (int64_t)MB * NB * kFrag;  // floats per packed weight
  const uint32_t vf = (uint32_t)(lane * 16);    // lane offset inside a 1-KiB fragment
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  auto frag = [&](rsrc_t r, int off) -> f32x4 {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)vf, off, 0));
  };
  // byte offset of row 16 b + r of a [rows][ldo] output (opaque base: formed where it is used)
  auto row_off = [&](int b, int r) -> uint32_t {
    uint32_t o = (uint32_t)(16 * b) * ld4;
    asm volatile("" : "+s"(o));
    return o + (uint32_t)r * ld4;
  };

  // The weight-fragment window of a pass, as in fused_rs_kernel: step s reads slot s % PF and
  // refills it with step s + PF; a wave's output pairs are one contiguous run of pack order 2, so
  // its view starts at its first pair and step s reads fragments 2s, 2s + 1.
  auto fetch = [&](rsrc_t r, auto S_, f32x4* fa, f32x4* fb) {
    constexpr int s = decltype(S_)::value;
    fa[s % PF] = frag(r, 2 * s * 1024);
    fb[s % PF] = frag(r, (2 * s + 1) * 1024);
  };
  auto prefetch = [&](auto NS_, rsrc_t r, f32x4* fa, f32x4* fb) {
    static_for<PF>([&](auto I_) {
      if constexpr (decltype(I_)::value < decltype(NS_)::value) fetch(r, I_, fa, fb);
    });
  };
  auto g1_view = [&](const float* wp) -> rsrc_t {
    return mkrsrc(wp + (int64_t)(b1o / 2) * MB * 2 * kFrag, (uint32_t)(S1 * 2 * kFrag * 4));
  };
  const rsrc_t ra = mkrsrc(a.Ap + (int64_t)(b2o / 2) * NB * 2 * kFrag,
                           (uint32_t)(S2 * 2 * kFrag * 4));
  const rsrc_t rat = g1_view(a.Atp);

  // G1: this wave's n-row blocks of (packed weight) x Var, Var (all m rows) from v0 -- and, DUAL,
  // the same fragments on v1 too.  epi(block, q0, q1) per output block.
  auto g1 = [&](auto DUAL_, rsrc_t rw, auto&& epi) {
    constexpr bool DUAL = decltype(DUAL_)::value;
    f32x4 fa[PF], fb[PF];
    prefetch(std::integral_constant<int, S1>{}, rw, fa, fb);
    // the B operand of step s + 1 is read from LDS ahead of step s's MFMAs (the wrap-around read
    // after the last step is of the same image: in range, unused)
    f32x4 nv0 = vx[0][lane], nv1 = zero4;
    if constexpr (DUAL) nv1 = vx[1][lane];
    static_for<NB4 / 2>([&](auto P_) {
      constexpr int pp = decltype(P_)::value;
      f32x4 ca = zero4, cb = zero4, da = zero4, db = zero4;
      static_for<MB>([&](auto J_) {
        constexpr int jb = decltype(J_)::value;
        constexpr int s = pp * MB + jb;
        const f32x4 v0 = nv0, v1 = nv1;
        nv0 = vx[0][((jb + 1) % MB) * 64 + lane];
        if constexpr (DUAL) nv1 = vx[1][((jb + 1) % MB) * 64 + lane];
        const f32x4 wa = fa[s % PF], wb = fb[s % PF];
        if constexpr (s + PF < S1) fetch(rw, std::integral_constant<int, s + PF>{}, fa, fb);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          ca = mfma4(wa[q], v0[q], ca);
          cb = mfma4(wb[q], v0[q], cb);
          if constexpr (DUAL) {
            da = mfma4(wa[q], v1[q], da);
            db = mfma4(wb[q], v1[q], db);
          }
        }
        // keep the step's refill with the step: under this kernel's register pressure the
        // scheduler otherwise sinks every fragment load to its use (a read-ahead of one)
        __builtin_amdgcn_sched_barrier(0);
      });
      epi(std::integral_constant<int, 2 * pp>{}, ca, da);
      epi(std::integral_constant<int, 2 * pp + 1>{}, cb, db);
    });
  };
  // G2: this wave's m-row blocks of A x Z, Z (all n rows) from z0 -- and, DUAL, from z1 too.
  // Two chains per block (k sub-steps x, z and y, w) summed once.
  auto g2 = [&](auto DUAL_, auto&& epi) {
    constexpr bool DUAL = decltype(DUAL_)::value;
    f32x4 fa[PF], fb[PF];
    prefetch(std::integral_constant<int, S2>{}, ra, fa, fb);
    f32x4 nz = zx[0][lane], ny = zero4;  // read ahead as in g1
    if constexpr (DUAL) ny = zx[1][lane];
    static_for<MB4 / 2>([&](auto P_) {
      constexpr int pp = decltype(P_)::value;
      f32x4 ca = zero4, cb = zero4, ca2 = zero4, cb2 = zero4;
      f32x4 da = zero4, db = zero4, da2 = zero4, db2 = zero4;
      static_for<NB>([&](auto K_) {
        constexpr int kb = decltype(K_)::value;
        constexpr int s = pp * NB + kb;
        const f32x4 z = nz, y = ny;
        nz = zx[0][((kb + 1) % NB) * 64 + lane];
        if constexpr (DUAL) ny = zx[1][((kb + 1) % NB) * 64 + lane];
        const f32x4 wa = fa[s % PF], wb = fb[s % PF];
        if constexpr (s + PF < S2) fetch(ra, std::integral_constant<int, s + PF>{}, fa, fb);
        ca = mfma4(wa.x, z[0], ca);
        cb = mfma4(wb.x, z[0], cb);
        ca2 = mfma4(wa.y, z[1], ca2);
        cb2 = mfma4(wb.y, z[1], cb2);
        ca = mfma4(wa.z, z[2], ca);
        cb = mfma4(wb.z, z[2], cb);
        ca2 = mfma4(wa.w, z[3], ca2);
        cb2 = mfma4(wb.w, z[3], cb2);
        if constexpr (DUAL) {
          da = mfma4(wa.x, y[0], da);
          db = mfma4(wb.x, y[0], db);
          da2 = mfma4(wa.y, y[1], da2);
          db2 = mfma4(wb.y, y[1], db2);
          da = mfma4(wa.z, y[2], da);
          db = mfma4(wb.z, y[2], db);
          da2 = mfma4(wa.w, y[3], da2);
          db2 = mfma4(wb.w, y[3], db2);
        }
        __builtin_amdgcn_sched_barrier(0);  // as in g1
      });
      epi(std::integral_constant<int, 2 * pp>{}, ca + ca2, da + da2);
      epi(std::integral_constant<int, 2 * pp + 1>{}, cb + cb2, db + db2);
    });
  };
  constexpr auto kOne = std::false_type{};
  constexpr auto kTwo = std::true_type{};

  // the KM step's constants (V5 form: EM_VVAR, PK_S1), the same for every layer
  const cfloat_p kmp = (cfloat_p)a.km;
  const LayerP KM = layer_params_at<EM_VVAR, PK_S1>(kmp, kmp, kmp);
  float mu = 0.f;

  __syncthreads();  // Z0 is in z0; layer 0's table is in tab
  {  // prologue: T0 = A Z0 + E0 - X (el_step's pro form), stored as T[0]
    const rsrc_t rt = mkrsrc(a.To, mbytes);
    g2(kOne, [&](auto LB_, const f32x4& q, const f32x4&) {
      constexpr int lb = decltype(LB_)::value;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const StepOut s = el_step<EM_VVAR>(
            q[r], Xr[lb][r], Ec[lb][r], Lc[lb][r], KM.b2, KM.b3, KM.ss2b, true,
            [&] { return KM.ss2; }, [&] { return KM.the; });
        Tc[lb][r] = s.t;
        bstore_s(rt, vo, row_off(b2o + lb, r), s.t);
      }
    });
  }

  for (int k = 0; k < K; ++k) {
    // v0 = Var of the learned step: what its own prologue pass forms from (Lc, T0 = Tc), beta1_k
    // of the row
#pragma unroll
    for (int b = 0; b < MB4; ++b) {
      const f32x4 b1 = tab_rows(T_B1, b2o + b);
      f32x4 vv;
#pragma unroll
      for (int r = 0; r < 4; ++r) vv[r] = StepOut{Ec[b][r], Lc[b][r], Tc[b][r]}.var(b1[r]);
      vx[0][(b2o + b) * 64 + lane] = vv;
    }
    __syncthreads();  // v0 complete; every wave is done reading z0, z1 of the layer before

    // 1. the learned Z-step (V2 / V3: no step size), theta_z_k of the row in the clamp form
    g1(kOne, g1_view(a.Wp + (int64_t)k * wl), [&](auto LB_, const f32x4& q, const f32x4&) {
      constexpr int lb = decltype(LB_)::value;
      const f32x4 tz = tab_rows(T_THZ, b1o + lb);
      f32x4 zv;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        Zl[lb][r] = z_step<PK_ROW>(Zc[lb][r], q[r], 0.f, [&] { return shrink_params(tz[r]); });
        zv[r] = Zl[lb][r];
        pin_agpr(Zl[lb][r]);
      }
      zx[0][(b1o + lb) * 64 + lane] = zv;
    });
    __syncthreads();  // z0 = Zl; every wave is done reading v0

    // 2. the learned E / L / T step on the row's beta2, beta3, (ss2,) theta_e (a float: the
    //    literal shrink form); the Var of both KM steps
    g2(kOne, [&](auto LB_, const f32x4& q, const f32x4&) {
      constexpr int lb = decltype(LB_)::value;
      const f32x4 b2 = tab_rows(T_B2, b2o + lb), b3 = tab_rows(T_B3, b2o + lb);
      const f32x4 te = tab_rows(T_THE, b2o + lb);
      f32x4 s2 = zero4;
      if constexpr (kV3) s2 = tab_rows(T_SS2, b2o + lb);
      f32x4 vs, vk;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const StepOut s = el_step<EMODE>(
            q[r], Xr[lb][r], Ec[lb][r], Lc[lb][r], b2[r], b3[r], 0.f, false,
            [&] { return s2[r]; }, [&] { return te[r]; });
        El[lb][r] = s.e;
        Ll[lb][r] = s.l;
        Tl[lb][r] = s.t;
        pin_agpr(El[lb][r]);
        pin_agpr(Ll[lb][r]);
        pin_agpr(Tl[lb][r]);
        vs[r] = s.var(KM.b1n);
        vk[r] = StepOut{Ec[lb][r], Lc[lb][r], Tc[lb][r]}.var(KM.b1n);
      }
      vx[1][(b2o + lb) * 64 + lane] = vs;
      vx[0][(b2o + lb) * 64 + lane] = vk;
    });
    __syncthreads();  // v0, v1 complete; every wave is done reading z0 and layer k's table

    // layer k + 1's table: the loads go out here, ahead of pass 3's fragments
    tab_issue(k + 1);

    // 3. both KM Z-steps on one stream of the shared A^T
    g1(kTwo, rat, [&](auto LB_, const f32x4& q0, const f32x4& q1) {
      constexpr int lb = decltype(LB_)::value;
      f32x4 zk, zs;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        Zc[lb][r] = z_step<PK_S1>(Zc[lb][r], q0[r], KM.s1, [&] { return KM.thz; });
        zk[r] = Zc[lb][r];
        pin_agpr(Zc[lb][r]);
        zs[r] = z_step<PK_S1>(Zl[lb][r], q1[r], KM.s1, [&] { return KM.thz; });
      }
      zx[0][(b1o + lb) * 64 + lane] = zk;
      zx[1][(b1o + lb) * 64 + lane] = zs;
    });
    tab_commit();     // older than every fragment load of pass 3: landed
    __syncthreads();  // z0 = Zk, z1 = Zs, the table of layer k + 1; all done reading v0, v1

    // 4. both KM E / L / T steps on one stream of A; the residual norm's terms of this lane's
    //    rows (safeguard_kernel's expression), and mu_0's: the KM step from the entry state
    double sn = 0.0, s0 = 0.0;
    g2(kTwo, [&](auto LB_, const f32x4& q0, const f32x4& q1) {
      constexpr int lb = decltype(LB_)::value;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float x = Xr[lb][r], ep = Ec[lb][r];
        const StepOut kk = el_step<EM_VVAR>(
            q0[r], x, ep, Lc[lb][r], KM.b2, KM.b3, KM.ss2b, false,
            [&] { return KM.ss2; }, [&] { return KM.the; });
        const StepOut ss = el_step<EM_VVAR>(
            q1[r], x, El[lb][r], Ll[lb][r], KM.b2, KM.b3, KM.ss2b, false,
            [&] { return KM.ss2; }, [&] { return KM.the; });
        const float t = a.beta * ss.t;
        const float e = a.c * ((ss.e - 2.0f * El[lb][r]) + ep);
        sn += (double)t * t + (double)e * e;
        const float t0 = a.beta * kk.t;
        const float e0 = a.c * ((kk.e - 2.0f * ep) + ep);
        s0 += (double)t0 * t0 + (double)e0 * e0;
        Ec[lb][r] = kk.e;
        Lc[lb][r] = kk.l;
        Tc[lb][r] = kk.t;
      }
    });
    // fixed order: the wave's four lane groups, then the four waves in order
    sn += __shfl_xor(sn, 16, 64);
    sn += __shfl_xor(sn, 32, 64);
    s0 += __shfl_xor(s0, 16, 64);
    s0 += __shfl_xor(s0, 32, 64);
    if (g == 0) {
      red[0][w][lane] = sn;
      red[1][w][lane] = s0;
    }
    __syncthreads();
    double tn = red[0][0][lane & 15], t0 = red[1][0][lane & 15];
#pragma unroll
    for (int q = 1; q < kWaves; ++q) {
      tn += red[0][q][lane & 15];
      t0 += red[1][q][lane & 15];
    }
    if (k == 0) mu = (float)sqrt(t0);  // mu_0 = |S(Z0, E0, L0, T0, X, E0)|
    const float nrm = (float)sqrt(tn);
    const bool keep = nrm < a.thresh * mu;
    {
      const float mu0 = mu;
      switch (a.updater) {
        case DLADMM_MU_EMA: mu = keep ? a.param * nrm + (1.0f - a.param) * mu0 : mu0; break;
        case DLADMM_MU_GS: mu = keep ? (1.0f - a.param) * mu0 : mu0; break;
        case DLADMM_MU_RT: mu = keep ? nrm : mu0; break;
        default: mu = 1e10f; break;  // BlankUpdater.step (mu_updater.py:108-110)
      }
    }
    // safeguarded valid columns of the group: one integer atomic per workgroup
    const unsigned long long bal = __ballot(cv && !keep && g == 0);
    if (threadIdx.x == 0 && bal) atomicAdd(a.count + k, (int)__popcll(bal));

    // select (lane-local) and store the selected state alone
    const rsrc_t rzo = mkrsrc(a.Zo + (int64_t)k * n * a.ldo, zbytes);
    const rsrc_t reo = mkrsrc(a.Eo + (int64_t)k * m * a.ldo, mbytes);
    const rsrc_t rlo = mkrsrc(a.Lo + (int64_t)k * m * a.ldo, mbytes);
    const rsrc_t rto = mkrsrc(a.To + (int64_t)(k + 1) * m * a.ldo, mbytes);
#pragma unroll
    for (int b = 0; b < NB4; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        Zc[b][r] = keep ? Zl[b][r] : Zc[b][r];
        bstore_s(rzo, vo, row_off(b1o + b, r), Zc[b][r]);
        pin_agpr(Zc[b][r]);
      }
#pragma unroll
    for (int b = 0; b < MB4; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        Ec[b][r] = keep ? El[b][r] : Ec[b][r];
        Lc[b][r] = keep ? Ll[b][r] : Lc[b][r];
        Tc[b][r] = keep ? Tl[b][r] : Tc[b][r];
        const uint32_t so = row_off(b2o + b, r);
        bstore_s(reo, vo, so, Ec[b][r]);
        bstore_s(rlo, vo, so, Lc[b][r]);
        bstore_s(rto, vo, so, Tc[b][r]);
      }
  }
  if (a.mu_out && w == 0 && g == 0 && cv) a.mu_out[col] = mu;
}

hipError_t launch_lskm_rowp_fused(int variant, const LskmRowpArgs& a, int grid, hipStream_t s) {
  if (variant == DLADMM_V3_FULL)
    hipLaunchKernelGGL((lskm_rowp_fused_kernel<kShapeMP[2], kShapeNP[2], EM_VVAR>), dim3(grid),
                       dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((lskm_rowp_fused_kernel<kShapeMP[2], kShapeNP[2], EM_V1>), dim3(grid),
                       dim3(256), 0, s, a);
  return hipGetLastError();
}

}  // namespace dladmm
