// dladmm_lskm_news_fused.hip -- the newS scripts' learned + safeguarded KM forward
// (test_syn_l1l1_newS.py:188-268, its _Acols, tied and partially tied forms) as ONE launch at the
// 256 x 512 register shape, fp32.
//
// The multi-launch path (lskm_news.py) runs, per safeguarded layer, three one-step ELZ forwards
// (the KM candidate, the L2O candidate, the KM step from the L2O candidate with its tail product),
// six weight packs and safeguard_news_kernel: seven product passes, three candidate states and two
// saved products through HBM.  Here a workgroup keeps its 16 columns for every layer, in the
// geometry of lskm_fused_kernel (dladmm_lskm_fused.hip) and path 5: wave w owns G1 output blocks
// 8w .. 8w + 7 and G2 blocks 4w .. 4w + 3, rows in the C/D map of v_mfma_f32_16x16x4_f32, weight
// fragments straight from L2 by 16-byte buffer loads RS_PF steps ahead (pack order 2), B operands
// from LDS images of the group's column state.  No workgroup waits for another.
//
// The loop carries (E, L, Z) and each step runs E, L, then Z, so both candidates' E / L halves
// start from A Zc -- the product the layer before already formed as A Zl or A Zk.  It is carried
// in registers (Pc) and selected per column with the rest of the state, which removes the two
// prologue products of the multi-launch path.
//
// Registers, across all layers: the current state (Zc 32, Ec / Lc / Pc 16 each), X 16, the L2O
// candidate (Zl 32, El / Ll / Pl 16 each), En 16 and the column's mu.  The KM candidate is formed
// in place over the current state.  LDS: two Z images z0, z1 (2 x 32 KiB), two Var images v0, v1
// (2 x 16 KiB), an fp64 pad.
//
// Layer k >= 0, five weight streams:
//   a. no product: (El, Ll) = the VVar E / L half from (Ec, Lc, Pc) on the E / L slots of layer
//      k - 1, v1 = Ll + beta1_k Tl;  (Ek, Lk) = the V7 half, in place, v0 = Lk + b Tk.  Layer 0
//      is a Z-step only: both keep (E0, L0), T0 = (P0 + E0) - X (el_step's pro form).
//   b. G1, W_k on v1:     Zl = S(Zc - s1_k W_k v1, theta_z_k)                  -> z1
//      G1, -A^T on v0:    Zk = S(Zc - ss1 A^T v0, ss1 alpha), in place over Zc -> z0
//   c. dual G2, A on z0 and z1, each fragment read once: Pk (over Pc), Pn = A Zl; on the Pn side
//      the V7 half from the L2O candidate: En, Varnn = Ln + b Tn                -> v0
//   d. G1, -A^T on v0:    Znn = S(Zl - ss1 A^T Varnn, ss1 alpha) (not kept)     -> z0
//      dd = sum (Znn - Zl)^2
//   e. G2, A on z0:       Pnn;  r1 = sum ((Pnn + En) - X)^2,  ad = sum (Pnn - Pn)^2
//   f. Snorm = sqrt(max(r1 + (dd inv_bs - ad), 0)) (safeguard_news_kernel's expression; fp64: a
//      lane's rows, its wave's four lane groups, the four waves in order through LDS), keep =
//      Snorm < (1 - delta) mu, the mu update of safeguard_kernel, the lane-local select of
//      (E, L, Z, P), non-temporal stores of slab k, mask[k], one integer atomic on count[k].
// mu_0 = Snorm_ELZ(E0, L0, Z0, X) (:196) is the same c - f from the entry state: the loop starts
// at k = -1 with both Z images = Z0 and (Zl, El, Ll) = (Z0, E0, L0), so pass c leaves Pc = Pl =
// A Z0, and f sets mu instead of deciding.
//
// Arithmetic: G1 one fma chain per output block over k in order, G2 two chains (k sub-steps x, z
// and y, w) summed once, the elementwise expressions of dladmm_step.h (V7 = EM_V1 / PK_S1; the
// learned step EM_VVAR / PK_S1 with s1 = 1 for the untied model, where 1 * q is q) -- every stored
// value is the multi-launch path's bit for bit as long as the decisions agree; the norm is the
// same fp64 sums in another order (tests/test_gpu_news_lskm_fused.py).
#include "dladmm_lskm_news_fused.h"

#include "dladmm_fused_rs_kernel.h"  // RS_PF; dladmm_step.h

namespace dladmm {

template <int MP, int NP>
__global__ __launch_bounds__(256, 1) void lskm_news_fused_kernel(const LskmNewsArgs a) {
  constexpr int MB = MP / 16, NB = NP / 16;
  constexpr int NB4 = NB / kWaves, MB4 = MB / kWaves;   // output blocks per wave
  static_assert(NB4 % 2 == 0 && MB4 % 2 == 0, "whole output pairs");
  constexpr int S1 = (NB4 / 2) * MB, S2 = (MB4 / 2) * NB;  // MFMA steps of a wave's G1 / G2
  constexpr int PF = RS_PF;
  __shared__ f32x4 zx[2][NB * 64];  // Z images of the 16 columns, block b at [b * 64 + lane]
  __shared__ f32x4 vx[2][MB * 64];  // Var images
  __shared__ double red[3][kWaves][16];  // per-wave column partials: r1, dd, ad

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

  float Zc[NB4][4], Ec[MB4][4], Lc[MB4][4], Pc[MB4][4], Xr[MB4][4];  // current state, X
  float Zl[NB4][4], El[MB4][4], Ll[MB4][4], Pl[MB4][4];              // L2O candidate
  float En[MB4][4];                                                  // E of the KM step from it
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
        zv[r] = Zl[b][r] = Zc[b][r];
        pin_agpr(Zc[b][r]);
        pin_agpr(Zl[b][r]);
      }
      zx[0][(b1o + b) * 64 + lane] = zv;
      zx[1][(b1o + b) * 64 + lane] = zv;
    }
#pragma unroll
    for (int b = 0; b < MB4; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint32_t ro = (uint32_t)(16 * (b2o + b) + r);
        Xr[b][r] = bload(rx, ox + ro * (uint32_t)(a.ldx * 4));
        El[b][r] = Ec[b][r] = bload(re, oe + ro * (uint32_t)(a.lde0 * 4));
        Ll[b][r] = Lc[b][r] = bload(rl, ol + ro * (uint32_t)(a.ldl0 * 4));
        Pc[b][r] = Pl[b][r] = En[b][r] = 0.f;
      }
  }

  const uint32_t vo = lane_off(a.ldo);
  const uint32_t ld4 = (uint32_t)(a.ldo * 4);
  const uint32_t zbytes = (uint32_t)(n * a.ldo * 4), mbytes = (uint32_t)(m * a.ldo * 4);
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

  // G1: this wave's n-row blocks of (packed weight) x Var, Var (all m rows) from image IMG of vx.
  // epi(block, q) per output block.
  auto g1 = [&](auto IMG_, rsrc_t rw, auto&& epi) {
    constexpr int im = decltype(IMG_)::value;
    f32x4 fa[PF], fb[PF];
    prefetch(std::integral_constant<int, S1>{}, rw, fa, fb);
    // the B operand of step s + 1 is read from LDS ahead of step s's MFMAs (the wrap-around read
    // after the last step is of the same image: in range, unused)
    f32x4 nv = vx[im][lane];
    static_for<NB4 / 2>([&](auto P_) {
      constexpr int pp = decltype(P_)::value;
      f32x4 ca = zero4, cb = zero4;
      static_for<MB>([&](auto J_) {
        constexpr int jb = decltype(J_)::value;
        constexpr int s = pp * MB + jb;
        const f32x4 v = nv;
        nv = vx[im][((jb + 1) % MB) * 64 + lane];
        const f32x4 wa = fa[s % PF], wb = fb[s % PF];
        if constexpr (s + PF < S1) fetch(rw, std::integral_constant<int, s + PF>{}, fa, fb);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          ca = mfma4(wa[q], v[q], ca);
          cb = mfma4(wb[q], v[q], cb);
        }
        // keep the step's refill with the step (lskm_fused_kernel: the scheduler otherwise sinks
        // every fragment load to its use)
        __builtin_amdgcn_sched_barrier(0);
      });
      epi(std::integral_constant<int, 2 * pp>{}, ca);
      epi(std::integral_constant<int, 2 * pp + 1>{}, cb);
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
  constexpr auto kImg0 = std::integral_constant<int, 0>{};
  constexpr auto kImg1 = std::integral_constant<int, 1>{};

  // the KM step's constants (V7: EM_V1, PK_S1), the same for every layer
  const cfloat_p kmp = (cfloat_p)a.km;
  const LayerP KM = layer_params_at<EM_V1, PK_S1>(kmp, kmp, kmp);
  const double inv_bs = (double)*(cfloat_p)a.inv_bs;
  typedef const float* const __attribute__((address_space(4)))* ctab_p;
  float mu = 0.f;

  for (int k = -1; k < K; ++k) {
    if (k >= 0) {
      // the learned step k: Z slots (and beta1) of layer k, E / L slots of layer k - 1
      const cfloat_p sk = (cfloat_p)a.scal + k * DLADMM_NSCALAR;
      const cfloat_p se = (cfloat_p)a.scal + (k > 0 ? k - 1 : 0) * DLADMM_NSCALAR;
      const LayerP P = layer_params_at<EM_VVAR, PK_S1>(sk, se, sk);
      const bool first = k == 0;  // a Z-step only: E, L stay, T0 = (P0 + E0) - X
      // a. both E / L halves from (Ec, Lc, Pc): the L2O one first, the KM one in place
#pragma unroll
      for (int b = 0; b < MB4; ++b) {
        f32x4 vl, vk;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float x = Xr[b][r], pc = Pc[b][r], e0 = Ec[b][r], l0 = Lc[b][r];
          const StepOut sl = el_step<EM_VVAR>(
              pc, x, e0, l0, P.b2, P.b3, P.ss2b, first, [&] { return P.ss2; },
              [&] { return P.the; });
          const StepOut sm = el_step<EM_V1>(
              pc, x, e0, l0, KM.b2, KM.b3, KM.ss2b, first, [&] { return KM.ss2; },
              [&] { return KM.the; });
          El[b][r] = sl.e;
          Ll[b][r] = sl.l;
          pin_agpr(El[b][r]);
          pin_agpr(Ll[b][r]);
          vl[r] = sl.var(P.b1n);
          Ec[b][r] = sm.e;
          Lc[b][r] = sm.l;
          vk[r] = sm.var(KM.b1n);
        }
        vx[1][(b2o + b) * 64 + lane] = vl;
        vx[0][(b2o + b) * 64 + lane] = vk;
      }
      __syncthreads();  // v0, v1 complete; every wave is done reading z0 of the layer before

      // b. the learned Z-step, then the KM Z-step in place
      g1(kImg1, g1_view(((ctab_p)a.wtab)[k]), [&](auto LB_, const f32x4& q) {
        constexpr int lb = decltype(LB_)::value;
        f32x4 zv;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          Zl[lb][r] = z_step<PK_S1>(Zc[lb][r], q[r], P.s1, [&] { return P.thz; });
          zv[r] = Zl[lb][r];
          pin_agpr(Zl[lb][r]);
        }
        zx[1][(b1o + lb) * 64 + lane] = zv;
      });
      g1(kImg0, rat, [&](auto LB_, const f32x4& q) {
        constexpr int lb = decltype(LB_)::value;
        f32x4 zv;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          Zc[lb][r] = z_step<PK_S1>(Zc[lb][r], q[r], KM.s1, [&] { return KM.thz; });
          zv[r] = Zc[lb][r];
          pin_agpr(Zc[lb][r]);
        }
        zx[0][(b1o + lb) * 64 + lane] = zv;
      });
    }
    __syncthreads();  // z0 = Zk, z1 = Zl (k = -1: both Z0); every wave is done reading v0, v1

    // c. both products on one stream of A; the KM step's E / L half from the L2O candidate
    g2(kTwo, [&](auto LB_, const f32x4& q0, const f32x4& q1) {
      constexpr int lb = decltype(LB_)::value;
      f32x4 vn;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        Pc[lb][r] = q0[r];
        Pl[lb][r] = q1[r];
        const StepOut sn = el_step<EM_V1>(
            q1[r], Xr[lb][r], El[lb][r], Ll[lb][r], KM.b2, KM.b3, KM.ss2b, false,
            [&] { return KM.ss2; }, [&] { return KM.the; });
        En[lb][r] = sn.e;
        vn[r] = sn.var(KM.b1n);
        pin_agpr(Pl[lb][r]);
      }
      vx[0][(b2o + lb) * 64 + lane] = vn;
    });
    __syncthreads();  // v0 = Varnn; every wave is done reading z0, z1

    // d. the KM Z-step from the L2O candidate (not kept); dd of this lane's rows
    double r1 = 0.0, dd = 0.0, ad = 0.0;
    g1(kImg0, rat, [&](auto LB_, const f32x4& q) {
      constexpr int lb = decltype(LB_)::value;
      f32x4 zv;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        zv[r] = z_step<PK_S1>(Zl[lb][r], q[r], KM.s1, [&] { return KM.thz; });
        const float dz = zv[r] - Zl[lb][r];
        dd += (double)dz * dz;
      }
      zx[0][(b1o + lb) * 64 + lane] = zv;
    });
    __syncthreads();  // z0 = Znn; every wave is done reading v0

    // e. A Znn; r1 and ad of this lane's rows (safeguard_news_kernel's expressions)
    g2(kOne, [&](auto LB_, const f32x4& q, const f32x4&) {
      constexpr int lb = decltype(LB_)::value;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float t = (q[r] + En[lb][r]) - Xr[lb][r];
        const float dp = q[r] - Pl[lb][r];
        r1 += (double)t * t;
        ad += (double)dp * dp;
      }
    });

    // f. fixed order: the wave's four lane groups, then the four waves in order
    r1 += __shfl_xor(r1, 16, 64);
    r1 += __shfl_xor(r1, 32, 64);
    dd += __shfl_xor(dd, 16, 64);
    dd += __shfl_xor(dd, 32, 64);
    ad += __shfl_xor(ad, 16, 64);
    ad += __shfl_xor(ad, 32, 64);
    if (g == 0) {
      red[0][w][lane] = r1;
      red[1][w][lane] = dd;
      red[2][w][lane] = ad;
    }
    __syncthreads();
    double t1 = red[0][0][lane & 15], t2 = red[1][0][lane & 15], t3 = red[2][0][lane & 15];
#pragma unroll
    for (int q = 1; q < kWaves; ++q) {
      t1 += red[0][q][lane & 15];
      t2 += red[1][q][lane & 15];
      t3 += red[2][q][lane & 15];
    }
    // P2 is positive definite: the clamp only meets rounding at d ~ 0 (safeguard_news_kernel)
    const double qn = t1 + (t2 * inv_bs - t3);
    const float nrm = (float)sqrt(qn > 0.0 ? qn : 0.0);
    if (k < 0) {  // mu_0 = Snorm_ELZ(E0, L0, Z0, X): no decision
      mu = nrm;
      continue;
    }
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
    if (a.mask && w == 0 && g == 0 && cv) a.mask[(int64_t)k * a.B + col] = keep ? 1 : 0;

    // select (lane-local) and store the selected state alone
    const rsrc_t rzo = mkrsrc(a.Zo + (int64_t)k * n * a.ldo, zbytes);
    const rsrc_t reo = mkrsrc(a.Eo + (int64_t)k * m * a.ldo, mbytes);
    const rsrc_t rlo = mkrsrc(a.Lo + (int64_t)k * m * a.ldo, mbytes);
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
        Pc[b][r] = keep ? Pl[b][r] : Pc[b][r];
        const uint32_t so = row_off(b2o + b, r);
        bstore_s(reo, vo, so, Ec[b][r]);
        bstore_s(rlo, vo, so, Lc[b][r]);
      }
  }
  if (a.mu_out && w == 0 && g == 0 && cv) a.mu_out[col] = mu;
}

hipError_t launch_lskm_news_fused(const LskmNewsArgs& a, int grid, hipStream_t s) {
  hipLaunchKernelGGL((lskm_news_fused_kernel<kShapeMP[2], kShapeNP[2]>), dim3(grid), dim3(256), 0,
                     s, a);
  return hipGetLastError();
}

}  // namespace dladmm
