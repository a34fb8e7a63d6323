// dladmm_sl2.hip -- the S-L2 training term of main_syn_l1l1-sl2_scalar.py / -sl2_full.py
// (:146-157, :263-274) and its adjoint as ONE launch at the 256 x 512 register shape, fp32:
//   S = [beta Tn ; c (En - 2 E + Ep)],  (Zn, En, Tn) = one classic KM step (:117-143) from the
//   network's last state (Z, E, L, T),   colsum[b] = |S[:, b]|^2,
// and, in the adjoint form, the cotangents of w sum_b colsum[b] w.r.t. Z, E, L, T and Ep -- what a
// dladmm_bwd_f32 call takes as its gZ / gE / gL / gT beside the fused L1L1 term.
//
// Geometry: path 5's, as in dladmm_lskm_fused.hip -- one workgroup of four waves keeps 16 columns,
// wave w owns G1 output blocks 8w .. 8w + 7 and G2 blocks 4w .. 4w + 3, rows in the C/D map of
// v_mfma_f32_16x16x4_f32, weight fragments straight from L2 by 16-byte buffer loads RS_PF steps
// ahead (pack order 2), B operands from LDS images of the group's columns.
//
// Four weight streams (the torch-op form: the same four products, each a GEMM launch with its
// operand through HBM, and a dozen elementwise passes forward and as many in autograd):
//   1. G1, -A^T on Var = L + beta T (v)        Zn = S(Z - ss1 A^T Var, thz)            -> z
//   2. G2, A on z, two chains                  TTn, En, Tn;  the lane's rows of |S|^2 in fp64;
//        the seeds (lane-local in the E / L / T layout), r = c (En - 2 E + Ep), w = coef:
//          gTn = 2 w beta^2 Tn,  gEn = gTn + 2 w c r,  gV = gEn [En != 0],
//          gPn = gTn - ss2 beta gV                                                     -> v (-gPn)
//        stores gE = gV - ss2 beta gV - 4 w c r, gEp = 2 w c r; keeps gV
//      |S|^2 per column: the lane's rows, the wave's four lane groups, the four waves in order
//      through LDS.  The sum-only form ends here.
//   3. G1, -A^T on -gPn (v)                    gU = (A^T gPn) [Zn != 0]: stored as gZ  -> z
//   4. G2, A on z                              gVar = -ss1 A gU,  gL = -ss2 gV + gVar,
//                                              gT = beta gVar
// Registers across the streams: Zn 32 (its sign pattern is the Z-step's mask), then E, L, X, Ep
// 16 each until stream 2 and gV 16 after it.  LDS: one Z image (32 KiB) and one Var image
// (16 KiB), each reused by the adjoint pass, and the fp64 pad.
// The masks [Zn != 0], [En != 0] are autograd's for thresholds > 0 (dladmm_sl2_f32 rejects the
// rest).  Rows past m / n and columns past B read zero and stay zero through every stream; their
// stores fall outside the buffer views and are dropped.
#include "dladmm_sl2.h"

#include "dladmm_fused_rs_kernel.h"  // RS_PF; dladmm_step.h

namespace dladmm {

template <int MP, int NP, bool GRAD>
__global__ __launch_bounds__(256, 1) void sl2_fused_kernel(const Sl2Args a) {
  constexpr int MB = MP / 16, NB = NP / 16;
  constexpr int NB4 = NB / kWaves, MB4 = MB / kWaves;   // output blocks per wave
  static_assert(NB4 % 2 == 0 && MB4 % 2 == 0, "whole output pairs");
  constexpr int S1 = (NB4 / 2) * MB, S2 = (MB4 / 2) * NB;  // MFMA steps of a wave's G1 / G2
  constexpr int PF = RS_PF;
  __shared__ f32x4 zx[NB * 64];  // Z image of the 16 columns, block b at [b * 64 + lane]
  __shared__ f32x4 vx[MB * 64];  // Var image
  __shared__ double red[kWaves][16];  // per-wave column partials of |S|^2

  const int grp = blockIdx.x;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4;
  const int64_t col = (int64_t)grp * 16 + (lane & 15);
  const bool cv = col < a.B;
  const int m = a.m, n = a.n;
  auto lane_off = [&](int64_t ld) -> uint32_t {
    return cv ? (uint32_t)((col + (int64_t)(4 * g) * ld) * 4) : kOOB;
  };
  const int b1o = w * NB4, b2o = w * MB4;  // first output block of this wave in G1 / G2
  const float beta = a.beta, ss2 = a.ss2;

  float Zn[NB4][4], Ec[MB4][4], Lc[MB4][4], Xr[MB4][4], Ep[MB4][4];
  {
    const rsrc_t rz = mkrsrc(a.Z, (uint32_t)(n * a.ldz * 4));
    const rsrc_t re = mkrsrc(a.E, (uint32_t)(m * a.lde * 4));
    const rsrc_t rl = mkrsrc(a.L, (uint32_t)(m * a.ldl * 4));
    const rsrc_t rt = mkrsrc(a.T, (uint32_t)(m * a.ldt * 4));
    const rsrc_t rx = mkrsrc(a.X, (uint32_t)(m * a.ldx * 4));
    const rsrc_t rp = mkrsrc(a.Ep, (uint32_t)(m * a.ldep * 4));
    const uint32_t oz = lane_off(a.ldz), oe = lane_off(a.lde), ol = lane_off(a.ldl),
                   ot = lane_off(a.ldt), ox = lane_off(a.ldx), op = lane_off(a.ldep);
#pragma unroll
    for (int b = 0; b < NB4; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        Zn[b][r] = bload(rz, oz + (uint32_t)((16 * (b1o + b) + r) * a.ldz * 4));
#pragma unroll
    for (int b = 0; b < MB4; ++b) {
      f32x4 vv;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const uint32_t ro = (uint32_t)(16 * (b2o + b) + r);
        Xr[b][r] = bload(rx, ox + ro * (uint32_t)(a.ldx * 4));
        Ec[b][r] = bload(re, oe + ro * (uint32_t)(a.lde * 4));
        Lc[b][r] = bload(rl, ol + ro * (uint32_t)(a.ldl * 4));
        Ep[b][r] = bload(rp, op + ro * (uint32_t)(a.ldep * 4));
        const float t = bload(rt, ot + ro * (uint32_t)(a.ldt * 4));
        vv[r] = StepOut{Ec[b][r], Lc[b][r], t}.var(beta);  // Varn = L + beta T     (:126)
      }
      vx[(b2o + b) * 64 + lane] = vv;
    }
  }

  const uint32_t vo = lane_off(a.ldg);
  const uint32_t ld4 = (uint32_t)(a.ldg * 4);
  const uint32_t zbytes = (uint32_t)(n * a.ldg * 4), mbytes = (uint32_t)(m * a.ldg * 4);
  const uint32_t vf = (uint32_t)(lane * 16);    // lane offset inside a 1-KiB fragment
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  auto frag = [&](rsrc_t r, int off) -> f32x4 {
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)vf, off, 0));
  };
  // byte offset of row 16 b + r of a [rows][ldg] output (opaque base: formed where it is used)
  auto row_off = [&](int b, int r) -> uint32_t {
    uint32_t o = (uint32_t)(16 * b) * ld4;
    asm volatile("" : "+s"(o));
    return o + (uint32_t)r * ld4;
  };

  // The weight-fragment window of a pass, as in lskm_fused_kernel: step s reads slot s % PF and
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
  const rsrc_t ra = mkrsrc(a.Ap + (int64_t)(b2o / 2) * NB * 2 * kFrag,
                           (uint32_t)(S2 * 2 * kFrag * 4));
  const rsrc_t rat = mkrsrc(a.Atp + (int64_t)(b1o / 2) * MB * 2 * kFrag,
                            (uint32_t)(S1 * 2 * kFrag * 4));

  // G1: this wave's n-row blocks of -A^T x (the Var image, all m rows); one fma chain per output
  // block over k in order.  epi(block, q) per output block.
  auto g1 = [&](auto&& epi) {
    f32x4 fa[PF], fb[PF];
    prefetch(std::integral_constant<int, S1>{}, rat, fa, fb);
    // the B operand of step s + 1 is read from LDS ahead of step s's MFMAs (the wrap-around read
    // after the last step is of the same image: in range, unused)
    f32x4 nv = vx[lane];
    static_for<NB4 / 2>([&](auto P_) {
      constexpr int pp = decltype(P_)::value;
      f32x4 ca = zero4, cb = zero4;
      static_for<MB>([&](auto J_) {
        constexpr int jb = decltype(J_)::value;
        constexpr int s = pp * MB + jb;
        const f32x4 v = nv;
        nv = vx[((jb + 1) % MB) * 64 + lane];
        const f32x4 wa = fa[s % PF], wb = fb[s % PF];
        if constexpr (s + PF < S1) fetch(rat, std::integral_constant<int, s + PF>{}, fa, fb);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          ca = mfma4(wa[q], v[q], ca);
          cb = mfma4(wb[q], v[q], cb);
        }
        __builtin_amdgcn_sched_barrier(0);  // keep the step's refill with the step
      });
      epi(std::integral_constant<int, 2 * pp>{}, ca);
      epi(std::integral_constant<int, 2 * pp + 1>{}, cb);
    });
  };
  // G2: this wave's m-row blocks of A x (the Z image, all n rows).  Two chains per block (k
  // sub-steps x, z and y, w) summed once, as everywhere.
  auto g2 = [&](auto&& epi) {
    f32x4 fa[PF], fb[PF];
    prefetch(std::integral_constant<int, S2>{}, ra, fa, fb);
    f32x4 nz = zx[lane];  // read ahead as in g1
    static_for<MB4 / 2>([&](auto P_) {
      constexpr int pp = decltype(P_)::value;
      f32x4 ca = zero4, cb = zero4, ca2 = zero4, cb2 = zero4;
      static_for<NB>([&](auto K_) {
        constexpr int kb = decltype(K_)::value;
        constexpr int s = pp * NB + kb;
        const f32x4 z = nz;
        nz = zx[((kb + 1) % NB) * 64 + lane];
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
        __builtin_amdgcn_sched_barrier(0);  // as in g1
      });
      epi(std::integral_constant<int, 2 * pp>{}, ca + ca2);
      epi(std::integral_constant<int, 2 * pp + 1>{}, cb + cb2);
    });
  };

  const ShrinkP thz = shrink_params(a.thz);
  __syncthreads();  // the Var image is complete

  // 1. the KM Z-step (:127-130)
  g1([&](auto LB_, const f32x4& q) {
    constexpr int lb = decltype(LB_)::value;
    f32x4 zv;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      Zn[lb][r] = z_step<PK_S1>(Zn[lb][r], q[r], a.ss1, [&] { return thz; });
      zv[r] = Zn[lb][r];
    }
    zx[(b1o + lb) * 64 + lane] = zv;
  });
  __syncthreads();  // z = Zn; every wave is done reading the Var image

  // 2. the KM E / T step (:133-140), the norm's terms of this lane's rows, the adjoint's seeds
  float w1 = 0.f;  // 2 w
  if constexpr (GRAD) w1 = 2.0f * ((cfloat_p)a.coef)[0];
  const float wb2 = w1 * (beta * beta), wc = w1 * a.c, sb = ss2 * beta;
  float gV[MB4][4];
  double sn = 0.0;
  {
    const rsrc_t rge = mkrsrc(a.gE, GRAD ? mbytes : 0u);
    // a null gEp (Ep is no saved layer: K == 1) drops its stores through a zero-size view
    const rsrc_t rgp = mkrsrc(a.gEp, (GRAD && a.gEp) ? mbytes : 0u);
    g2([&](auto LB_, const f32x4& q) {
      constexpr int lb = decltype(LB_)::value;
      f32x4 gp;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e0 = Ec[lb][r];
        const StepOut s = el_step<EM_VVAR>(
            q[r], Xr[lb][r], e0, Lc[lb][r], beta, beta, 0.f, false,
            [&] { return ss2; }, [&] { return ss2; });
        const float t = beta * s.t;
        const float rr = a.c * ((s.e - 2.0f * e0) + Ep[lb][r]);
        sn += (double)t * t + (double)rr * rr;
        if constexpr (GRAD) {
          const float gTn = wb2 * s.t;
          const float wr = wc * rr;                     // 2 w c r
          const float gv = s.e != 0.0f ? gTn + wr : 0.0f;
          gV[lb][r] = gv;
          gp[r] = sb * gv - gTn;                        // -gPn
          const uint32_t so = row_off(b2o + lb, r);
          bstore_s(rge, vo, so, (gv - sb * gv) - 2.0f * wr);
          bstore_s(rgp, vo, so, wr);
        }
      }
      if constexpr (GRAD) vx[(b2o + lb) * 64 + lane] = gp;
    });
  }
  // fixed order: the wave's four lane groups, then the four waves in order
  sn += __shfl_xor(sn, 16, 64);
  sn += __shfl_xor(sn, 32, 64);
  if (g == 0) red[w][lane] = sn;
  __syncthreads();  // the partials; v = -gPn; every wave is done reading z
  if (w == 0 && g == 0 && cv) {
    double tn = red[0][lane];
#pragma unroll
    for (int q = 1; q < kWaves; ++q) tn += red[q][lane];
    a.colsum[col] = tn;
  }
  if constexpr (GRAD) {
    // 3. A^T gPn through the Z-step's mask: the cotangent of Z
    {
      const rsrc_t rgz = mkrsrc(a.gZ, zbytes);
      g1([&](auto LB_, const f32x4& q) {
        constexpr int lb = decltype(LB_)::value;
        f32x4 gu;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          gu[r] = Zn[lb][r] != 0.0f ? q[r] : 0.0f;
          bstore_s(rgz, vo, row_off(b1o + lb, r), gu[r]);
        }
        zx[(b1o + lb) * 64 + lane] = gu;
      });
    }
    __syncthreads();  // z = gU

    // 4. A gU: the cotangents of Var's operands L and T
    {
      const rsrc_t rgl = mkrsrc(a.gL, mbytes);
      const rsrc_t rgt = mkrsrc(a.gT, mbytes);
      g2([&](auto LB_, const f32x4& q) {
        constexpr int lb = decltype(LB_)::value;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float gvar = -a.ss1 * q[r];
          const uint32_t so = row_off(b2o + lb, r);
          bstore_s(rgl, vo, so, gvar - ss2 * gV[lb][r]);
          bstore_s(rgt, vo, so, beta * gvar);
        }
      });
    }
  }
}

// colsum's total in a fixed order: lane l sums the entries l, l + 64, ... in order, then the
// wave's xor tree
__global__ __launch_bounds__(64) void sl2_total_kernel(const double* colsum, int B,
                                                       double* total) {
  double s = 0.0;
  for (int i = threadIdx.x; i < B; i += 64) s += colsum[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (threadIdx.x == 0) total[0] = s;
}

hipError_t launch_sl2(const Sl2Args& a, bool grad, int grid, hipStream_t s) {
  if (grad)
    hipLaunchKernelGGL((sl2_fused_kernel<kShapeMP[2], kShapeNP[2], true>), dim3(grid), dim3(256),
                       0, s, a);
  else
    hipLaunchKernelGGL((sl2_fused_kernel<kShapeMP[2], kShapeNP[2], false>), dim3(grid),
                       dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_sl2_total(const double* colsum, int B, double* total, hipStream_t s) {
  hipLaunchKernelGGL(sl2_total_kernel, dim3(1), dim3(64), 0, s, colsum, B, total);
  return hipGetLastError();
}

}  // namespace dladmm
