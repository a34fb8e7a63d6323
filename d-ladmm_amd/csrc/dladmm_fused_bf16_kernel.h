// dladmm_bf16_fused_kernel.h -- MI355X (gfx950) fused K-layer D-LADMM forward with bf16 MFMA
// operands (DLADMM_PREC_BF16 + DLADMM_F_BF16_FUSED, forward path 7).  The kernel template;
// dladmm_fused_bf16.hip instantiates it.
//
// Arithmetic: that of the bf16 tile kernels (path 3) -- A, -W_k and the state operands Var / Z_k
// rounded to bf16 (RNE), v_mfma_f32_16x16x32_bf16 with fp32 accumulation, every elementwise
// update in fp32 through dladmm_step.h in the reference's operation order (the prologue
// T_0 = A Z0 + E0 - X on bf16 operands too) -- as ONE launch for all K layers with the state in
// registers, where path 3 runs 2K + 1 launches and round-trips every layer through HBM.
//
// Geometry (that of the split-f16 kernel, path 4): one workgroup = 4 waves = 64 batch columns,
// wave w owns 16 columns; lane l holds column l & 15 and rows 16 b + 4 (l >> 4) + r of every state
// block b.  k-step s of a 16 x 16 x 32 MFMA contracts rows 32 s .. 32 s + 31 = the lane's own
// registers [2s][0..3], [2s+1][0..3]; the packed weights carry that k order (pack_frags_kernel,
// bf16 = 2), so an epilogue's output is the next product's B operand with no lane movement.
//
// What is this kernel's own:
//   * Operands.  The B operand of a k-step is ONE bf16x8 (4 registers): the epilogue rounds its
//     fp32 results once (v_cvt_pk_bf16_f32) when a block pair is complete.  No column scales, no
//     hi / lo halves, no provisional scale, no re-split pass; one MFMA per k-step.
//   * Registers (per lane at 256 x 512; one wave per SIMD, 512 registers).  AGPR-pinned: fp32 Z
//     (128), Zpk (64), Vpk (32) = 224.  VGPRs: E, L (128), four fragments in rotation (16), two
//     accumulators (8), the deferred tiles (12), V1's beta ring (36), temporaries.  fp32 Z STAYS
//     RESIDENT across layers: G1's epilogue reads Z_{k-1} from its own register and overwrites it,
//     so no Z block ever travels through the LDS ring, lean mode needs no Z workspace, and the
//     ring carries weights only.  fp32 Var is never kept: it feeds nothing but the next G1's B
//     operand.  X rows wait in LDS (64 KiB), read back once per block.
//   * Weight stream.  -W_k and A as 1 KiB fragments (one per k-step, half of path 4's stream) in
//     one flat chunk sequence A, -W_0, A, -W_1, ... through a 5-slot LDS ring of 16-step (16 KiB)
//     chunks by LDS-DMA, four chunks in flight; the ring barrier waits with a counted vmcnt
//     (Sched::win) that leaves the younger DMA groups, the tile stores and V1's beta loads in
//     flight.  The chunk sequence ignores pass boundaries, so a shape with two chunks per pass
//     (64 x 256) streams like the large one.
//   * Stores.  An epilogue row writes its value into the wave's 16 x 16 staging tile (LDS); one
//     step after the block's last row the tile is read back, one step later it leaves as one
//     dwordx4 store per lane.  Every step issues the same VM operations in every pass of its
//     type (a pass that returns nothing stores through an empty buffer range), which is what
//     makes the barrier's count static.
//   * Per-row parameters (V2 / V3, PK_ROW; DLADMM_F_BF16_FUSED_ROWP).  No LDS is left for the
//     fp32 fused kernel's row table, so an epilogue row's values come straight from a.rowp by
//     dword buffer loads into a register ring a few rows deep, each row reloading its own slot
//     for a later row; the loads are counted in Sched::ops1 / ops2 like V1's.  V3 at 256 x 512
//     (kTight) also holds E: a one-row ring, two fragments in rotation, and the lane index formed
//     again at its once-per-pass uses bring it to zero scratch.
#pragma once

#include "dladmm_common.h"
#include "dladmm_internal.h"
#include "dladmm_step.h"

namespace dladmm {

typedef int bi32x4 __attribute__((ext_vector_type(4)));

namespace bf {

constexpr int kSlots = 5;  // LDS ring slots
constexpr int kSPC = 16;   // k-steps (= 1 KiB fragments) per ring chunk
constexpr int kDma = kSPC / kWaves;  // DMA instructions per wave and chunk (one glds16x4)
static_assert(kDma == 4, "one glds16x4 per wave and chunk");

// rows 4g + 0..3 of two consecutive 16-row blocks -> the lane's 8 k-values of one k-step (RNE)
__device__ __forceinline__ bf16x8 cvt8(const float (&a)[4], const float (&b)[4]) {
  bf16x8 v;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[j] = (__bf16)a[j];
    v[4 + j] = (__bf16)b[j];
  }
  return v;
}
__device__ __forceinline__ void pin_agpr_b(bf16x8& b) { asm("" : "+a"(b)); }

// per-row models: epilogue rows (one per KS / 4 steps) that cover 8 steps, the row-table look-ahead
constexpr int rp_depth(int KS) { return KS >= 16 ? 2 : 32 / KS; }

__device__ __forceinline__ void bstore4(rsrc_t r, uint32_t voff, uint32_t soff, f32x4 v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(bi32x4, v), r, (int)voff, (int)soff, 0);
}

// The static schedule of a pass of KS-step blocks.  Block b's accumulator is complete after its
// last step; its epilogue rows run in block b + 1's steps (row r at step (r KS) / 4), its staged
// tiles are read back one step after row 3 and stored one step after that.  "Step" counts on
// past the pass's last MFMA step (the tail runs the same actions without MFMAs).
// PF: V1's per-element beta loads per epilogue row (3), issued one block ahead of the rows.
// RP: the per-row models' (V2 / V3) row-table loads per G2 epilogue row (4 / 5; a G1 row: one,
// theta_z).  The epilogue rows of a pass form one sequence q = 4 b + r; row q, once it has
// consumed its ring slot, reloads the slot for row q + DQ (DQ1 / DQ2: the ring depth of G1 / G2 in
// rows).
template <int MB, int NB, int KS1, int KS2, int PF, int RP = 0, int DQ1 = 0, int DQ2 = 0>
struct Sched {
  static constexpr int ST = NB * KS1;
  static constexpr int row_step(int r, int KS) { return (r * KS) / 4; }
  static constexpr int s3(int KS) { return row_step(3, KS); }
  static constexpr int rows_at(int s, int KS) {
    int c = 0;
    for (int r = 0; r < 4; ++r) c += row_step(r, KS) == s ? 1 : 0;
    return c;
  }
  // block whose tiles are read back / stored at step t (-1: none)
  static constexpr int rb_block(int t, int KS) {
    const int u = t - s3(KS) - 1;
    return (u >= KS && u % KS == 0) ? u / KS - 1 : -1;
  }
  static constexpr int st_block(int t, int KS) { return rb_block(t - 1, KS); }
  // epilogue rows of step t (block t / KS - 1's) that reload their row-table slots: those whose
  // row q + DQ is still a row of the pass
  static constexpr int rp_rows(int t, int KS, int NBLK, int DQ) {
    int c = 0;
    for (int r = 0; r < 4; ++r)
      c += (RP && t / KS >= 1 && row_step(r, KS) == t % KS && 4 * (t / KS - 1) + r + DQ < 4 * NBLK)
               ? 1 : 0;
    return c;
  }
  // VM operations a step body issues (t < ST): G1 the Z tile and the rows' theta_z loads; G2 the
  // E, L, T tiles, the beta loads of block t / KS2 + 1 and the rows' row-table loads
  static constexpr int ops1(int t) {
    return (st_block(t, KS1) >= 0 ? 1 : 0) + rp_rows(t, KS1, NB, DQ1);
  }
  static constexpr int ops2(int t) {
    return (st_block(t, KS2) >= 0 ? 3 : 0) +
           ((PF && t / KS2 + 1 < MB) ? PF * rows_at(t % KS2, KS2) : 0) +
           RP * rp_rows(t, KS2, MB, DQ2);
  }
  // The ring barrier in the head of step T (chunk ch = T / kSPC) waits for chunk ch + 1, whose
  // DMA group went out in the head of step T - (kSlots - 1) kSPC.  Younger than it: the bodies
  // of the (kSlots - 1) kSPC steps since -- walking back across pass boundaries, the pass types
  // alternate -- and the groups of chunks ch + 2 .. ch + kSlots - 1.  What runs between two
  // passes only adds younger operations; the first kSlots - 1 barriers of the kernel wait for
  // chunks the priming already drained.
  template <int T, bool G1>
  static constexpr int win() {
    int n = (kSlots - 2) * kDma, t = T;
    bool g1 = G1;
    for (int i = 0; i < (kSlots - 1) * kSPC; ++i) {
      if (--t < 0) {
        t += ST;
        g1 = !g1;
      }
      n += g1 ? ops1(t) : ops2(t);
    }
    return n < 63 ? n : 63;
  }
};

}  // namespace bf

// LQ: the fused objective's fit term is 0.5 (X - A Z)^2 (LASSO) instead of |X - A Z|
template <int MP, int NP, int EMODE, int PKIND, bool LQ>
__global__ __launch_bounds__(256, 1) void bf16_fused_kernel(const FusedArgs a) {
  using namespace bf;
  constexpr int MB = MP / 16, NB = NP / 16, KS1 = MP / 32, KS2 = NP / 32;
  constexpr int ST = NB * KS1;  // k-steps of either GEMM
  static_assert(ST == MB * KS2, "both GEMMs have MP*NP/512 steps");
  static_assert(MB % 2 == 0 && NB % 2 == 0 && KS1 >= 2, "k-steps cover two 16-row blocks");
  static_assert(ST % kSPC == 0, "whole chunks per pass");
  constexpr int NCH = ST / kSPC;
  // V3 at 256 x 512 (per-row parameters and a resident E): the tightest register budget
  constexpr bool kTight = PKIND == PK_ROW && EMODE == EM_VVAR && MP == 256;
  // fragment register rotation; divides ST: every pass starts at 0
  constexpr int R = kTight ? 2 : 4;
  constexpr int D = R - 1;  // fragment read-ahead (steps)
  static_assert(ST % R == 0 && kSPC >= D + 1, "rotation");
  constexpr int SLOT_F4 = kSPC * 64;
  constexpr int RING_F4 = kSlots * SLOT_F4;
  constexpr int X_F4 = kWaves * MB * 64;
  constexpr int STG_F4 = kWaves * 4 * 64;  // per wave 4 output tiles of 16 x 16 floats
  static_assert((RING_F4 + X_F4 + STG_F4) * 16 <= 160 * 1024, "LDS budget");
  static_assert(PKIND == PK_SCALAR || PKIND == PK_S1 || (PKIND == PK_ELEM && EMODE == EM_V1) ||
                    (PKIND == PK_ROW && (EMODE == EM_V1 || EMODE == EM_VVAR)),
                "bf16 fused path: scalar-parameter variants, V1's per-sample betas, V2 / V3's rows");
  constexpr bool kElem = PKIND == PK_ELEM;
  constexpr bool kRow = PKIND == PK_ROW;
  // per-row models: beta2, beta3, beta1 of the next layer, theta_e, and V3's ss2
  constexpr int RP = kRow ? (EMODE == EM_VVAR ? 5 : 4) : 0;
  // their ring depths in rows: a value is loaded at least 8 steps ahead of its row (V3 at
  // 256 x 512, which also keeps E resident: 4 steps, the depth its registers leave room for)
  constexpr int DQ1 = kRow ? rp_depth(KS1) : 0;
  constexpr int DQ2 = kRow ? ((EMODE == EM_VVAR && MP == 256) ? 1 : rp_depth(KS2)) : 0;
  using S = Sched<MB, NB, KS1, KS2, kElem ? 3 : 0, RP, DQ1, DQ2>;
  static_assert(DQ1 <= 4 * NB && DQ2 <= 4 * MB, "row-table look-ahead within a pass");
  constexpr int S31 = S::s3(KS1), S32 = S::s3(KS2);
  static_assert(S32 + 1 < KS2, "G2: X rows read after the block's last row");
  __shared__ f32x4 smem[RING_F4 + X_F4 + STG_F4];
  f32x4* ring = smem;
  f32x4* xs = smem + RING_F4;  // xs[w][b][lane] = X rows 16b+4g+0..3 of this lane's column

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, g = lane >> 4;
  const int64_t c0 = (int64_t)blockIdx.x * kTileCols + w * 16;
  const int64_t col = c0 + j;
  const bool cv = col < a.B;
  const int m = a.m, n = a.n, K = a.K;
  const bool lossz = a.loss_kind != 0;
  // dword form: rows 4g.. of the lane's column; 16-B form: row l >> 2, columns 4 (l & 3) .. +3 of
  // the wave's 16 (the plan routes a batch that is no multiple of 4 or unaligned rows to path 3,
  // so a lane's 4 columns are all valid or all padding)
  auto lane_off = [&](int64_t ld) -> uint32_t {
    return cv ? (uint32_t)((col + (int64_t)(4 * g) * ld) * 4) : kOOB;
  };
  auto off4 = [&](int64_t ld) -> uint32_t {
    const int64_t c4 = c0 + 4 * (lane & 3);
    return c4 < a.B ? (uint32_t)(((lane >> 2) * ld + c4) * 4) : kOOB;
  };

  float Er[MB][4], Lr[MB][4], Zr[NB][4];
  bf16x8 Vpk[KS1], Zpk[KS2];
  float regsum = 0.f, fit = 0.f;

  // ---------------------------------------------------------------- staging tiles and stores
  f32x4* stg = smem + RING_F4 + X_F4 + w * 4 * 64;
  auto stage = [&](int tile, int r, float v) {
    reinterpret_cast<float*>(stg + tile * 64)[(4 * g + r) * 16 + j] = v;
  };
  f32x4 pst[3];
  uint32_t pso = 0u;

  // ---------------------------------------------------------------- weight stream
  // GEMM gi: 0 = prologue A, 2k+1 = -W_k, 2k+2 = A; past the last GEMM, A again as filler.
  const int64_t wl = (int64_t)ST * kFrag;  // floats per packed tensor: ST fragments of 1 KiB
  auto gsrc = [&](int gi) -> const float* {
    const int kk = gi >> 1;
    return ((gi & 1) && kk < K) ? a.Wp + (int64_t)(kk * a.wstep) * wl : a.Ap;
  };
  // DMA group of chunk CH (relative to pass gi; CH >= NCH: a later pass) into `slot`: wave w
  // moves fragments 4w .. 4w+3
  auto issue = [&](auto CH_, int gi, int slot) {
    constexpr int CH = decltype(CH_)::value;
    uint64_t sb = (uint64_t)gsrc(gi + CH / NCH);
    asm volatile("" : "+s"(sb));
    const float* base = (const float*)sb + (int64_t)(CH % NCH) * kSPC * kFrag;
    glds16x4(base + 4 * w * kFrag, lane * 16, ring + slot * SLOT_F4 + 4 * w * 64);
  };
  auto slot_add = [](int s, int d) -> int { s += d; return s >= kSlots ? s - kSlots : s; };
  int cur = 0;
  auto frag = [&](int slot, int f) -> bf16x8 {
    return __builtin_bit_cast(bf16x8, ring[slot * SLOT_F4 + f * 64 + lane]);
  };

  // ---------------------------------------------------------------- parameters
  auto layer_params = [&](int k) -> LayerP {
    const int kk = k < 0 ? 0 : k;
    const int kn = k < 0 ? 0 : (k + 1 < K ? k + 1 : k);
    cfloat_p sp = (cfloat_p)a.scal + kk * DLADMM_NSCALAR;
    return dladmm::layer_params_at<EMODE, PKIND>(sp, sp, (cfloat_p)a.scal + kn * DLADMM_NSCALAR);
  };

  // ---------------------------------------------------------------- initial state
  const uint32_t oo4 = off4(a.ldo);
  {
    const rsrc_t re = mkrsrc(a.E0, (uint32_t)(m * a.lde0 * 4));
    const rsrc_t rl = mkrsrc(a.L0, (uint32_t)(m * a.ldl0 * 4));
    const rsrc_t rx = mkrsrc(a.X, (uint32_t)(m * a.ldx * 4));
    const uint32_t oe = lane_off(a.lde0), ol = lane_off(a.ldl0), ox = lane_off(a.ldx);
#pragma unroll
    for (int b = 0; b < MB; ++b) {
      f32x4 xv;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        xv[r] = bload(rx, ox + (uint32_t)((16 * b + r) * a.ldx * 4));
        Er[b][r] = bload(re, oe + (uint32_t)((16 * b + r) * a.lde0 * 4));
        Lr[b][r] = bload(rl, ol + (uint32_t)((16 * b + r) * a.ldl0 * 4));
      }
      xs[(w * MB + b) * 64 + lane] = xv;  // read back only by this wave
      __builtin_amdgcn_sched_barrier(0);
    }
    // Z0: fp32 into the resident registers, bf16 into the prologue's B operand
    const rsrc_t rz = mkrsrc(a.Z0, (uint32_t)(n * a.ldz0 * 4));
    const uint32_t oz0 = lane_off(a.ldz0);
#pragma unroll
    for (int s = 0; s < KS2; ++s) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        Zr[2 * s][r] = bload(rz, oz0 + (uint32_t)((32 * s + r) * a.ldz0 * 4));
        Zr[2 * s + 1][r] = bload(rz, oz0 + (uint32_t)((32 * s + 16 + r) * a.ldz0 * 4));
      }
      Zpk[s] = cvt8(Zr[2 * s], Zr[2 * s + 1]);
      pin_agpr_b(Zpk[s]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        pin_agpr(Zr[2 * s][r]);
        pin_agpr(Zr[2 * s + 1][r]);
      }
      if (s % 2 == 1) __builtin_amdgcn_sched_barrier(0);  // at most 16 loads in flight
    }
  }

  const uint32_t mbytes = (uint32_t)(m * a.ldo * 4);
  SWalk zw{0u, (uint32_t)(a.ldo * 4)}, mw{0u, (uint32_t)(a.ldo * 4)};

  // ---------------------------------------------------------------- per-row parameters (V2 / V3)
  // Layer k's slot s of a.rowp ([K][8][rstride]) holds one value per row.  They travel as V1's
  // per-sample betas do: one dword load per row and parameter straight into a register ring (no
  // LDS: the weight ring, the X rows and the tiles fill it) -- G2's pr[q % DQ2][p], G1's
  // pz[q % DQ1] for row q = 4 b + r of the pass; the two rings are never live together.  An
  // epilogue row reloads its own slot for row q + DQ right after reading it, so the ring is DQ
  // rows deep and needs no slot beside those in use.  Each slot has a resource of its
  // own that ends at the slot's true length (m; n for theta_z), so the rows of the padding read 0
  // -- and stay exactly 0: with Z = q = 0, S(0, th) = 0 for every th; E = S(0 - ss2 0, th) = 0,
  // T = 0, L = 0 + b3 0, Var = 0 (dladmm_step.h).  The empty asm after a row's loads keeps the
  // compiler from merging the loads of two rows (adjacent dwords) into one: the ring barrier's
  // count (Sched::ops1 / ops2) is per load.
  enum { RP_B2 = 0, RP_B3 = 1, RP_B1N = 2, RP_THE = 3, RP_SS2 = 4 };
  const uint32_t vrow = (uint32_t)(16 * g);
  auto row_rsrc = [&](int k, int slot, int rows) -> rsrc_t {
    return mkrsrc(a.rowp + ((int64_t)k * DLADMM_NSCALAR + slot) * a.rstride, (uint32_t)(rows * 4));
  };
  float pz[kRow ? DQ1 : 1];
  float pr[kRow ? DQ2 : 1][kRow ? RP : 1];
  rsrc_t rrz = mkrsrc(nullptr, 0u);
  rsrc_t rrp[kRow ? RP : 1];
  // row q of the pass, if the pass has it
  auto rp_row1 = [&](auto Q_) {
    constexpr int q = decltype(Q_)::value;
    if constexpr (kRow && q < 4 * NB) {
      pz[q % DQ1] = bload(rrz, vrow + (uint32_t)(64 * (q / 4) + 4 * (q % 4)));
      asm volatile("");
    }
  };
  auto rp_row2 = [&](auto Q_) {
    constexpr int q = decltype(Q_)::value;
    if constexpr (kRow && q < 4 * MB) {
      static_for<RP>([&](auto P_) {
        constexpr int p = decltype(P_)::value;
        pr[q % DQ2][p] = bload(rrp[p], vrow + (uint32_t)(64 * (q / 4) + 4 * (q % 4)));
      });
      asm volatile("");
    }
  };

  // ---------------------------------------------------------------- epilogue rows
  // G1 block b, row r of layer k: Z_k = S(Z_{k-1} + [s1] q, theta_z), q = -W_k Var (the packed
  // weights are negated), on the resident fp32 Z (main_lena.py:86)
  auto epi1_row = [&](const LayerP& P, int b, int r, float q) {
    const float z = z_step<PKIND>(Zr[b][r], q, P.s1, [&]() -> ShrinkP {
      if constexpr (kRow) return shrink_params(pz[(4 * b + r) % DQ1]);
      else return P.thz;
    });
    Zr[b][r] = z;
    pin_agpr(Zr[b][r]);
    stage(0, r, z);
    regsum += fabsf(z);
    // materialise the running sum here: left alone the scheduler sinks the chain below the pass
    asm volatile("" : "+v"(regsum));
  };
  // V1 (PK_ELEM): beta1_k, beta2_k and beta1_{k+1} of a G2 block's rows, loaded one block ahead of
  // the block whose steps run the rows (two ahead of the rows) into a 3-block register ring
  float pb[kElem ? 3 : 1][3][4];
  float vn[2][4];  // Var_{k+1} of the current block pair, rounded into Vpk when complete
  auto epi2_row = [&](const LayerP& P, bool pro, int b, int r, float Pv, float x) {
    float b2 = P.b2, b3 = P.b3, b1n = P.b1n;
    if constexpr (kElem) {
      b3 = pb[b % 3][0][r];
      b2 = pb[b % 3][1][r];
      b1n = pb[b % 3][2][r];
    } else if constexpr (kRow) {
      // every value counts as used, also in the prologue, whose rows need beta1 only: a load the
      // compiler dropped there would be missing from the ring barrier's count
#pragma unroll
      for (int p = 0; p < RP; ++p) asm volatile("" : "+v"(pr[(4 * b + r) % DQ2][p]));
      b2 = pr[(4 * b + r) % DQ2][RP_B2];
      b3 = pr[(4 * b + r) % DQ2][RP_B3];
      b1n = pr[(4 * b + r) % DQ2][RP_B1N];
    }
    // per-row step and threshold: a float threshold takes the literal shrink form (dladmm_step.h)
    const StepOut s = el_step<EMODE>(
        Pv, x, Er[b][r], Lr[b][r], b2, b3, P.ss2b, pro,
        [&] {
          if constexpr (kRow && EMODE == EM_VVAR) return pr[(4 * b + r) % DQ2][RP_SS2];
          else return P.ss2;
        },
        [&] {
          if constexpr (kRow) return pr[(4 * b + r) % DQ2][RP_THE];
          else return P.the;
        });
    Er[b][r] = s.e;
    Lr[b][r] = s.l;
    stage(1, r, s.e);
    stage(2, r, s.l);
    stage(3, r, s.t);
    const float res = x - Pv;
    if constexpr (LQ) fit = __builtin_fmaf(res, res, fit);
    else fit += fabsf(res);
    asm volatile("" : "+v"(fit));
    vn[b & 1][r] = s.var(b1n);  // Var of the next layer (main_lena.py:85)
  };
  // kTight: the lane index formed again where a once-per-pass action needs it (the volatile asm
  // keeps it from being hoisted), so that no lane-derived address lives across the passes
  auto lane_here = [&]() -> int {
    if constexpr (kTight) {
      int z = 0;
      asm volatile("" : "+v"(z));
      return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, (unsigned)z));
    } else {
      return lane;
    }
  };
  // col_sum (dladmm_common.h) with the lane index passed in: the same two exchanges and adds
  auto col_sum_at = [&](float v, int ln) -> float {
    if constexpr (kTight) {
      v += __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((ln ^ 16) << 2, __builtin_bit_cast(int, v)));
      v += __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute((ln ^ 32) << 2, __builtin_bit_cast(int, v)));
      return v;
    } else {
      return col_sum(v);
    }
  };
  auto flush_loss = [&](int k) {
    if (lossz && k >= 0) {
      const int ln = lane_here();
      const float rs = col_sum_at(regsum, ln);
      const float fs = LQ ? 0.5f * col_sum_at(fit, ln) : col_sum_at(fit, ln);
      if (g == 0) {
        a.lossp[(int64_t)(2 * k + 0) * a.ldl + col] = rs;
        a.lossp[(int64_t)(2 * k + 1) * a.ldl + col] = fs;
      }
    }
    regsum = 0.f;
    fit = 0.f;
  };

  // ---------------------------------------------------------------- ring steps
  // Head of step t: the fragment of step t + D into the rotation; at chunk position kSPC - D
  // first the ring barrier (chunk ch + 1 landed, every wave done with chunk ch) and the DMA group
  // of chunk ch + kSlots into the freed slot.
  bf16x8 fr[R];
  auto step_head = [&](auto G1_, auto T_, int gi) {
    constexpr bool G1 = decltype(G1_)::value;
    constexpr int t = decltype(T_)::value;
    constexpr int c = t % kSPC, ch = t / kSPC, tn = t + D;
    if constexpr (c + D < kSPC) {
      fr[tn % R] = frag(cur, c + D);
    } else {
      if constexpr (c + D == kSPC) {
        ring_barrier_cnt<S::template win<t, G1>()>();
        issue(std::integral_constant<int, ch + kSlots>{}, gi, cur);
      }
      fr[tn % R] = frag(slot_add(cur, 1), c + D - kSPC);
    }
  };
  auto step_tail = [&](auto T_) {
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (decltype(T_)::value % kSPC == kSPC - 1) cur = slot_add(cur, 1);
  };

  // prime the ring: chunks 0 .. kSlots-1 of the stream, all landed before the first step
  static_for<kSlots>([&](auto C_) { issue(C_, 0, decltype(C_)::value); });
  ring_barrier_cnt<0>();
#pragma unroll
  for (int t = 0; t < D; ++t) fr[t] = frag(0, t);

  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  // ---------------------------------------------------------------- G1(k): -W_k Var -> Z_k
  f32x4 qp = zero4;
  auto g1_acts = [&](auto T_, const LayerP& P, rsrc_t rzo) {
    constexpr int t = decltype(T_)::value;
    constexpr int ib = t / KS1 - 1, s = t % KS1;
    // read-back first: at KS1 = 2 the next block's rows 0, 1 are staged in this very step
    if constexpr (S::rb_block(t, KS1) >= 0 && S::rb_block(t, KS1) < NB) {
      pst[0] = stg[lane];
      pso = zw.at(0);
      zw.next();
    }
    if constexpr (S::st_block(t, KS1) >= 0 && S::st_block(t, KS1) < NB)
      bstore4(rzo, oo4, pso, pst[0]);
    if constexpr (ib >= 0 && ib < NB) {
      static_for<4>([&](auto R_) {
        constexpr int r = decltype(R_)::value;
        if constexpr (S::row_step(r, KS1) == s) {
          epi1_row(P, ib, r, qp[r]);
          rp_row1(std::integral_constant<int, 4 * ib + r + DQ1>{});
        }
      });
      // blocks ib - 1, ib complete: the B operand of G2's k-step ib / 2
      if constexpr ((ib & 1) && s == S31) {
        Zpk[ib / 2] = cvt8(Zr[ib - 1], Zr[ib]);
        pin_agpr_b(Zpk[ib / 2]);
      }
    }
  };
  auto g1_pass = [&](int k, const LayerP& P, rsrc_t rzo) {
    const int gi = 2 * k + 1;
    zw.reset();
    if constexpr (kRow) {
      rrz = row_rsrc(k, DLADMM_P_THETA_Z, n);
      // the first DQ1 rows' thresholds, ahead of the pass (younger than every group waited for)
      static_for<DQ1>([&](auto Q_) { rp_row1(Q_); });
    }
    static_for<NB>([&](auto IB_) {
      constexpr int ib = decltype(IB_)::value;
      f32x4 acc = zero4;
      static_for<KS1>([&](auto S_) {
        constexpr int s = decltype(S_)::value;
        constexpr int t = ib * KS1 + s;
        step_head(std::true_type{}, std::integral_constant<int, t>{}, gi);
        g1_acts(std::integral_constant<int, t>{}, P, rzo);
        acc = mfma_bf16(fr[t % R], Vpk[s], acc);
        step_tail(std::integral_constant<int, t>{});
      });
      qp = acc;
    });
    // tail: the last block's rows, the last two tiles
    static_for<KS1 + 2>([&](auto I_) {
      g1_acts(std::integral_constant<int, ST + decltype(I_)::value>{}, P, rzo);
    });
  };

  // ---------------------------------------------------------------- G2(k): A Z_k -> E, L, T, Var
  const uint32_t vb = lane_off(a.ldb);
  rsrc_t rb1 = mkrsrc(nullptr, 0u), rb2 = rb1, rbn = rb1;
  SWalk bw{0u, (uint32_t)(a.ldb * 4)};
  auto pf_row = [&](auto B_, auto R_) {
    constexpr int bb = decltype(B_)::value, rr = decltype(R_)::value;
    if constexpr (kElem) {
      const int so = (int)bw.at(rr);
      pb[bb % 3][0][rr] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rb1, (int)vb, so, 0));
      pb[bb % 3][1][rr] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rb2, (int)vb, so, 0));
      pb[bb % 3][2][rr] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rbn, (int)vb, so, 0));
      if constexpr (rr == 3) bw.next();
    }
  };
  struct OutR { rsrc_t e, l, t; };
  f32x4 xv;
  auto g2_acts = [&](auto T_, auto PRO_, const LayerP& P, const OutR& O) {
    constexpr int t = decltype(T_)::value;
    constexpr bool PRO = decltype(PRO_)::value;
    constexpr int ib = t / KS2 - 1, s = t % KS2;
    if constexpr (S::rb_block(t, KS2) >= 0 && S::rb_block(t, KS2) < MB) {
      pst[0] = stg[64 + lane];
      pst[1] = stg[128 + lane];
      pst[2] = stg[192 + lane];
      pso = mw.at(0);
      mw.next();
    }
    if constexpr (S::st_block(t, KS2) >= 0 && S::st_block(t, KS2) < MB) {
      bstore4(O.e, oo4, pso, pst[0]);
      bstore4(O.l, oo4, pso, pst[1]);
      bstore4(O.t, oo4, pso, pst[2]);
    }
    if constexpr (ib >= 0 && ib < MB) {
      static_for<4>([&](auto R_) {
        constexpr int r = decltype(R_)::value;
        if constexpr (S::row_step(r, KS2) == s) {
          epi2_row(P, PRO, ib, r, qp[r], xv[r]);
          rp_row2(std::integral_constant<int, 4 * ib + r + DQ2>{});
        }
      });
      if constexpr ((ib & 1) && s == S32) {
        Vpk[ib / 2] = cvt8(vn[0], vn[1]);
        pin_agpr_b(Vpk[ib / 2]);
      }
    }
    // X rows of block ib + 1 (its rows run in the next block's steps), once row 3 has used xv
    if constexpr (s == S32 + 1 && ib + 1 >= 0 && ib + 1 < MB)
      xv = xs[(w * MB + ib + 1) * 64 + lane_here()];
  };
  auto g2_pass = [&](auto PRO_, int k, const LayerP& P, const OutR& O) {
    constexpr bool PRO = decltype(PRO_)::value;
    const int gi = 2 * k + 2;
    mw.reset();
    if constexpr (kElem) {
      // beta1_k, beta2_k, beta1_{k+1} (the prologue: beta1_0 for Var_0 only), from the device
      // tables by scalar loads; then block 0's rows, ahead of the pass
      typedef const float* const __attribute__((address_space(4)))* ctab_p;
      const ctab_p t1 = (ctab_p)a.b1t, t2 = (ctab_p)a.b2t;
      const uint32_t eb = (uint32_t)(m * a.ldb * 4);
      const int kn = k + 1;
      rb1 = mkrsrc(PRO ? nullptr : t1[k < 0 ? 0 : k], PRO ? 0u : eb);
      rb2 = mkrsrc(PRO ? nullptr : t2[k < 0 ? 0 : k], PRO ? 0u : eb);
      rbn = mkrsrc(kn < K ? t1[kn] : nullptr, kn < K ? eb : 0u);
      bw.reset();
      static_for<4>([&](auto R_) { pf_row(std::integral_constant<int, 0>{}, R_); });
    }
    if constexpr (kRow) {
      // layer k's slots (the prologue: layer 0's, used for Var_0 only) and beta1 of layer k + 1,
      // clamped at the last layer: that load is issued all the same, its Var feeds nothing
      const int kk = k < 0 ? 0 : k;
      const int kn = k < 0 ? 0 : (k + 1 < K ? k + 1 : k);
      rrp[RP_B2] = row_rsrc(kk, DLADMM_P_BETA2, m);
      rrp[RP_B3] = row_rsrc(kk, DLADMM_P_BETA3, m);  // V2's table holds beta1 there
      rrp[RP_B1N] = row_rsrc(kn, DLADMM_P_BETA1, m);
      rrp[RP_THE] = row_rsrc(kk, DLADMM_P_THETA_E, m);
      if constexpr (RP > RP_SS2) rrp[RP_SS2] = row_rsrc(kk, DLADMM_P_SS2, m);
      static_for<DQ2>([&](auto Q_) { rp_row2(Q_); });
    }
    xv = xs[(w * MB) * 64 + lane_here()];
    static_for<MB>([&](auto IB_) {
      constexpr int ib = decltype(IB_)::value;
      f32x4 acc = zero4;
      static_for<KS2>([&](auto S_) {
        constexpr int s = decltype(S_)::value;
        constexpr int t = ib * KS2 + s;
        step_head(std::false_type{}, std::integral_constant<int, t>{}, gi);
        // V1: block ib + 1's betas, one row per epilogue-row step
        if constexpr (kElem && ib + 1 < MB) {
          static_for<4>([&](auto R_) {
            if constexpr (S::row_step(decltype(R_)::value, KS2) == s)
              pf_row(std::integral_constant<int, ib + 1>{}, R_);
          });
        }
        g2_acts(std::integral_constant<int, t>{}, PRO_, P, O);
        acc = mfma_bf16(fr[t % R], Zpk[s], acc);
        step_tail(std::integral_constant<int, t>{});
      });
      qp = acc;
    });
    static_for<KS2 + 2>([&](auto I_) {
      g2_acts(std::integral_constant<int, ST + decltype(I_)::value>{}, PRO_, P, O);
    });
  };

  // ---------------------------------------------------------------- prologue + K layers
  const rsrc_t none = mkrsrc(nullptr, 0u);
  {
    const LayerP P0 = layer_params(-1);
    const OutR O0{none, none,
                  mkrsrc(a.keep_all ? a.To : nullptr, (a.keep_all && a.To) ? mbytes : 0u)};
    g2_pass(std::true_type{}, -1, P0, O0);
  }
  flush_loss(-1);
  for (int k = 0; k < K; ++k) {
    const bool st = a.keep_all || k == K - 1;
    const int ko = a.keep_all ? k : 0;
    const LayerP P = layer_params(k);
    // a layer that is not returned (lean mode) stores through an empty range
    g1_pass(k, P, mkrsrc(a.Zo + (int64_t)ko * n * a.ldo, st ? (uint32_t)(n * a.ldo * 4) : 0u));
    const OutR O{mkrsrc(a.Eo + (int64_t)ko * m * a.ldo, st ? mbytes : 0u),
                 mkrsrc(a.Lo + (int64_t)ko * m * a.ldo, st ? mbytes : 0u),
                 mkrsrc(a.To ? a.To + (int64_t)(a.keep_all ? k + 1 : 0) * m * a.ldo : nullptr,
                        (a.To && st) ? mbytes : 0u)};
    g2_pass(std::false_type{}, k, P, O);
    flush_loss(k);
  }
  // drain: the ring's last LDS-DMAs must land before the workgroup's LDS is released
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

template <int MP, int NP, int EM, int PK>
hipError_t launch_bf16(const FusedArgs& a, int grid, hipStream_t s) {
  if (a.loss_kind == DLADMM_LOSS_LASSO)
    hipLaunchKernelGGL((bf16_fused_kernel<MP, NP, EM, PK, true>), dim3(grid), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((bf16_fused_kernel<MP, NP, EM, PK, false>), dim3(grid), dim3(256), 0, s, a);
  return hipGetLastError();
}

template <int MP, int NP>
hipError_t dispatch_bf16_variant(int variant, const FusedArgs& a, int grid, hipStream_t s) {
  switch (variant) {
    case DLADMM_V4_SCALAR: return launch_bf16<MP, NP, EM_VVAR, PK_SCALAR>(a, grid, s);
    case DLADMM_V5_TIED: return launch_bf16<MP, NP, EM_VVAR, PK_S1>(a, grid, s);
    case DLADMM_V6_LASSO: return launch_bf16<MP, NP, EM_LASSO, PK_SCALAR>(a, grid, s);
    case DLADMM_V1_LENA: return launch_bf16<MP, NP, EM_V1, PK_ELEM>(a, grid, s);
    case DLADMM_V2_LTHETA: return launch_bf16<MP, NP, EM_V1, PK_ROW>(a, grid, s);
    case DLADMM_V3_FULL: return launch_bf16<MP, NP, EM_VVAR, PK_ROW>(a, grid, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace dladmm
