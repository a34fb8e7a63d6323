// dladmm_elemloss.hip -- the element-wise training terms of the supervised and reweighted scripts
// over a forward's stacked outputs, every layer in ONE streaming launch, fp32 in, fp64 sums:
//   square   (main_syn_gt.py:243-248, main_syn_gt_ltheta.py:243-246, --loss-fn gt of the
//            *_newS_layerwise.py scripts)   sum (Z_k - Zref)^2, sum (E_k - Eref)^2
//   absolute (main_syn_l1l1_rw_ltheta.py:236-238)   sum |Z_k - Zref|, sum |E_k - Eref|
// per layer and column, and, in the adjoint form, the cotangent seeds 2 w[k] (V_k - Vref) /
// w[k] sgn(V_k - Vref) that dladmm_bwd_f32 takes as gZ / gE.  The C entry points
// (dladmm_elemloss_f32, dladmm_elemloss_workspace_bytes) are at the end of this file.
//
// Geometry.  The rows of Z (n, padded to a multiple of 4) and of E (m) form one virtual row
// space; a workgroup of four waves owns a column tile and a slab of it, grid = (column tiles,
// slabs).  Two tiles, chosen by the batch on the host (kElWideBatch):
//   narrow  16 columns; a wave access covers 4 rows x 16 columns (lane = 16 g + c), NR = 2
//           accesses per wave and layer: slabs of 32 rows, so that the scripts' B = 20 (two
//           column tiles) still gives 2 x 24 workgroups at 250 x 500;
//   wide    64 columns; a wave access is one row's full 256-byte segment, NR = 16 accesses per
//           wave and layer: slabs of 64 rows.
// A lane keeps the NR reference elements of its rows in registers for the whole call: they are
// read once, and the K layers stream past them.  Layer k + 1's NR rows are requested before layer
// k's are consumed, so a wave has 2 NR row accesses in flight; the one-past-the-end request goes
// to a zero-size view.  Every operand is a buffer view with the row's uniform part in soffset:
// a NULL operand, an unwanted layer's cotangents, rows past n / m and columns past B all fall
// outside their view (loads give 0, stores are dropped), so the body has no branch.  A row
// access is a Z or an E access as a whole (n is padded to the 4 rows of a narrow access): base,
// size and stride are selected on the scalar unit.  Cotangent stores are non-temporal.
//
// Reduction, fp64, fixed order: the lane's rows in order (the difference in fp32 as the
// reference forms it, its square or modulus accumulated in fp64), the narrow tile's four lane
// groups by an xor tree, the four waves in order through LDS (two pads alternate: one barrier
// per layer), then the slabs in order in a second small launch that also forms the totals.  No
// atomics; nothing is zeroed.
#include "dladmm_elemloss.h"

#include "dladmm.h"
#include "dladmm_common.h"

namespace dladmm {

namespace {

constexpr int kElWaves = 4;

__device__ __forceinline__ float bload_s(rsrc_t r, uint32_t voff, uint32_t soff) {
  return __builtin_bit_cast(float,
                            __builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, (int)soff, 0));
}

}  // namespace

template <int CT, int NR, bool ABSF, bool GRAD>
__global__ __launch_bounds__(256) void elemloss_fused_kernel(const ElemLossArgs a) {
  constexpr int RW = 64 / CT;              // rows of one wave access
  constexpr int SR = kElWaves * NR * RW;   // rows of a slab
  static_assert(SR <= kElMaxSlabRows, "the host validates offsets over kElMaxSlabRows");
  __shared__ double red[2][kElWaves][2][CT];

  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = lane % CT, g = lane / CT;
  const int64_t col = (int64_t)blockIdx.x * CT + c;
  const bool cv = col < a.B;
  auto lane_off = [&](int64_t ld) -> uint32_t {
    return cv ? (uint32_t)((col + (int64_t)g * ld) * 4) : kOOB;
  };
  const uint32_t vz = lane_off(a.ldz), ve = lane_off(a.lde), vg = lane_off(a.ldg);

  // this wave's NR accesses: which operand, and the row of the access's first lane group in it
  const int row0 = (int)blockIdx.y * SR + w * (NR * RW);
  bool isz[NR];
  uint32_t rr[NR];
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    const int rb = row0 + i * RW;
    isz[i] = rb < a.n4;
    rr[i] = (uint32_t)(isz[i] ? rb : rb - a.n4);
  }

  float ref[NR];
  {
    const uint32_t vzr = lane_off(a.ldzr), ver = lane_off(a.lder);
#pragma unroll
    for (int i = 0; i < NR; ++i)
      ref[i] = bload_s(mkrsrc(isz[i] ? a.Zref : a.Eref, isz[i] ? a.zrbytes : a.erbytes),
                       isz[i] ? vzr : ver, rr[i] * (uint32_t)((isz[i] ? a.ldzr : a.lder) * 4));
  }

  // layer k's rows; k == k1 (the request past the last layer) reads zero-size views
  auto issue = [&](int k, float (&v)[NR]) {
    const bool live = k < a.k1;
    const float* pz = a.Z + (int64_t)k * a.zls;
    const float* pe = a.E + (int64_t)k * a.els;
    const uint32_t bz = live ? a.zbytes : 0u, be = live ? a.ebytes : 0u;
#pragma unroll
    for (int i = 0; i < NR; ++i)
      v[i] = bload_s(mkrsrc(isz[i] ? pz : pe, isz[i] ? bz : be), isz[i] ? vz : ve,
                     rr[i] * (uint32_t)((isz[i] ? a.ldz : a.lde) * 4));
  };

  float nxt[NR];
  issue(a.k0, nxt);
  for (int k = a.k0; k < a.k1; ++k) {
    float cur[NR];
#pragma unroll
    for (int i = 0; i < NR; ++i) cur[i] = nxt[i];
    issue(k + 1, nxt);

    float cw = 0.f;
    float *pgz = nullptr, *pge = nullptr;
    uint32_t bgz = 0u, bge = 0u;
    if constexpr (GRAD) {
      const float wk = ((cfloat_p)a.w)[k];
      cw = ABSF ? wk : 2.0f * wk;
      const bool wanted = (a.want >> (k - a.k0)) & 1u;
      pgz = a.gZ + (int64_t)k * a.gzls;
      pge = a.gE + (int64_t)k * a.gels;
      bgz = wanted ? a.gzbytes : 0u;
      bge = wanted ? a.gebytes : 0u;
    }
    double sz = 0.0, se = 0.0;
#pragma unroll
    for (int i = 0; i < NR; ++i) {
      const float d = cur[i] - ref[i];   // fp32, as the reference's subtraction
      const double t = ABSF ? (double)__builtin_fabsf(d) : (double)d * (double)d;
      sz += isz[i] ? t : 0.0;
      se += isz[i] ? 0.0 : t;
      if constexpr (GRAD) {
        // torch.abs differentiates to sgn with sgn(0) = 0
        const float gv = ABSF ? (d > 0.0f ? cw : (d < 0.0f ? -cw : 0.0f)) : cw * d;
        bstore_s(mkrsrc(isz[i] ? pgz : pge, isz[i] ? bgz : bge), vg,
                 rr[i] * (uint32_t)(a.ldg * 4), gv);
      }
    }
    // fixed order: the lane groups that share a column, then the four waves in order
#pragma unroll
    for (int o = CT; o < 64; o <<= 1) {
      sz += __shfl_xor(sz, o, 64);
      se += __shfl_xor(se, o, 64);
    }
    const int buf = (k - a.k0) & 1;
    if (g == 0) {
      red[buf][w][0][c] = sz;
      red[buf][w][1][c] = se;
    }
    __syncthreads();  // pad buf is complete; pad buf ^ 1 was read before the previous barrier
    if (w < 2 && g == 0 && cv) {
      double tn = red[buf][0][w][c];
#pragma unroll
      for (int q = 1; q < kElWaves; ++q) tn += red[buf][q][w][c];
      a.part[(((int64_t)blockIdx.y * a.K + k) * 2 + w) * a.B + col] = tn;
    }
  }
}

namespace {

// thread values -> one sum: the wave's xor tree, then the four waves in order
__device__ __forceinline__ double block_sum(double s, double* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

}  // namespace

// grid (ceil(B / 256), 2 K): the slabs in order; with one column block also the total
__global__ __launch_bounds__(256) void elemloss_colsum_kernel(const double* part, int slabs,
                                                              int K2, int B, double* colsum,
                                                              double* total) {
  __shared__ double sh[4];
  const int kt = blockIdx.y;
  const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double s = 0.0;
  if (col < B) {
    for (int sl = 0; sl < slabs; ++sl) s += part[((int64_t)sl * K2 + kt) * B + col];
    colsum[(int64_t)kt * B + col] = s;
  }
  if (total && gridDim.x == 1) {
    const double t = block_sum(s, sh);
    if (threadIdx.x == 0) total[kt] = t;
  }
}

// grid 2 K: thread t sums the columns t, t + 256, ... in order (B > 256)
__global__ __launch_bounds__(256) void elemloss_total_kernel(const double* colsum, int B,
                                                             double* total) {
  __shared__ double sh[4];
  const int kt = blockIdx.x;
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < B; i += 256) s += colsum[(int64_t)kt * B + i];
  const double t = block_sum(s, sh);
  if (threadIdx.x == 0) total[kt] = t;
}

template <int CT, int NR>
static hipError_t launch_tile(const ElemLossArgs& a, bool absf, bool grad, dim3 grid,
                              hipStream_t s) {
  if (absf && grad)
    hipLaunchKernelGGL((elemloss_fused_kernel<CT, NR, true, true>), grid, dim3(256), 0, s, a);
  else if (absf)
    hipLaunchKernelGGL((elemloss_fused_kernel<CT, NR, true, false>), grid, dim3(256), 0, s, a);
  else if (grad)
    hipLaunchKernelGGL((elemloss_fused_kernel<CT, NR, false, true>), grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((elemloss_fused_kernel<CT, NR, false, false>), grid, dim3(256), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_elemloss(const ElemLossArgs& a, bool wide, bool absf, bool grad, dim3 grid,
                           hipStream_t s) {
  return wide ? launch_tile<kElWideCT, kElWideNR>(a, absf, grad, grid, s)
              : launch_tile<kElNarrowCT, kElNarrowNR>(a, absf, grad, grid, s);
}

hipError_t launch_elemloss_finish(const double* part, int slabs, int K2, int B, double* colsum,
                                  double* total, hipStream_t s) {
  const int cb = (B + 255) / 256;
  hipLaunchKernelGGL(elemloss_colsum_kernel, dim3((unsigned)cb, (unsigned)K2), dim3(256), 0, s,
                     part, slabs, K2, B, colsum, total);
  if (hipError_t e = hipGetLastError()) return e;
  if (total && cb > 1) {
    hipLaunchKernelGGL(elemloss_total_kernel, dim3((unsigned)K2), dim3(256), 0, s,
                       (const double*)colsum, B, total);
    return hipGetLastError();
  }
  return hipSuccess;
}

namespace {

struct ElPlan {
  bool wide;
  int n4, slabs, ctiles;
  size_t bytes;
};

// shape checks and the tile; `sizing`: only what the workspace size depends on
int el_plan(const dladmm_elemloss_desc* d, ElPlan* p, bool sizing) {
  if (!d) return DLADMM_E_NULL;
  if (d->abi_version != DLADMM_ABI_VERSION) return DLADMM_E_ABI_VERSION;
  if (d->m < 1 || d->n < 1 || d->batch < 1) return DLADMM_E_SHAPE;
  if (d->layers < 1 || d->layers > DLADMM_MAX_LAYERS) return DLADMM_E_LAYERS;
  if ((d->power != 1 && d->power != 2) || (d->mode != 0 && d->mode != 1))
    return DLADMM_E_UNSUPPORTED;
  if (!d->Z && !d->E) return DLADMM_E_NULL;
  const int64_t B = d->batch;
  if (!sizing) {
    const int64_t lds[] = {d->ld_z, d->ld_e, d->ld_zref, d->ld_eref, d->ld_g,
                           d->z_layer_stride, d->e_layer_stride, d->gz_layer_stride,
                           d->ge_layer_stride};
    for (int64_t v : lds)
      if (v < 0) return DLADMM_E_SHAPE;
    if ((d->Z && d->ld_z < B) || (d->E && d->ld_e < B) || (d->Z && d->Zref && d->ld_zref < B) ||
        (d->E && d->Eref && d->ld_eref < B))
      return DLADMM_E_SHAPE;
    if (!d->colsum) return DLADMM_E_NULL;
    if (d->mode == 1) {
      if (!d->w || (d->Z && !d->gZ) || (d->E && !d->gE)) return DLADMM_E_NULL;
      if (d->ld_g < B) return DLADMM_E_SHAPE;
    }
    // 32-bit buffer offsets over a slab's padded rows
    const int64_t lim = (int64_t)1 << 31;
    const int64_t rows = (d->n > d->m ? d->n : d->m) + kElMaxSlabRows + 4;
    const int64_t ldmax[] = {d->Z ? d->ld_z : 0, d->E ? d->ld_e : 0, d->Zref ? d->ld_zref : 0,
                             d->Eref ? d->ld_eref : 0, d->mode == 1 ? d->ld_g : 0};
    for (int64_t v : ldmax)
      if (rows * v * 4 >= lim) return DLADMM_E_UNSUPPORTED;
  }
  p->wide = d->batch >= kElWideBatch;
  const int ct = p->wide ? kElWideCT : kElNarrowCT;
  const int sr = kElWaves * (p->wide ? kElWideNR : kElNarrowNR) * (64 / ct);
  p->n4 = d->Z ? (d->n + 3) / 4 * 4 : 0;
  const int rv = p->n4 + (d->E ? d->m : 0);
  p->slabs = (rv + sr - 1) / sr;
  p->ctiles = (d->batch + ct - 1) / ct;
  // grid.y: the slabs of the fused launch, the 2 K rows of sums of the finish
  if (p->slabs > kElMaxGridY || 2 * (int64_t)d->layers > kElMaxGridY) return DLADMM_E_UNSUPPORTED;
  const size_t b = (size_t)p->slabs * (size_t)d->layers * 2 * (size_t)B * sizeof(double);
  p->bytes = (b + 255) & ~(size_t)255;
  return 0;
}

}  // namespace

}  // namespace dladmm

extern "C" {

size_t dladmm_elemloss_workspace_bytes(const dladmm_elemloss_desc* d) {
  dladmm::ElPlan p;
  return dladmm::el_plan(d, &p, true) ? 0 : p.bytes;
}

int dladmm_elemloss_f32(const dladmm_elemloss_desc* d, void* stream) {
  using namespace dladmm;
  ElPlan p;
  if (int e = el_plan(d, &p, false)) return e;
  if (!d->workspace || d->workspace_bytes < p.bytes) return DLADMM_E_WORKSPACE;
  if (((uintptr_t)d->workspace) & 255) return DLADMM_E_ALIGN;
  hipStream_t s = (hipStream_t)stream;
  const bool grad = d->mode == 1;
  const uint32_t B4 = 4u;
  ElemLossArgs a{};
  a.n4 = p.n4; a.B = d->batch; a.K = d->layers;
  if (d->Z) {
    a.Z = d->Z; a.zls = d->z_layer_stride; a.ldz = d->ld_z;
    a.zbytes = (uint32_t)(d->n * d->ld_z * B4);
    if (d->Zref) { a.Zref = d->Zref; a.ldzr = d->ld_zref; a.zrbytes = (uint32_t)(d->n * d->ld_zref * B4); }
    if (grad) { a.gZ = d->gZ; a.gzls = d->gz_layer_stride; a.gzbytes = (uint32_t)(d->n * d->ld_g * B4); }
  }
  if (d->E) {
    a.E = d->E; a.els = d->e_layer_stride; a.lde = d->ld_e;
    a.ebytes = (uint32_t)(d->m * d->ld_e * B4);
    if (d->Eref) { a.Eref = d->Eref; a.lder = d->ld_eref; a.erbytes = (uint32_t)(d->m * d->ld_eref * B4); }
    if (grad) { a.gE = d->gE; a.gels = d->ge_layer_stride; a.gebytes = (uint32_t)(d->m * d->ld_g * B4); }
  }
  a.w = d->w; a.ldg = grad ? d->ld_g : 0;
  a.part = (double*)d->workspace;
  const dim3 grid((unsigned)p.ctiles, (unsigned)p.slabs);
  // the wanted-layer mask is a kernel argument: one launch per kElChunk layers
  for (int k0 = 0; k0 < d->layers; k0 += kElChunk) {
    a.k0 = k0;
    a.k1 = k0 + kElChunk < d->layers ? k0 + kElChunk : d->layers;
    a.want = 0;
    if (grad)
      for (int k = a.k0; k < a.k1; ++k)
        if (!d->want || d->want[k]) a.want |= (uint64_t)1 << (k - k0);
    if (hipError_t e = launch_elemloss(a, p.wide, d->power == 1, grad, grid, s)) return (int)e;
  }
  return (int)launch_elemloss_finish(a.part, p.slabs, 2 * d->layers, d->batch, d->colsum,
                                     d->total, s);
}

}  // extern "C"
