// dladmm_elemloss.h -- contract between dladmm_elemloss_f32 and its kernels (dladmm_elemloss.hip):
// the element-wise training terms sum (V_k - Vref)^2 / sum |V_k - Vref| of all K layers of a
// forward's stacked Z and E outputs, and their cotangent seeds, in one streaming launch.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dladmm {

constexpr int kElChunk = 64;  // layers of one launch (the wanted-layer mask is a kernel argument)

// The two tiles.  A workgroup of four waves owns CT columns and a slab of 4 * NR * (64 / CT) rows
// of the virtual row space [Z rows, padded to a multiple of 4; E rows].
constexpr int kElNarrowCT = 16, kElNarrowNR = 2;  // 4 rows x 16 columns per wave access
constexpr int kElWideCT = 64, kElWideNR = 16;     // 1 row x 64 columns: a full 256-byte segment
constexpr int kElWideBatch = 2048;                // batch >= this: the wide tile
constexpr int kElMaxSlabRows = 64;                // of either tile (offset-range validation)
constexpr int kElMaxGridY = 65535;                // a launch's second grid dimension

struct ElemLossArgs {
  int n4;             // Z rows of the virtual space: n rounded up to 4 (0: no Z)
  int B, K;           // columns; layers of the whole call (the partials' layout)
  int k0, k1;         // this launch's layers
  uint64_t want;      // bit (k - k0): layer k's cotangents are stored (the adjoint form)
  const float* Z; int64_t zls, ldz; uint32_t zbytes;    // layer stride, row stride; n * ldz * 4
  const float* E; int64_t els, lde; uint32_t ebytes;
  const float* Zref; int64_t ldzr; uint32_t zrbytes;    // 0 bytes: no reference (zero)
  const float* Eref; int64_t lder; uint32_t erbytes;
  const float* w;     // device [K] (the adjoint form)
  float* gZ; int64_t gzls; uint32_t gzbytes;            // 0 bytes: not stored
  float* gE; int64_t gels; uint32_t gebytes;
  int64_t ldg;
  double* part;       // [slabs][K][2][B] column partials of the row slabs
};

// grid (column tiles, row slabs); wide: the 64-column tile; absf: |.| instead of (.)^2;
// grad: also the cotangents
hipError_t launch_elemloss(const ElemLossArgs& a, bool wide, bool absf, bool grad, dim3 grid,
                           hipStream_t s);
// colsum[kt][b] = part[0][kt][b] + ... + part[slabs - 1][kt][b], kt < K2 = 2 K, and total[kt] =
// the sum of colsum[kt][:] (thread t: columns t, t + 256, ... in order; the wave's xor tree; the
// four waves in order)
hipError_t launch_elemloss_finish(const double* part, int slabs, int K2, int B, double* colsum,
                                  double* total, hipStream_t s);

}  // namespace dladmm
