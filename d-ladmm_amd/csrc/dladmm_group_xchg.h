// dladmm_group_xchg.h -- the group exchange of the row-split kernels: how the workgroups that
// share 16 batch columns (a group) hand the B operand of the next product to each other.  Used by
// the forward (dladmm_fused_rs_kernel.h, paths 5 and 6) and the reverse sweep
// (dladmm_reverse_rs_kernel.h, bwd paths 2 and 3); this is the one copy of the protocol.
//
// MEM = 1: the group is one workgroup, the operand goes through LDS and the hand-off is a
// workgroup barrier.  MEM = kXsMembers: the group is 4 workgroups on 4 CUs.  After each product
// every wave stores its blocks to the group's exchange buffer in global memory (xstore: 16-byte
// `sc1` stores), then handoff():
//   every storing wave's `s_waitcnt vmcnt(0)`, a workgroup barrier, one agent-scope atomic add per
//   member to the group's counter; one lane polls the counter with `sc1` loads (bounded), a
//   workgroup barrier, then every thread's `sc1` loads of the buffer into LDS, and a barrier.
// MI355X_MICROARCH.md, inter-workgroup visibility: a CU's vector L1 is never refreshed by another
// CU's stores and the per-XCD L2s are not coherent, so `sc1` loads may stand in for an agent
// acquire only when (1) EVERY load of the handed-off bytes is a `global_` / `buffer_` `sc1` load,
// (2) the producer stored every one of those bytes `sc1`, (3) every storing wave ran
// `s_waitcnt vmcnt(0)` after its stores and the lane that signals for the other waves of its
// workgroup does so behind a workgroup barrier, (4) the hand-off matches one row of that
// section's table in every cell.  This is its first row: ONE lane of each storing workgroup adds
// to the counter for ALL that workgroup's stores; the consumer learns it by an `sc1` load poll of
// that counter; the other waves load after a workgroup barrier the polling wave then joins;
// hipMalloc memory, one workgroup per CU; 16-byte stores and loads.  Valid at any placement.
// Members are blocks b, b + 8, b + 16, b + 24 of a 32-block stripe, which the dispatcher deals to
// one XCD (observed, speed only: the hand-off stays in that XCD's L2).  A group is resident
// together because the plan launches at most one workgroup per CU.  Every poll is bounded (it
// ends after XS_SPIN polls, never a hang) and a timeout is sticky: every output written after it
// goes through fin() and is NaN, not silently wrong.
#pragma once
#include "dladmm_internal.h"

#ifndef XS_SPIN
#define XS_SPIN (1 << 22)  // bound of every hand-off poll, forward and backward
#endif
#ifndef XS_ABL
#define XS_ABL 0  // timing ablations only (wrong results): 1 no poll wait, 2 no exchange loads
                  // into LDS, 4 no exchange stores (tools/ablate_units.py)
#endif
#ifndef XS_PRE_LATE
#define XS_PRE_LATE 1  // 1: issue the caller's loads (the forward: the next pass's first weight
                       // fragments) right behind the exchange loads (the LDS writes wait for
                       // those only); 0: before the poll.  V4 K = 15 (ms, B = 20 / 1,000):
                       // 0.201 / 0.214 vs 0.207 / 0.221 (profiles/r06_xsplit_ab.json)
#endif

namespace dladmm {

constexpr int kXsMembersLog2 = 2, kXsStripeLog2 = 3;
constexpr int kXsMembers = 1 << kXsMembersLog2;  // workgroups per 16-column group
constexpr int kXsWaves = kXsMembers * kWaves;    // waves per group
constexpr int kXsStripe = 1 << kXsStripeLog2;    // groups per stripe (kXsStripe * kXsMembers blocks)
constexpr int kXsNB = kShapeNP[2] / 16, kXsMB = kShapeMP[2] / 16;  // blocks of the n / m states

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

template <int MEM>
struct GroupXchg {
  static_assert(MEM == 1 || MEM == kXsMembers, "one workgroup per group, or kXsMembers");
  int grp, mem;       // this workgroup's 16-column group and its member index in it
  unsigned* cnt = nullptr;  // the group's hand-off counter, on a line of its own (zeroed
                            // before the launch)
  unsigned hand = 0;  // the count that completes the next hand-off
  int* xerr = nullptr;  // LDS, sticky: a hand-off timed out
  bool bad = false;

  __device__ __forceinline__ GroupXchg() {
    const int xb = blockIdx.x;
    // members share xb % kXsStripe (one XCD)
    grp = MEM == 1 ? xb
                   : (xb >> (kXsStripeLog2 + kXsMembersLog2)) * kXsStripe + (xb & (kXsStripe - 1));
    mem = MEM == 1 ? 0 : (xb >> kXsStripeLog2) & (kXsMembers - 1);
  }
  // a group that holds columns joins the exchange (a padding group has left: every member does)
  __device__ __forceinline__ void join(unsigned* xcnt) {
    if constexpr (MEM > 1) {
      __shared__ int err;
      cnt = xcnt + grp * 64;
      xerr = &err;
      if (threadIdx.x == 0) err = 0;
    }
  }
  // an output value, or NaN once a hand-off has timed out (the outputs of every later product
  // would be computed on incomplete operands)
  __device__ __forceinline__ float fin(float x) const {
    return MEM > 1 && bad ? __builtin_nanf("") : x;
  }
  // block blk of this wave's output to the exchange buffer rb
  __device__ __forceinline__ void xstore(const rsrc_t& rb, int blk, int lane,
                                         const f32x4& val) const {
    if constexpr (MEM > 1 && !(XS_ABL & 4))
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, val), rb,
                                             (blk * 64 + lane) * 16, 0, 16);
  }
  // hand-off, called by every wave of the workgroup: this member's stores are done; wait for every
  // member's, then the buffer's NBLK blocks (sc1: past this CU's L1) into LDS at dst.  pre():
  // loads of the caller's to issue behind the exchange loads
  template <int NBLK, class Pre>
  __device__ __forceinline__ void handoff(const rsrc_t& rb, f32x4* dst,
                                          std::integral_constant<int, NBLK>, Pre&& pre) {
    if constexpr (MEM == 1) {
      __syncthreads();
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if constexpr (!XS_PRE_LATE) pre();  // in flight while lane 0 polls
      hand += MEM;
      if (threadIdx.x == 0) {
        __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        int it = 0;
        unsigned c = __hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        while (!(XS_ABL & 1) && c < hand && ++it < XS_SPIN) {
          __builtin_amdgcn_s_sleep(1);
          c = __hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (!(XS_ABL & 1) && c < hand) *xerr = 1;  // a member never arrived
      }
      __syncthreads();
      bad = __builtin_amdgcn_readfirstlane(*xerr) != 0;
      constexpr int per = (XS_ABL & 2) ? 0 : NBLK * 64 / 256;  // f32x4 per thread
      f32x4 t[per > 0 ? per : 1];
#pragma unroll
      for (int j = 0; j < per; ++j)
        t[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                             rb, (threadIdx.x + 256 * j) * 16, 0, 16));
      if constexpr (XS_PRE_LATE) pre();
#pragma unroll
      for (int j = 0; j < per; ++j) dst[threadIdx.x + 256 * j] = t[j];
      __syncthreads();
    }
  }
  template <int NBLK>
  __device__ __forceinline__ void handoff(const rsrc_t& rb, f32x4* dst,
                                          std::integral_constant<int, NBLK> n) {
    handoff(rb, dst, n, [] {});
  }
};

}  // namespace dladmm
