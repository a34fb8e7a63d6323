// dladmm_ring_windows.h -- the weight ring's issue schedule and the counted vmcnt windows of its
// barriers, as pure compile-time arithmetic: no device code, no HIP header, so the host replay of
// tests/test_ring_windows.py includes this file as the fused kernel (dladmm_fused_kernel.h) does.
//
// The ring.  The weight stream is cut into chunks of CF fragments (SPC = CF / 2 MFMA steps); a
// wave brings in NPC = CF / 4 one-KiB pieces of every chunk by LDS-DMA.  The head of a chunk's
// last step holds the ring barrier: it waits until chunk c + 1 has landed, and it frees a slot,
// into which chunk c + AH is issued.  D = AH - 1 barriers later that chunk is awaited.
//  * DLADMM_RING_OWN = 0: the freed slot is the one of chunk c - 1 (AH = SLOTS - 1, SLOTS >= 3).
//  * DLADMM_RING_OWN = 1: the freed slot is chunk c's own (AH = SLOTS, SLOTS >= 2).  By that
//    barrier every wave has read chunk c's last two fragments into registers -- they are read in
//    the head of the step before, and the barrier's lgkmcnt(0) precedes its s_barrier -- so no
//    wave reads slot c again, and the first LDS-DMA into it is issued after the barrier.  S slots
//    then hold S chunks ahead of the reader: the lead of the 4-slot ring at 3 slots, or chunks of
//    32 fragments in a 2-slot ring at the same 64 KiB and half the barriers.
// When the pieces are issued, as offsets o in steps from the barrier step (o = 0):
//  * default: all NPC in the head of the barrier step, before the step's body;
//  * DLADMM_DMA_LATE: all NPC after the barrier step's MFMAs;
//  * DLADMM_DMA_SPREAD: piece i after the MFMAs of step o = i + stag(w), one per step, never
//    beside the fragment reads of a step head.  DLADMM_DMA_STAGGER: stag(w) = 0 | w & 1 | w,
//    reduced modulo SMAX + 1 so that every piece is issued before the next barrier.
#pragma once

#ifndef DLADMM_SLOTS
#define DLADMM_SLOTS 4  // weight ring slots; the per-row kinds (their parameter tables take
                        // 24 KiB of LDS) use at most 64 KiB of ring
#endif
#ifndef DLADMM_CNT
#define DLADMM_CNT 1  // ring barriers of every variant wait with counted vmcnt (else only V1)
#endif
#ifndef DLADMM_CHUNK
#define DLADMM_CHUNK 16
#endif
#ifndef DLADMM_DMA_LATE
#define DLADMM_DMA_LATE 0  // ring LDS-DMA group issued after the barrier step's MFMAs instead of
                           // beside its fragment reads (A/B; the ring windows count accordingly)
#endif
#ifndef DLADMM_RING_OWN
#define DLADMM_RING_OWN 0  // the barrier at a chunk's last step refills that chunk's own slot
#endif
#ifndef DLADMM_DMA_SPREAD
#define DLADMM_DMA_SPREAD 0  // one piece per MFMA step after the barrier, each after the MFMAs
#endif
#ifndef DLADMM_DMA_STAGGER
#define DLADMM_DMA_STAGGER 0  // with DLADMM_DMA_SPREAD: wave w starts 0 | w & 1 | w steps later
#endif
#ifndef DLADMM_RING2
// The adopted form: an instantiation with at least 512 fragments per GEMM
// (256 x 512) streams chunks of 32 fragments through a two-slot own-slot ring -- the same 64 KiB
// as four slots of 16, half the barriers -- with its pieces spread.  A deliberate deviation from
// the four-slot ring's lead: a chunk's first piece is issued 16 steps before the barrier that
// awaits it, as the whole clump was before, but its last piece only 8 steps before; measured, the
// vmcnt wait per barrier did not grow.  Smaller instantiations keep the ring the knobs above
// describe: 64 x 256 would have two such chunks per GEMM and measured 13 % slower with them,
// 32 x 32 has one 4-fragment chunk per GEMM.
// 0: every instantiation uses the knobs above as given (at their defaults: the ring before).
#define DLADMM_RING2 1
#endif
#if DLADMM_DMA_SPREAD && DLADMM_DMA_LATE
#error "DLADMM_DMA_SPREAD and DLADMM_DMA_LATE are alternatives"
#endif

namespace dladmm {

constexpr int kWinPkRow = 1, kWinPkElem = 2;  // = PK_ROW, PK_ELEM (dladmm_common.h)

// Ring geometry and piece schedule of an instantiation with GF fragments per GEMM.  ALLOW2 =
// false: an instantiation that keeps the ring the knobs describe whatever DLADMM_RING2 says (the
// kernel decides which: it would spill with the adopted form, or measured slower).
template <int GF, int PKIND, bool ALLOW2 = true>
struct RingSched {
  static constexpr bool R2 = DLADMM_RING2 != 0 && ALLOW2 && GF >= 512 && GF % 32 == 0;
  static constexpr int CHUNK = R2 ? 32 : DLADMM_CHUNK, WANT = R2 ? 2 : DLADMM_SLOTS;
  static constexpr int CF = GF < CHUNK ? GF : CHUNK;                // fragments per chunk
  static constexpr int NCH = GF / CF;                               // chunks per GEMM
  static constexpr int SPC = CF / 2;                                // steps per chunk
  static constexpr int NPC = (CF + 3) / 4;                          // pieces per wave and chunk
  static constexpr int ROWMAX = CF > 16 ? 64 / CF : 4;              // per-row kinds: 64 KiB
  static constexpr int SLOTS =
      (PKIND == kWinPkRow && WANT > ROWMAX) ? ROWMAX : WANT;
  static constexpr bool OWN = R2 || DLADMM_RING_OWN != 0;
  static constexpr int AH = OWN ? SLOTS : SLOTS - 1;  // chunks ahead: barrier c issues c + AH
  static constexpr int D = AH - 1;                    // barriers from issue to await
  static constexpr bool SPREAD = R2 || DLADMM_DMA_SPREAD != 0;
  static constexpr bool LATE = !R2 && DLADMM_DMA_LATE != 0;
  // largest stagger that keeps the last piece before the next barrier (o <= SPC - 1)
  static constexpr int SROOM = SPC - NPC;
  static constexpr int SWANT = DLADMM_DMA_STAGGER == 1 ? 1 : DLADMM_DMA_STAGGER == 2 ? 3 : 0;
  static constexpr int SMAX = !SPREAD ? 0 : (SWANT < SROOM ? SWANT : (SROOM > 0 ? SROOM : 0));
  static constexpr int stag(int w) {
    const int s = DLADMM_DMA_STAGGER == 1 ? (w & 1) : DLADMM_DMA_STAGGER == 2 ? w : 0;
    return s % (SMAX + 1);
  }
  // offset (steps after the barrier step) at which wave w issues piece i; the default and the
  // late form issue every piece in the barrier step
  static constexpr int piece_offset(int i, int w) { return SPREAD ? i + stag(w) : 0; }
  static constexpr int OLAST = SPREAD ? NPC - 1 + SMAX : 0;  // latest offset of any wave
  static_assert(SLOTS >= (OWN ? 2 : 3), "one slot being read, one landed (and one in flight)");
  static_assert(!SPREAD || CF % 4 == 0, "spread pieces: every wave has the same NPC");
  static_assert(!SPREAD || OLAST <= SPC - 1, "every piece is issued before the next barrier");
};

// pending epilogue row i (0..7: block half i/4, row i%4) runs at step (i * SP) / 8 of a pair of
// SP steps
constexpr bool rows_at(int step, int SP, int i) { return (i * SP) / 8 == step; }

// Static VM-operation windows of the ring barriers (V1 / PK_ELEM: its 24 beta loads per G2 pair
// would otherwise be drained by the vmcnt(0) of the next barrier, one chunk after issue).  A
// barrier at step s (the last step of a chunk of SPC steps) waits for the chunk whose pieces were
// issued from the barrier step s - D * SPC on.  Newer than the LAST of those pieces are: every
// store and beta load issued in the bodies of the steps after it up to s - 1 (the barrier step's
// own body follows its head), and all pieces of the D - 1 chunks issued since -- they count like
// stores.  The last piece is issued before the body of its step (default), or after it (late and
// spread forms: that body is older); with a stagger the window starts after the latest wave's
// last piece, so that one count is right for every wave.  Counted: the stores of the epilogue
// rows (always issued; out-of-range ones go to 0-record buffers) and the beta prefetch at each G2
// pair start.  Not counted (conditional): the per-column objective stores and the per-row
// tables' DMA -- counting too few only waits longer; counting one too many is a data race.
// Without DLADMM_CNT the variants other than V1 return 0 (plain vmcnt(0)).
template <int MB, int NB, int CF, int PKIND, bool SAVEP, bool ALLOW2 = true>
struct WinCount {
  using R = RingSched<MB * NB, PKIND, ALLOW2>;
  static_assert(R::CF == CF, "chunk size");
  static constexpr int ST2 = SAVEP ? 4 : 3;  // stores of a G2 row: E, L, T (+ P)
  static constexpr int SPC = CF / 2;  // steps per chunk
  static constexpr int rows_in(int step, int SP) {
    int c = 0;
    for (int i = 0; i < 8; ++i) c += ((i * SP) / 8 == step) ? 1 : 0;
    return c;
  }
  // VM operations issued in the body of step t of a G1 / G2 pass
  static constexpr int ops1(int t) {
    return rows_in(t % MB, MB) * (t / MB == 0 ? ST2 : 1);  // pair 0 runs G2 rows (E, L, T)
  }
  // step of the pair that issues beta-prefetch part `part` (3 loads)
  static constexpr int part_step(int part) { return (part * NB) / 16; }
  static constexpr int parts_at(int kb) {
    int c = 0;
    for (int q = 0; q < 8; ++q) c += part_step(q) == kb ? 1 : 0;
    return c;
  }
  static constexpr int ops2(int t, bool pro) {
    const int p = t / NB, kb = t % NB;
    constexpr int pf = PKIND == kWinPkElem ? 3 : 0;  // beta loads per prefetch part
    if (p == 0) return (pro ? 0 : rows_in(kb, NB)) + pf * parts_at(kb);  // G1 rows + prefetch
    return (ST2 + pf) * rows_in(kb, NB);  // G2 rows (E, L, T stores) + a prefetch part each
  }
  static constexpr int T1 = (NB / 2) * MB, T2 = (MB / 2) * NB;  // steps of a G1 / G2 pass
  // A step before the pass counts with the previous pass's schedule (the smaller of the two
  // possible previous passes before G1; nothing before the prologue).
  static constexpr int SLOTS = R::SLOTS;
  static constexpr int WSTEPS = R::D * SPC;
  // first step after the barrier step s - WSTEPS whose body is newer than the awaited chunk
  static constexpr int W0 = R::LATE ? 1 : R::SPREAD ? R::OLAST + 1 : 0;
  static constexpr int DMAG = (R::D - 1) * R::NPC;
  template <int S>
  static constexpr int g1() {
    if constexpr ((PKIND != kWinPkElem && !DLADMM_CNT) || S % SPC != SPC - 1) return 0;
    int n = DMAG;
    for (int t = S - WSTEPS + W0; t < S; ++t) {
      if (t >= 0) n += ops1(t);
      else if (T2 + t >= 0) {
        const int a = ops2(T2 + t, true), b = ops2(T2 + t, false);
        n += a < b ? a : b;
      }
    }
    return n < 63 ? n : 63;
  }
  template <int S, bool PRO>
  static constexpr int g2() {
    if constexpr ((PKIND != kWinPkElem && !DLADMM_CNT) || S % SPC != SPC - 1) return 0;
    int n = DMAG;
    for (int t = S - WSTEPS + W0; t < S; ++t) {
      if (t >= 0) n += ops2(t, PRO);
      else if (!PRO && T1 + t >= 0) n += ops1(T1 + t);
    }
    return n < 63 ? n : 63;
  }
};

}  // namespace dladmm
