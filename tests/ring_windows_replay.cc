// ring_windows_replay.cc -- host replay of the fused kernel's weight-ring schedule
// (d-ladmm_amd/csrc/dladmm_ring_windows.h), built and run by tests/test_ring_windows.py with the
// knob sets the library can be built with.
//
// For every (MB, NB, PKIND, SAVEP, load-P0 form) and every wave, the program lists in program
// order every vector-memory operation the kernel issues over the passes of a forward: the ring's
// LDS-DMA pieces at their steps, the stores of the epilogue rows, V1's beta loads.  The list is
// written from the kernel's loop structure (dladmm_fused_kernel.h: step_head, the rows, the
// MFMAs, step_tail), not from WinCount.  Then, for every ring barrier:
//   * every piece of the awaited chunk was issued before the barrier;
//   * the counted window is at most the number of operations issued after the awaited chunk's
//     last piece (one more would let the barrier pass before that piece has landed);
//   * no piece went into a slot before the barrier that freed it.
// Prints the slack (operations issued minus window) per instantiation; exit status 1 on failure.
#include <cstdio>
#include <utility>
#include <vector>

#include "dladmm_ring_windows.h"

using namespace dladmm;

namespace {

enum { EV_PIECE, EV_OP, EV_BARRIER };
struct Ev {
  int type, chunk, n;  // PIECE: chunk; BARRIER: chunk whose last step holds it, n = window
};

template <typename W, int... S>
std::vector<int> table_g1(std::integer_sequence<int, S...>) {
  return {W::template g1<S>()...};
}
template <typename W, bool PRO, int... S>
std::vector<int> table_g2(std::integer_sequence<int, S...>) {
  return {W::template g2<S, PRO>()...};
}

int failures = 0;

// ALLOW2: what the kernel passes for the instantiation (false: it keeps the ring of the knobs
// whatever DLADMM_RING2 says); both values are replayed for every instantiation
template <int MB, int NB, int PKIND, bool SAVEP, bool P0LOAD, bool ALLOW2>
void replay() {
  using R = RingSched<MB * NB, PKIND, ALLOW2>;
  using W = WinCount<MB, NB, R::CF, PKIND, SAVEP, ALLOW2>;
  constexpr int T1 = (NB / 2) * MB, T2 = (MB / 2) * NB, SPC = R::SPC;
  constexpr int ST2 = SAVEP ? 4 : 3, PF = PKIND == kWinPkElem ? 3 : 0;
  const std::vector<int> w1 = table_g1<W>(std::make_integer_sequence<int, T1>{});
  const std::vector<int> w2p = table_g2<W, true>(std::make_integer_sequence<int, T2>{});
  const std::vector<int> w2 = table_g2<W, false>(std::make_integer_sequence<int, T2>{});
  constexpr int K = 3;
  int min_slack = 1 << 30, max_win = 0, barriers = 0;
  for (int w = 0; w < 4; ++w) {
    std::vector<Ev> ev;
    // priming: chunks 0 .. AH-2 whole and the offset-0 pieces of chunk AH-1 are issued and waited
    // for (vmcnt(0)) before the first step: they are complete, not part of the list.  `primed`
    // pieces of chunk AH-1:
    int primed_last = 0;
    for (int i = 0; i < R::NPC; ++i) primed_last += R::piece_offset(i, w) == 0 ? 1 : 0;
    int gs = 0;  // global step = position in the chunk stream
    auto pieces_at = [&](int o, int chunk) {  // the pieces of offset o, in the kernel's order
      for (int i = 0; i < R::NPC; ++i)
        if (R::piece_offset(i, w) == o) ev.push_back({EV_PIECE, chunk, 0});
    };
    auto pass = [&](int kind) {  // 0: prologue G2, 1: G1, 2: G2
      const int T = kind == 1 ? T1 : T2;
      for (int s = 0; s < T; ++s, ++gs) {
        const int c = gs / SPC, pos = gs % SPC;
        const bool boundary = pos == SPC - 1;
        // step_head
        if (boundary) {
          const int n = kind == 1 ? w1[s] : kind == 0 ? w2p[s] : w2[s];
          ev.push_back({EV_BARRIER, c, n});
          if (!R::LATE && !R::SPREAD) pieces_at(0, c + R::AH);
        } else if ((kind == 1 ? w1[s] : kind == 0 ? w2p[s] : w2[s]) != 0) {
          std::printf("FAIL window at a step without a barrier\n");
          ++failures;
        }
        // the step's body: beta prefetch parts, epilogue rows
        if (kind == 1) {
          const int p = s / MB, jb = s % MB;
          for (int i = 0; i < 8; ++i)
            if (rows_at(jb, MB, i))
              for (int q = 0; q < (p == 0 ? ST2 : 1); ++q) ev.push_back({EV_OP, 0, 0});
        } else {
          const int p = s / NB, kb = s % NB;
          if (p == 0)
            for (int part = 0; part < 8; ++part)
              if (W::part_step(part) == kb)
                for (int q = 0; q < PF; ++q) ev.push_back({EV_OP, 0, 0});
          for (int i = 0; i < 8; ++i)
            if (rows_at(kb, NB, i)) {
              if (p == 0) {
                if (kind == 2) ev.push_back({EV_OP, 0, 0});  // G1's last pair: one Z store
              } else {
                for (int q = 0; q < ST2 + PF; ++q) ev.push_back({EV_OP, 0, 0});
              }
            }
        }
        // step_tail
        if (boundary && R::LATE) pieces_at(0, c + R::AH);
        if (R::SPREAD) {
          // offset from the last barrier step; before the first barrier the priming stands in
          const int o = boundary ? 0 : pos + 1;
          const int chunk = (boundary ? c : c - 1) + R::AH;
          pieces_at(o, chunk);
        }
      }
    };
    if (!P0LOAD) pass(0);
    for (int k = 0; k < K; ++k) {
      pass(1);
      pass(2);
    }
    // checks
    const int nchunks = gs / SPC;
    std::vector<int> barrier_at(nchunks + 1, -1), last_piece(nchunks + R::AH + 1, -1),
        first_piece(nchunks + R::AH + 1, -1), npieces(nchunks + R::AH + 1, 0);
    for (int e = 0; e < (int)ev.size(); ++e) {
      if (ev[e].type == EV_BARRIER) barrier_at[ev[e].chunk] = e;
      if (ev[e].type == EV_PIECE) {
        if (first_piece[ev[e].chunk] < 0) first_piece[ev[e].chunk] = e;
        last_piece[ev[e].chunk] = e;
        ++npieces[ev[e].chunk];
      }
    }
    for (int c = 0; c + 1 < nchunks; ++c) {
      const int b = barrier_at[c], a = c + 1;  // barrier at chunk c's last step awaits chunk a
      if (b < 0) {
        std::printf("FAIL no barrier at the last step of chunk %d\n", c);
        ++failures;
        continue;
      }
      ++barriers;
      const int win = ev[b].n;
      max_win = win > max_win ? win : max_win;
      const int want = R::NPC - (a == R::AH - 1 ? primed_last : 0);
      if (a < R::AH - 1 || want == 0) continue;  // landed before the first step: any count is safe
      if (npieces[a] != want || last_piece[a] > b) {
        std::printf("FAIL wave %d chunk %d: %d of %d pieces issued before its barrier\n", w, a,
                    npieces[a], want);
        ++failures;
        continue;
      }
      int issued = 0;
      for (int e = last_piece[a] + 1; e < b; ++e) issued += ev[e].type != EV_BARRIER ? 1 : 0;
      if (win > issued) {
        std::printf("FAIL wave %d barrier of chunk %d: window %d > %d operations issued since\n",
                    w, c, win, issued);
        ++failures;
      }
      min_slack = issued - win < min_slack ? issued - win : min_slack;
      // chunk a's slot held chunk a - SLOTS: free from the barrier at that chunk's last step
      const int freed = a - R::SLOTS;
      if (freed >= 0 && first_piece[a] < barrier_at[freed]) {
        std::printf("FAIL wave %d chunk %d issued before the barrier that frees its slot\n", w, a);
        ++failures;
      }
    }
  }
  std::printf("MB %2d NB %2d CF %2d SLOTS %d PKIND %d SAVEP %d P0LOAD %d ALLOW2 %d: barriers %4d "
              "max window %2d min slack %d\n",
              MB, NB, R::CF, R::SLOTS, PKIND, (int)SAVEP, (int)P0LOAD, (int)ALLOW2, barriers,
              max_win, min_slack);
}

template <int MB, int NB, int PKIND>
void forms() {
  replay<MB, NB, PKIND, false, false, true>();
  replay<MB, NB, PKIND, true, false, true>();
  replay<MB, NB, PKIND, false, true, true>();
  replay<MB, NB, PKIND, true, true, true>();
  replay<MB, NB, PKIND, false, false, false>();
  replay<MB, NB, PKIND, true, false, false>();
  replay<MB, NB, PKIND, false, true, false>();
  replay<MB, NB, PKIND, true, true, false>();
}

template <int MB, int NB>
void kinds() {
  forms<MB, NB, 0>();  // PK_SCALAR: V4, V6
  forms<MB, NB, 1>();  // PK_ROW: V2, V3
  forms<MB, NB, 2>();  // PK_ELEM: V1
  forms<MB, NB, 3>();  // PK_S1: V5, V7, the ELZ units
}

}  // namespace

int main() {
  std::printf("RING2 %d CHUNK %d SLOTS %d OWN %d LATE %d SPREAD %d STAGGER %d CNT %d\n",
              DLADMM_RING2, DLADMM_CHUNK, DLADMM_SLOTS, DLADMM_RING_OWN, DLADMM_DMA_LATE,
              DLADMM_DMA_SPREAD, DLADMM_DMA_STAGGER, DLADMM_CNT);
  kinds<2, 2>();    // 32 x 32
  kinds<4, 16>();   // 64 x 256
  kinds<16, 32>();  // 256 x 512
  std::printf(failures ? "FAILED: %d\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
