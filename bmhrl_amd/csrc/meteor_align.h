// The METEOR alignment of one hypothesis prefix against one reference by one wave, shared by the
// per-prefix reward launch (meteor.hip) and the all-pairs matrix launch (soda.hip).
//
// The lanes of a wave hold the reference positions j = 64 q + lane (kQ = R/64 per lane: word, stem and a "used" bit) and the
// hypothesis words h = 64 p + lane (kP = L/64 per lane: word, stem, and the reference position the word was matched to).
// Which words are matched is a wave-uniform bit mask.  For every stage (exact, stem, synonym) the wave walks the set bits of
// "h < m and unmatched" from the top; the word's key comes out of its lane by readlane, the lanes test their unused
// reference positions, a ballot per 64 positions from the top picks the highest j, and the owning lanes mark it used and
// record it (a reference of at most 64 words takes a body without the loop over the groups of 64).  The chunk count compares
// every lane's match with its lower neighbour's.
//
// Include it after common.h and include/bmhrl_hip.h, inside a file that has set `#pragma clang fp contract(off)`.
#pragma once
#include "caption_text.h"                // kMaxL, kMaxR; the stages around the alignment

namespace {

typedef unsigned long long u64;

constexpr int kQ = kMaxR / WAVE;       // reference positions per lane
constexpr int kP = kMaxL / WAVE;       // hypothesis words per lane
static_assert(kMaxR % WAVE == 0 && kMaxL % WAVE == 0 && kQ <= 32, "the used bits of a lane are one word");

// the highest unused reference position that passes the stage's test for the word h with this key (-1: none); its lane
// marks it used.  STAGE 0: equal words, 1: equal stems, 2: the word's precomputed synonym mask.
// NQ: the groups of 64 reference positions the code covers (1: a reference of at most 64 words, no loop; kQ: nq of them).
template <int STAGE, int NQ>
__device__ __forceinline__ int take_highest(int key, int h, int nq, int lane, const u64 (*syn)[kQ], const int (&rw)[kQ],
                                            const int (&rs)[kQ], unsigned& used) {
  int j = -1;
#pragma unroll
  for (int q = NQ - 1; q >= 0; --q) {
    if (NQ == 1 || (q < nq && j < 0)) {
      bool hit = !((used >> q) & 1u);
      if (STAGE == 0) hit = hit && rw[q] == key;
      if (STAGE == 1) hit = hit && rs[q] == key;
      if (STAGE == 2) hit = hit && ((syn[h][q] >> lane) & 1ull);
      const u64 bal = __ballot(hit);
      if (bal) {
        const int l = 63 - __clzll((long long)bal);
        j = q * WAVE + l;
        if (lane == l) used |= 1u << q;
      }
    }
  }
  return j;
}

// One stage over the prefix of m words: every unmatched h from last to first takes the highest unused reference position
// whose test holds.  matched[p] bit l: word 64 p + l is matched, to mate[p] of lane l.
template <int STAGE, int NQ>
__device__ __forceinline__ void match_stage(int m, int nq, int lane, const int (&hw)[kP], const int (&hs)[kP],
                                            const u64 (*syn)[kQ], const int (&rw)[kQ], const int (&rs)[kQ], unsigned& used,
                                            u64 (&matched)[kP], int (&mate)[kP]) {
#pragma unroll
  for (int p = kP - 1; p >= 0; --p) {
    if (p * WAVE < m) {
      const int n = m - p * WAVE;       // words of the prefix in this group of 64 (at least one)
      u64 todo = (n >= WAVE ? ~0ull : (1ull << n) - 1ull) & ~matched[p];
      while (todo) {
        const int l = 63 - __clzll((long long)todo);
        todo &= ~(1ull << l);
        const int key = __builtin_amdgcn_readlane(STAGE == 1 ? hs[p] : hw[p], l);
        const int j = take_highest<STAGE, NQ>(key, p * WAVE + l, nq, lane, syn, rw, rs, used);
        if (j >= 0) {
          matched[p] |= 1ull << l;
          if (lane == l) mate[p] = j;
        }
      }
    }
  }
}

// The alignment of the prefix of m words, from scratch: the number of matches and of chunks.
template <int NQ>
__device__ __forceinline__ void align_prefix(int m, int nq, int lane, bool stems, bool syns, const int (&hw)[kP],
                                             const int (&hs)[kP], const u64 (*syn)[kQ], const int (&rw)[kQ],
                                             const int (&rs)[kQ], unsigned used, int& matches, int& chunks) {
  u64 matched[kP];
  int mate[kP];
#pragma unroll
  for (int p = 0; p < kP; ++p) {
    matched[p] = 0;
    mate[p] = -1;
  }
  match_stage<0, NQ>(m, nq, lane, hw, hs, syn, rw, rs, used, matched, mate);
  if (stems) match_stage<1, NQ>(m, nq, lane, hw, hs, syn, rw, rs, used, matched, mate);
  if (syns) match_stage<2, NQ>(m, nq, lane, hw, hs, syn, rw, rs, used, matched, mate);
  // the matches sorted by h: a match starts a chunk unless the word before it is matched to the position before its own
  int below = -1;
  matches = chunks = 0;
#pragma unroll
  for (int p = 0; p < kP; ++p) {
    if (p * WAVE < m) {
      const int j = ((matched[p] >> lane) & 1ull) ? mate[p] : -1;
      int jp = __shfl_up(j, 1, WAVE);
      if (lane == 0) jp = below;
      matches += __popcll(matched[p]);
      chunks += __popcll(__ballot(j >= 0 && !(jp >= 0 && j == jp + 1)));
      below = __builtin_amdgcn_readlane(j, WAVE - 1);
    }
  }
}

}  // namespace
