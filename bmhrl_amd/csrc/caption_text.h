// Stages the caption-scoring kernels share: rewards.hip, caption_eval.hip, meteor.hip and soda.hip (the last two also share
// the alignment, meteor_align.h).
//
// Include it after common.h and include/bmhrl_hip.h, inside a file that has set `#pragma clang fp contract(off)`.
#pragma once

namespace {

constexpr int kMaxL = BMHRL_REWARDS_MAX_L;
constexpr int kMaxR = BMHRL_REWARDS_MAX_R;
constexpr int kMaxN = 4;               // longest gram

// words a[0, k) == b[0, k): all four words are read (the word arrays carry kMaxN words of padding), no early exit
__device__ __forceinline__ bool gram_eq(const int* a, const int* b, int k) {
  bool eq = true;
#pragma unroll
  for (int q = 0; q < kMaxN; ++q) eq &= q >= k || a[q] == b[q];
  return eq;
}

// the last g in [0, G) with off[g] <= x (off ascends from 0; x < off[G])
__device__ __forceinline__ int group_of(const int32_t* __restrict__ off, int G, int x) {
  int lo = 0, hi = G - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= x) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// METEOR's hypothesis in LDS: what every token brings along, and the same of the words the tokens yield.  16-byte aligned
// as separate LDS arrays are, so that reads of neighbouring words still combine into wide LDS loads.
struct alignas(16) HypWords {
  int tw[kMaxL], ts[kMaxL], tb[kMaxL], te[kMaxL];   // per token: word id (-1: none), stem id, synonym row
  int mc[kMaxL];                                    // words among tokens [0, t]
  int hw[kMaxL], hs[kMaxL], hb[kMaxL], he[kMaxL];   // the same of the compacted hypothesis words
};

// Every token's word id, stem id and synonym row bounds are fetched in one pass, so that the vocabulary tables are read
// once, and the words are compacted into hw[0, M), M = mc[L - 1].  Called by all nthreads threads of the workgroup; both
// barriers are workgroup barriers, and what a caller wrote to LDS before the call is visible after it.
__device__ __forceinline__ void stage_hyp_words(HypWords& s, const int64_t* __restrict__ hyp_row, int L, int nthreads,
                                                const int32_t* __restrict__ vmap, const int32_t* __restrict__ vstem, int V,
                                                const int32_t* __restrict__ syn_off, int n_syn) {
  const int tid = threadIdx.x;
  for (int t = tid; t < L; t += nthreads) {
    const long v = (long)hyp_row[t];
    const bool ok = v >= 0 && v < V;
    s.tw[t] = ok ? vmap[v] : -1;
    s.ts[t] = ok && vstem ? vstem[v] : -1;
    int beg = ok && syn_off ? syn_off[v] : 0, end = ok && syn_off ? syn_off[v + 1] : 0;
    beg = beg < 0 ? 0 : beg;
    end = end > n_syn ? n_syn : end;
    s.tb[t] = beg;
    s.te[t] = end;
  }
  __syncthreads();
  for (int t = tid; t < L; t += nthreads) {
    int c = 0;
    for (int j = 0; j <= t; ++j) c += s.tw[j] >= 0;
    s.mc[t] = c;
    if (s.tw[t] >= 0) {
      s.hw[c - 1] = s.tw[t];
      s.hs[c - 1] = s.ts[t];
      s.hb[c - 1] = s.tb[t];
      s.he[c - 1] = s.te[t];
    }
  }
  __syncthreads();
}

// METEOR of m hypothesis words against Rb reference words from the alignment's counts, fp64, in the order of the
// reference's Python arithmetic
__device__ __forceinline__ double meteor_score(int matches, int chunks, int m, int Rb, double alpha, double beta,
                                               double gamma) {
  double score = 0.0;
  if (matches > 0) {
    const double p = (double)matches / (double)m, r = (double)matches / (double)Rb;
    const double den = alpha * p + (1.0 - alpha) * r;
    if (den != 0.0) {
      const double fmean = (p * r) / den;
      const double frag = (double)chunks / (double)matches;
      const double penalty = gamma * pow(frag, beta);
      score = (1.0 - penalty) * fmean;
    }
  }
  return score;
}

}  // namespace
