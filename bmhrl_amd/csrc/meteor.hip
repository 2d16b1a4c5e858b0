// Per-prefix METEOR rewards of sampled captions (bmhrl_amd/rewards.py MeteorScorer): the score row the reference builds by
// calling nltk's single_meteor_score on every prefix of every sampled caption on the host (metrics/batched_meteor.py
// _meteor_diff), as one launch that a captured RL step can hold.  The rules are in DESIGN.md section 19.
//
// Strings never reach the device: the stem of a word and its synonym set depend on the vocabulary alone, so the host hands
// over vmap (vocab id -> word id), vstem (vocab id -> stem id) and the synonym sets as CSR rows of word ids over vocab ids.
//
// One 1024-thread workgroup (16 waves) per sample.  Every token's word id, stem id and synonym row bounds are fetched in one
// pass and compacted into the word sequence hw[0, M) in LDS; the reference words and stems are staged next to them.  A
// prefix's score depends only on the number m of words in it, so the kernel scores m = 1..M once and spreads the row over
// the token positions.  The alignment of a prefix is NOT the restriction of the next prefix's alignment (the walk starts at
// the prefix's own last word), so every prefix is aligned from scratch: a wave takes one prefix at a time, and the prefixes
// are dealt to the waves back and forth (1..16, then 32..17, ...), so that every wave gets about the same number of words.
//
// All per-prefix state is in registers.  The lanes of a wave hold the reference positions j = 64 q + lane (kQ = R/64 per
// lane: word, stem and a "used" bit) and the hypothesis words h = 64 p + lane (kP = L/64 per lane: word, stem, and the
// reference position the word was matched to).  Which words are matched is a wave-uniform bit mask.  For every stage
// (exact, stem, synonym) the wave walks the set bits of "h < m and unmatched" from the top; the word's key comes out of its
// lane by readlane, the lanes test their unused reference positions, a ballot per 64 positions from the top picks the
// highest j, and the owning lanes mark it used and record it (a reference of at most 64 words takes a body without the loop
// over the groups of 64).  The chunk count compares every lane's match with its lower neighbour's.  Which reference positions a word's synonym set (or the word itself) selects does not depend on the prefix:
// it is evaluated once per word as a bit mask over the reference (syn[h][q], ballots, in LDS) before the prefixes start, so
// the CSR rows are searched M times and not M^2 / 2 times.
//
// Contraction to FMA is off in this file: every product and sum rounds as the reference's Python arithmetic does.
#include <math.h>
#include "common.h"
#include "../../include/bmhrl_hip.h"

#pragma clang fp contract(off)

#include "meteor_align.h"                // align_prefix and, through caption_text.h, the staging and the score: shared with soda.hip

#define S_(x) ((hipStream_t)(x))

namespace {

constexpr int kWaves = 16;
constexpr int kThreads = kWaves * WAVE;

__global__ __launch_bounds__(kThreads) void meteor_kernel(
    const int64_t* __restrict__ hyp, long ldh, const int32_t* __restrict__ vmap, const int32_t* __restrict__ vstem, int V,
    const int32_t* __restrict__ syn_off, const int32_t* __restrict__ syn_ids, int n_syn, const int32_t* __restrict__ ref,
    const int32_t* __restrict__ ref_stem, long ldr, const int32_t* __restrict__ ref_len, double alpha, double beta,
    double gamma, int L, int R, double* __restrict__ scores, long lds, float* __restrict__ delta, long ldd) {
  __shared__ HypWords s_h;                                // the tokens and the compacted hypothesis words (caption_text.h)
  __shared__ int s_rw[kMaxR], s_rs[kMaxR];                // the reference: word ids, stem ids
  __shared__ u64 s_syn[kMaxL][kQ];                        // reference positions the synonym test of word h selects
  __shared__ double s_score[kMaxL + 1];

  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE);
  const int Rb = clampi(ref_len[b], 0, R);
  for (int r = tid; r < Rb; r += kThreads) {
    s_rw[r] = ref[(size_t)b * ldr + r];
    s_rs[r] = vstem ? ref_stem[(size_t)b * ldr + r] : -1;
  }
  if (tid == 0) s_score[0] = 0.0;
  // (the helper's first barrier covers the reference words and s_score[0] above)
  stage_hyp_words(s_h, hyp + (size_t)b * ldh, L, kThreads, vmap, vstem, V, syn_off, n_syn);
  const int M = __builtin_amdgcn_readfirstlane(s_h.mc[L - 1]);
  const int nq = (Rb + WAVE - 1) / WAVE;

  // this lane's reference positions (those behind the reference start out used) and hypothesis words
  int rw[kQ], rs[kQ], hw[kP], hs[kP];
  unsigned used0 = 0;
#pragma unroll
  for (int q = 0; q < kQ; ++q) {
    const int r = q * WAVE + lane;
    const bool ok = r < Rb;
    rw[q] = ok ? s_rw[r] : -1;
    rs[q] = ok ? s_rs[r] : -1;
    used0 |= ok ? 0u : 1u << q;
  }
#pragma unroll
  for (int p = 0; p < kP; ++p) {
    const int h = p * WAVE + lane;
    hw[p] = h < M ? s_h.hw[h] : -1;
    hs[p] = h < M ? s_h.hs[h] : -1;
  }

  if (syn_off && Rb > 0) {
    // 64 ids of a row per load, one per lane; the first load of the wave's next word is in flight while this one is searched
    int nbeg = 0, nend = 0, nmine = -1;
    if (wave < M) {
      nbeg = __builtin_amdgcn_readfirstlane(s_h.hb[wave]);
      nend = __builtin_amdgcn_readfirstlane(s_h.he[wave]);
      nmine = nbeg + lane < nend ? syn_ids[nbeg + lane] : -1;
    }
    for (int h = wave; h < M; h += kWaves) {
      const int w = __builtin_amdgcn_readfirstlane(s_h.hw[h]), beg = nbeg, end = nend;
      int mine = nmine;
      if (h + kWaves < M) {
        nbeg = __builtin_amdgcn_readfirstlane(s_h.hb[h + kWaves]);
        nend = __builtin_amdgcn_readfirstlane(s_h.he[h + kWaves]);
        nmine = nbeg + lane < nend ? syn_ids[nbeg + lane] : -1;
      }
      bool hit[kQ];
#pragma unroll
      for (int q = 0; q < kQ; ++q) hit[q] = rw[q] == w;
      for (int e0 = beg; e0 < end; e0 += WAVE) {
        if (e0 > beg) mine = e0 + lane < end ? syn_ids[e0 + lane] : -1;
        const int n = end - e0 < WAVE ? end - e0 : WAVE;
        for (int i = 0; i < n; ++i) {
          const int id = __builtin_amdgcn_readlane(mine, i);
#pragma unroll
          for (int q = 0; q < kQ; ++q) hit[q] |= rw[q] == id;
        }
      }
#pragma unroll
      for (int q = 0; q < kQ; ++q) {
        const u64 bal = __ballot(hit[q] && !((used0 >> q) & 1u));
        if (lane == 0) s_syn[h][q] = bal;
      }
    }
  }
  __syncthreads();

  for (int k = 0; k * kWaves < M; ++k) {
    const int m = k * kWaves + ((k & 1) ? kWaves - 1 - wave : wave) + 1;
    if (m > M) continue;
    double score = 0.0;
    if (Rb > 0) {
      int matches, chunks;
      if (nq == 1)
        align_prefix<1>(m, nq, lane, vstem != nullptr, syn_off != nullptr, hw, hs, s_syn, rw, rs, used0, matches, chunks);
      else
        align_prefix<kQ>(m, nq, lane, vstem != nullptr, syn_off != nullptr, hw, hs, s_syn, rw, rs, used0, matches, chunks);
      score = meteor_score(matches, chunks, m, Rb, alpha, beta, gamma);
    }
    if (lane == 0) s_score[m] = score;
  }
  __syncthreads();

  // the row over token positions: a token that yields no word repeats the score before it.  The reference keeps the row
  // in float32, so the differences are taken in float32.
  for (int t = tid; t < L; t += kThreads) {
    const double cur = s_score[s_h.mc[t]];
    scores[(size_t)b * lds + t] = cur;
    delta[(size_t)b * ldd + t] = t == 0 ? (float)cur : (float)cur - (float)s_score[s_h.mc[t - 1]];
  }
}

}  // namespace

extern "C" int bmhrl_meteor(const int64_t* hyp, int64_t ldh, const int32_t* vmap, const int32_t* vstem, int32_t V,
                            const int32_t* syn_off, const int32_t* syn_ids, int32_t n_syn, const int32_t* ref,
                            const int32_t* ref_stem, int64_t ldr, const int32_t* ref_len, double alpha, double beta,
                            double gamma, int32_t B, int32_t L, int32_t R, double* scores, int64_t lds, float* delta,
                            int64_t ldd, bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(hyp && vmap && ref && ref_len && scores && delta);
  BMHRL_CHECK_ARG(!vstem || ref_stem);
  BMHRL_CHECK_ARG((syn_off != nullptr) == (syn_ids != nullptr));
  BMHRL_CHECK_ARG(!syn_off || n_syn >= 0);
  BMHRL_CHECK_ARG(B > 0 && L >= 1 && L <= kMaxL && R >= 1 && R <= kMaxR && V >= 1);
  BMHRL_CHECK_ARG(ldh >= L && ldr >= R && lds >= L && ldd >= L);
  hipLaunchKernelGGL(meteor_kernel, dim3(B), dim3(kThreads), 0, S_(stream), hyp, (long)ldh, vmap, vstem, V, syn_off, syn_ids,
                     n_syn, ref, ref_stem, (long)ldr, ref_len, alpha, beta, gamma, L, R, scores, (long)lds, delta, (long)ldd);
  return hip_status(hipGetLastError());
}
