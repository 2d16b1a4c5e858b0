// Exact n-gram occurrence statistics of paragraphs (bmhrl_amd/evaluate.py paragraph_stats): a video's
// captions read in time order are one paragraph, and per paragraph and gram length n = 1..4 the kernel counts the
// occurrences, the distinct grams, the occurrences of a gram that occurs at least twice, the occurrences of a gram that an
// earlier sentence of the paragraph already holds, and the largest multiplicity.  A gram lies inside one sentence.
//
// One 256-thread workgroup per paragraph.  The paragraph's word ids are staged in LDS together with one word per token
// that packs the start of the token's sentence (paragraph-relative) and min(tokens left in the sentence, 4): a start i
// carries an n-gram exactly when that count is >= n, and an equal gram lies in an earlier sentence exactly when it
// starts before the start of i's sentence.  Wave w owns gram length w + 1 (a template parameter of its loop): lane l
// takes the starts l, l + 64, ... and compares its gram with the gram at every start j of the paragraph.  j is the same
// in every lane, so both LDS reads of a step are broadcasts, and the four words at j slide through registers.  Each lane
// keeps five integers; one wave reduction per gram length and lane 0 stores the row.  No atomics, and integers only:
// any order gives the same bits.
//
// T <= 1024 tokens per paragraph: at most 4 T^2 compares, 8 KB of LDS.
#include <vector>
#include "common.h"
#include "../../include/bmhrl_hip.h"

#pragma clang fp contract(off)

#include "caption_text.h"                // kMaxN

#define S_(x) ((hipStream_t)(x))

namespace {

constexpr int kThreads = 256;
constexpr int kMaxT = BMHRL_PARAGRAPH_MAX_TOKENS;
constexpr int kStats = BMHRL_NGRAM_STATS_INTS;
static_assert(kThreads == kMaxN * WAVE, "one wave per gram length");

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int u = __shfl_xor(v, o, 64);
    v = u > v ? u : v;
  }
  return v;
}

// the statistics of gram length N over the T staged tokens, by one wave; lane 0 stores out[0, kStats)
template <int N>
__device__ __forceinline__ void gram_stats(const int* s_tok, const int* s_meta, int T, int lane, int32_t* __restrict__ out) {
  int total = 0, distinct = 0, repeated = 0, cross = 0, max_count = 0;
  for (int base = 0; base < T; base += WAVE) {
    const int i = base + lane;
    const int m = i < T ? s_meta[i] : 0;     // 0: no gram starts here
    const bool valid = (m & 7) >= N;
    const int beg = m >> 3, at = i < T ? i : 0;
    const int a0 = s_tok[at], a1 = s_tok[at + 1], a2 = s_tok[at + 2], a3 = s_tok[at + 3];
    int count = 0, before = 0, earlier = 0;
    int w0 = s_tok[0], w1 = s_tok[1], w2 = s_tok[2], w3 = s_tok[3], mj = s_meta[0];
    // j, and so every LDS address below, is the same in all lanes; both reads are for a later step.  Not unrolled: the
    // unrolled loop keeps every step's compare masks in scalar registers and spills them
#pragma nounroll
    for (int j = 0; j < T; ++j) {
      const bool eq = ((mj & 7) >= N) & (w0 == a0) & ((N < 2) | (w1 == a1)) & ((N < 3) | (w2 == a2)) &
                      ((N < 4) | (w3 == a3));
      count += eq;
      before |= eq & (j < i);
      earlier |= eq & (j < beg);
      w0 = w1;
      w1 = w2;
      w2 = w3;
      w3 = s_tok[j + 4];                     // at most T + 3: inside the padding
      mj = s_meta[j + 1];                    // at most T: the padding word
    }
    if (valid) {
      ++total;
      distinct += !before;
      repeated += count >= 2;
      cross += earlier;
      max_count = count > max_count ? count : max_count;
    }
  }
  total = wave_sum_i(total);
  distinct = wave_sum_i(distinct);
  repeated = wave_sum_i(repeated);
  cross = wave_sum_i(cross);
  max_count = wave_max_i(max_count);
  if (lane == 0) {
    out[0] = total;
    out[1] = distinct;
    out[2] = repeated;
    out[3] = cross;
    out[4] = max_count;
  }
}

__global__ __launch_bounds__(kThreads) void ngram_stats_kernel(
    const int32_t* __restrict__ tok, int n_tok, const int32_t* __restrict__ sent_off, int S,
    const int32_t* __restrict__ para_off, int32_t* __restrict__ stats) {
  __shared__ int s_tok[kMaxT + kMaxN];      // the word ids (+ the padding the sliding window reads)
  __shared__ int s_meta[kMaxT + 1];         // (start of the token's sentence) << 3 | min(tokens left in the sentence, 4)

  const int g = blockIdx.x, tid = threadIdx.x;
  // the host has checked the offsets; the clamps keep every index in range whatever the device copy holds
  const int p0 = clampi(para_off[g], 0, S), p1 = clampi(para_off[g + 1], p0, S);
  const int t0 = clampi(sent_off[p0], 0, n_tok), t1 = clampi(sent_off[p1], t0, n_tok);
  const int T = p1 > p0 ? (t1 - t0 < kMaxT ? t1 - t0 : kMaxT) : 0;

  if (tid < kMaxN) s_tok[T + tid] = 0;       // never part of a gram: the validity test masks it
  if (tid == 0) s_meta[T] = 0;
  for (int t = tid; t < T; t += kThreads) {
    s_tok[t] = tok[t0 + t];
    // the sentence of token t: the last s in [p0, p1) with sent_off[s] <= t0 + t (behind every empty sentence there)
    int lo = p0, hi = p1 - 1;
    while (lo < hi) {
      const int mid = lo + ((hi - lo + 1) >> 1);
      if (sent_off[mid] <= t0 + t) lo = mid; else hi = mid - 1;
    }
    const int beg = clampi(sent_off[lo] - t0, 0, t), end = clampi(sent_off[lo + 1] - t0, t + 1, T);
    s_meta[t] = beg << 3 | (end - t < kMaxN ? end - t : kMaxN);
  }
  __syncthreads();

  const int wave = tid >> 6, lane = tid & (WAVE - 1);
  int32_t* out = stats + ((size_t)g * kMaxN + wave) * kStats;
  switch (wave) {
    case 0: gram_stats<1>(s_tok, s_meta, T, lane, out); break;
    case 1: gram_stats<2>(s_tok, s_meta, T, lane, out); break;
    case 2: gram_stats<3>(s_tok, s_meta, T, lane, out); break;
    default: gram_stats<4>(s_tok, s_meta, T, lane, out); break;
  }
}

}  // namespace

extern "C" int bmhrl_ngram_stats(const int32_t* tok, int32_t n_tok, const int32_t* sent_off, int32_t S,
                                 const int32_t* para_off, int32_t G, int32_t* stats, bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(sent_off && para_off && stats && (tok || n_tok == 0));
  BMHRL_CHECK_ARG(G > 0 && S >= 0 && n_tok >= 0);
  // the offsets decide which words a workgroup reads: they are checked here, before the launch (two small copies back)
  std::vector<int32_t> so((size_t)S + 1), po((size_t)G + 1);
  hipError_t e = hipMemcpyAsync(so.data(), sent_off, so.size() * sizeof(int32_t), hipMemcpyDeviceToHost, S_(stream));
  if (e == hipSuccess)
    e = hipMemcpyAsync(po.data(), para_off, po.size() * sizeof(int32_t), hipMemcpyDeviceToHost, S_(stream));
  if (e == hipSuccess) e = hipStreamSynchronize(S_(stream));
  if (e != hipSuccess) return hip_status(e);
  BMHRL_CHECK_ARG(so[0] == 0 && so[S] == n_tok && po[0] == 0 && po[G] == S);
  for (int s = 0; s < S; ++s) BMHRL_CHECK_ARG(so[s] <= so[s + 1]);
  for (int g = 0; g < G; ++g) BMHRL_CHECK_ARG(po[g] <= po[g + 1]);
  for (int g = 0; g < G; ++g) BMHRL_CHECK_ARG(so[po[g + 1]] - so[po[g]] <= kMaxT);
  hipLaunchKernelGGL(ngram_stats_kernel, dim3(G), dim3(kThreads), 0, S_(stream), tok, (int)n_tok, sent_off, (int)S, para_off,
                     stats);
  return hip_status(hipGetLastError());
}
