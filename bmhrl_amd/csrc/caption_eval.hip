// Evaluation forms of the caption metrics (bmhrl_amd/evaluate.py DenseCaptionEvaluator): what the
// reference's evaluation/evaluate.py asks of pycocoevalcap's Bleu, Rouge and Cider for every video -- corpus BLEU over the
// video's (prediction, reference) pairs, the mean ROUGE-L and the mean CIDEr with document frequencies taken from those
// same pairs -- as two launches with nothing read back between them.  The pairs of a video (a group) are contiguous.
//
// Launch 1, one 256-thread workgroup per pair: the pair's words are staged in LDS.  One work item per (gram length, start
// position) finds whether the gram is the first occurrence of itself, its count in the hypothesis and in the reference
// (BLEU's clipped matches, CIDEr's term frequencies).  The document frequency of every distinct gram -- the number of
// pairs of the group whose reference holds it -- is counted by scanning the references of the whole group out of global
// memory (the scan position is the same for every lane, so the loads are wave-uniform); nothing about the group is kept
// in LDS or assumed to fit a workgroup, so a group may hold any number of pairs and distinct grams.  The LCS length is an
// anti-diagonal wavefront: lane i owns hypothesis word i, one step per diagonal.  The CIDEr sums run over the distinct
// grams in first-occurrence order, the order the reference's dicts iterate in.
//
// Launch 2, one workgroup per group: integer sums of the BLEU counts (any order: exact), then the BLEU formula; the
// ROUGE-L and CIDEr means are summed in pair order by one lane each, so two runs give equal bits.
//
// Contraction to FMA is off in this file: every product and sum rounds as the reference's Python arithmetic does.
#include <math.h>
#include <vector>
#include "common.h"
#include "../../include/bmhrl_hip.h"

#pragma clang fp contract(off)

#include "caption_text.h"                // kMaxL, kMaxR, kMaxN, gram_eq (shared with rewards.hip), group_of (with soda.hip)

#define S_(x) ((hipStream_t)(x))

namespace {

constexpr int kThreads = 256;
constexpr int kInts = BMHRL_CAPTION_EVAL_PAIR_INTS;
constexpr int kOuts = BMHRL_CAPTION_EVAL_GROUP_SCORES;

// the number of pairs in [g0, g1) whose reference holds the gram a[0, k).  Word ids are >= 0; the window behind a
// reference's end holds -1, so a gram never matches across it.  q and j are the same in every lane.
__device__ int gram_doc_freq(const int* a, int k, const int32_t* __restrict__ ref, long ldr,
                             const int32_t* __restrict__ ref_len, int R, int g0, int g1) {
  const int a0 = a[0], a1 = a[1], a2 = a[2], a3 = a[3];
  int df = 0;
  for (int q = g0; q < g1; ++q) {
    const int Rq = clampi(ref_len[q], 0, R);
    const int32_t* row = ref + (size_t)q * ldr;
    int w0 = Rq > 0 ? row[0] : -1, w1 = Rq > 1 ? row[1] : -1, w2 = Rq > 2 ? row[2] : -1, w3 = Rq > 3 ? row[3] : -1;
    bool found = false;
    for (int j = 0; j < Rq; ++j) {
      found |= (w0 == a0) & ((k < 2) | (w1 == a1)) & ((k < 3) | (w2 == a2)) & ((k < 4) | (w3 == a3));
      w0 = w1;
      w1 = w2;
      w2 = w3;
      w3 = j + 4 < Rq ? row[j + 4] : -1;
    }
    df += found;
  }
  return df;
}

__global__ __launch_bounds__(kThreads) void caption_pair_kernel(
    const int32_t* __restrict__ hyp, long ldh, const int32_t* __restrict__ hyp_len, const int32_t* __restrict__ ref,
    long ldr, const int32_t* __restrict__ ref_len, const int32_t* __restrict__ group_off, int P, int G, int L, int R,
    int32_t* __restrict__ pair_ints, int32_t* __restrict__ pair_lcs, double* __restrict__ pair_cider) {
  __shared__ int s_hw[kMaxL + kMaxN];       // the hypothesis words (+ padding read by gram_eq)
  __shared__ int s_rw[kMaxR + kMaxN];       // the reference words (+ padding)
  __shared__ int s_hcnt[kMaxN][kMaxL];      // count in the hypothesis of the gram starting here (0: not its first occurrence)
  __shared__ int s_htr[kMaxN][kMaxL];       // count in the reference of the same gram
  __shared__ int s_hdf[kMaxN][kMaxL];       // document frequency of the same gram
  __shared__ int s_rcnt[kMaxN][kMaxR];      // the same for the reference's grams
  __shared__ int s_rdf[kMaxN][kMaxR];
  __shared__ int s_diag[3][kMaxL + 1];      // LCS: the last three anti-diagonals, row i at index i + 1
  __shared__ double s_val[kMaxN], s_nh[kMaxN], s_nr[kMaxN];
  __shared__ int s_g0, s_g1, s_lcs;

  const int p = blockIdx.x, tid = threadIdx.x;
  const int M = clampi(hyp_len[p], 0, L), Rb = clampi(ref_len[p], 0, R);
  if (tid == 0) {
    const int g = group_of(group_off, G, p);  // the group of this pair
    s_g0 = clampi(group_off[g], 0, P);
    s_g1 = clampi(group_off[g + 1], 0, P);
    s_lcs = 0;
  }
  if (tid < kMaxN) s_hw[M + tid] = s_rw[Rb + tid] = -1;
  for (int t = tid; t < M; t += kThreads) s_hw[t] = hyp[(size_t)p * ldh + t];
  for (int r = tid; r < Rb; r += kThreads) s_rw[r] = ref[(size_t)p * ldr + r];
  for (int i = tid; i < 3 * (kMaxL + 1); i += kThreads) (&s_diag[0][0])[i] = 0;
  __syncthreads();
  const int g0 = s_g0, g1 = s_g1;

  // every gram length at once: work item q = (k - 1) * M + start position
  for (int q = tid; q < kMaxN * M; q += kThreads) {
    const int k = q / M + 1, i = q % M, Gh = M - k + 1, Gr = Rb - k + 1;
    int th = 0, tr = 0;
    if (i < Gh) {
      const int* g = s_hw + i;
      bool first = true;
      for (int j = 0; j < i; ++j) first &= !gram_eq(s_hw + j, g, k);
      if (first) {
        for (int j = i; j < Gh; ++j) th += gram_eq(s_hw + j, g, k);
        for (int r = 0; r < Gr; ++r) tr += gram_eq(s_rw + r, g, k);
      }
    }
    s_hcnt[k - 1][i] = th;
    s_htr[k - 1][i] = tr;
  }
  for (int q = tid; q < kMaxN * Rb; q += kThreads) {
    const int k = q / Rb + 1, r = q % Rb, Gr = Rb - k + 1;
    int cnt = 0;
    if (r < Gr) {
      const int* g = s_rw + r;
      bool first = true;
      for (int j = 0; j < r; ++j) first &= !gram_eq(s_rw + j, g, k);
      if (first)
        for (int j = r; j < Gr; ++j) cnt += gram_eq(s_rw + j, g, k);
    }
    s_rcnt[k - 1][r] = cnt;
  }
  __syncthreads();

  // document frequencies of the distinct grams of both sides, over the references of the whole group
  for (int q = tid; q < kMaxN * (M + Rb); q += kThreads) {
    if (q < kMaxN * M) {
      const int k = q / M + 1, i = q % M;
      s_hdf[k - 1][i] = s_hcnt[k - 1][i] ? gram_doc_freq(s_hw + i, k, ref, ldr, ref_len, R, g0, g1) : 0;
    } else {
      const int q2 = q - kMaxN * M, k = q2 / Rb + 1, r = q2 % Rb;
      s_rdf[k - 1][r] = s_rcnt[k - 1][r] ? gram_doc_freq(s_rw + r, k, ref, ldr, ref_len, R, g0, g1) : 0;
    }
  }

  // LCS length: lane i holds c(i, j - 1) in `left`; c(i - 1, j) and c(i - 1, j - 1) come from the two diagonals before
  {
    int left = 0;
    const int hw = tid < M ? s_hw[tid] : -2;
    const int steps = (M > 0 && Rb > 0) ? M + Rb - 1 : 0;
    for (int d = 0; d < steps; ++d) {
      int* cur = s_diag[d % 3];
      const int* p1 = s_diag[(d + 2) % 3];
      const int* p2 = s_diag[(d + 1) % 3];
      const int j = d - tid;
      if (tid < M && j >= 0 && j < Rb) {
        const int up = p1[tid], dg = j > 0 ? p2[tid] : 0;
        const int v = hw == s_rw[j] ? dg + 1 : (up > left ? up : left);
        cur[tid + 1] = v;
        left = v;
      }
      __syncthreads();
    }
    if (steps > 0 && tid == M - 1) s_lcs = left;
  }
  __syncthreads();

  const double rl = log((double)(g1 - g0));   // log of the number of pairs (the group holds this pair: >= 1)
  if (tid < kMaxN) {                          // the hypothesis side of gram length tid + 1, in first-occurrence order
    const int k = tid;
    double nh2 = 0.0, val = 0.0;
    int correct = 0;
    for (int i = 0; i < M - k; ++i) {
      const int th = s_hcnt[k][i], tr = s_htr[k][i];
      if (!th) continue;
      correct += th < tr ? th : tr;
      const double df = (double)s_hdf[k][i];
      const double w = rl - log(df > 1.0 ? df : 1.0);
      const double vh = (double)th * w, vr = (double)tr * w;
      nh2 += vh * vh;
      val += (vr < vh ? vr : vh) * vr;
    }
    s_val[k] = val;
    s_nh[k] = sqrt(nh2);
    pair_ints[(size_t)p * kInts + k] = M - k > 0 ? M - k : 0;       // guess
    pair_ints[(size_t)p * kInts + kMaxN + k] = correct;
  } else if (tid >= 64 && tid < 64 + kMaxN) { // the reference norm of gram length tid - 63 (another wave)
    const int k = tid - 64;
    double nr2 = 0.0;
    for (int r = 0; r < Rb - k; ++r) {
      const int c = s_rcnt[k][r];
      if (!c) continue;
      const double df = (double)s_rdf[k][r];
      const double v = (double)c * (rl - log(df > 1.0 ? df : 1.0));
      nr2 += v * v;
    }
    s_nr[k] = sqrt(nr2);
  }
  __syncthreads();
  if (tid == 0) {
    const double sigma = 6.0;
    const double dl = (double)((M > 1 ? M - 1 : 0) - (Rb > 1 ? Rb - 1 : 0));   // the bigram counts
    const double pen = pow(M_E, -(dl * dl) / (2.0 * (sigma * sigma)));
    double s = 0.0;
    for (int k = 0; k < kMaxN; ++k) {
      double v = s_val[k];
      if (s_nh[k] != 0.0 && s_nr[k] != 0.0) v /= s_nh[k] * s_nr[k];
      v *= pen;
      s += v;
    }
    pair_cider[p] = s / (double)kMaxN * 10.0;
    pair_ints[(size_t)p * kInts + 8] = M;
    pair_ints[(size_t)p * kInts + 9] = Rb;
    pair_lcs[p] = s_lcs;
  }
}

__global__ __launch_bounds__(kThreads) void caption_group_kernel(
    const int32_t* __restrict__ pair_ints, const int32_t* __restrict__ pair_lcs, const double* __restrict__ pair_cider,
    const int32_t* __restrict__ group_off, int P, double* __restrict__ group_scores) {
  __shared__ int s_sum[kInts];
  __shared__ double s_rouge[kThreads], s_cider[kThreads];
  __shared__ double s_tot[2];
  const int g = blockIdx.x, tid = threadIdx.x;
  const int g0 = clampi(group_off[g], 0, P), g1 = clampi(group_off[g + 1], g0, P);
  if (tid < kInts) s_sum[tid] = 0;
  if (tid < 2) s_tot[tid] = 0.0;
  __syncthreads();
  int acc[kInts];
#pragma unroll
  for (int c = 0; c < kInts; ++c) acc[c] = 0;
  for (int p = g0 + tid; p < g1; p += kThreads) {
#pragma unroll
    for (int c = 0; c < kInts; ++c) acc[c] += pair_ints[(size_t)p * kInts + c];
  }
#pragma unroll
  for (int c = 0; c < kInts; ++c)
    if (acc[c]) atomicAdd(&s_sum[c], acc[c]);       // integers: the order does not matter
  const double b2 = 1.2 * 1.2;
  for (int base = g0; base < g1; base += kThreads) {
    const int p = base + tid;
    if (p < g1) {
      const int M = pair_ints[(size_t)p * kInts + 8], Rb = pair_ints[(size_t)p * kInts + 9], l = pair_lcs[p];
      double sc = 0.0;
      if (l > 0 && M > 0 && Rb > 0) {
        const double pr = (double)l / (double)M, rc = (double)l / (double)Rb;
        sc = ((1.0 + b2) * pr * rc) / (rc + b2 * pr);
      }
      s_rouge[tid] = sc;
      s_cider[tid] = pair_cider[p];
    }
    __syncthreads();
    const int n = g1 - base < kThreads ? g1 - base : kThreads;
    if (tid == 0 || tid == 64) {                    // pair order, one lane per metric (two waves)
      const double* v = tid == 0 ? s_rouge : s_cider;
      double t = s_tot[tid != 0];
      for (int i = 0; i < n; ++i) t += v[i];
      s_tot[tid != 0] = t;
    }
    __syncthreads();
  }
  __syncthreads();
  if (tid == 0) {
    double* out = group_scores + (size_t)g * kOuts;
    const int n = g1 - g0;
    if (n <= 0) {
      for (int c = 0; c < kOuts; ++c) out[c] = 0.0;
      return;
    }
    const double tiny = 1e-15, small = 1e-9;
    const double ratio = ((double)s_sum[8] + tiny) / ((double)s_sum[9] + small);
    double bl = 1.0;
    for (int k = 0; k < kMaxN; ++k) {
      bl *= ((double)s_sum[kMaxN + k] + tiny) / ((double)s_sum[k] + small);
      double bk = pow(bl, 1.0 / (double)(k + 1));
      if (ratio < 1.0) bk *= exp(1.0 - 1.0 / ratio);
      out[k] = bk;
    }
    out[4] = s_tot[0] / (double)n;
    out[5] = s_tot[1] / (double)n;
  }
}

}  // namespace

extern "C" int bmhrl_caption_eval(const int32_t* hyp, int64_t ldh, const int32_t* hyp_len, const int32_t* ref, int64_t ldr,
                                  const int32_t* ref_len, const int32_t* group_off, int32_t P, int32_t G, int32_t L,
                                  int32_t R, int32_t* pair_ints, int32_t* pair_lcs, double* pair_cider,
                                  double* group_scores, bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(hyp && hyp_len && ref && ref_len && group_off && pair_ints && pair_lcs && pair_cider && group_scores);
  BMHRL_CHECK_ARG(P > 0 && G > 0 && L >= 1 && L <= kMaxL && R >= 1 && R <= kMaxR && ldh >= L && ldr >= R);
  // the offsets decide which rows a workgroup reads: they are checked here, before the launches (one small copy back)
  std::vector<int32_t> off((size_t)G + 1);
  hipError_t e = hipMemcpyAsync(off.data(), group_off, off.size() * sizeof(int32_t), hipMemcpyDeviceToHost, S_(stream));
  if (e == hipSuccess) e = hipStreamSynchronize(S_(stream));
  if (e != hipSuccess) return hip_status(e);
  BMHRL_CHECK_ARG(off[0] == 0 && off[G] == P);
  for (int g = 0; g < G; ++g) BMHRL_CHECK_ARG(off[g] <= off[g + 1]);
  hipLaunchKernelGGL(caption_pair_kernel, dim3(P), dim3(kThreads), 0, S_(stream), hyp, (long)ldh, hyp_len, ref, (long)ldr,
                     ref_len, group_off, P, G, L, R, pair_ints, pair_lcs, pair_cider);
  e = hipGetLastError();
  if (e != hipSuccess) return hip_status(e);
  hipLaunchKernelGGL(caption_group_kernel, dim3(G), dim3(kThreads), 0, S_(stream), pair_ints, pair_lcs, pair_cider, group_off,
                     P, group_scores);
  return hip_status(hipGetLastError());
}
