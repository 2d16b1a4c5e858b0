// Per-prefix CIDEr / BLEU rewards of sampled captions (bmhrl_amd/rewards.py): the score row the reference's scorers build
// by scoring every prefix of every sampled caption on the host (metrics/cider.py _cider_diff, metrics/bleu.py _bleu_diff),
// as one launch that a captured RL step can hold.
//
// One 256-thread workgroup per sample.  The sample's tokens are mapped to word ids (vocab id -> word id, -1: the token
// yields no word) and compacted into the word sequence hw[0, M) in LDS (CIDEr: only the tokens before the first end
// token); the reference words ref[0, R_b) are staged next to them.  Prefix scores depend only on the number m of words in
// the prefix, so the kernel scores m = 0..M once and spreads the row over the token positions.
//
// For every gram length k at once (one work item per (k, position)), every hypothesis start position i gets, once:
// whether it is the first occurrence of its gram (first), the next start position of the same gram (next), the gram's
// count in the reference (tr) and, for CIDEr, its log document frequency from the device hash table (dh).  The count of
// a gram in the prefix of m words is the length of its `next` chain up to the last start m - k, so every (m, k) pair sums
// over the distinct grams in first-occurrence order -- the order the reference's dicts iterate in -- without any
// per-prefix table.  The reference side (count and idf of every distinct reference gram, the reference norm) is computed
// once per (sample, k).  Gram comparisons read all four words and the scans do not exit early, so their LDS reads issue
// back to back (the launch is latency-bound).  Everything is fp64; the BLEU average is formed in fp32 as the
// reference's torch.sum does.
//
// Contraction to FMA is off in this file: every product and sum rounds as the reference's Python arithmetic does.
#include <climits>
#include <math.h>
#include "common.h"
#include "../../include/bmhrl_hip.h"

#pragma clang fp contract(off)

#include "caption_text.h"                // kMaxL, kMaxR, kMaxN, gram_eq: shared with caption_eval.hip

#define S_(x) ((hipStream_t)(x))

namespace {

constexpr int kThreads = 256;

// the host's hash of a key of 4 word ids (bmhrl_amd/rewards.py _hash): uint32 arithmetic, wrap-around
__device__ __forceinline__ uint32_t gram_hash(const int32_t* w) {
  uint32_t h = (uint32_t)w[0] * 0x9E3779B1u ^ (uint32_t)w[1] * 0x85EBCA77u ^ (uint32_t)w[2] * 0xC2B2AE3Du ^
               (uint32_t)w[3] * 0x27D4EB2Fu;
  h ^= h >> 15;
  h *= 0x2C1B3C6Du;
  h ^= h >> 12;
  return h;
}

// log(max(1, df)) of the gram words[0, k): 0 when the table does not hold it (df <= 1).  Open addressing with linear
// probing; the table is at most half full, so the probe ends at an empty slot (key[0] = -1) within cap steps.
__device__ double gram_log_df(const int32_t* words, int k, const int32_t* __restrict__ keys, const double* __restrict__ logs,
                              int cap) {
  int32_t w[4] = {-1, -1, -1, -1};
  for (int q = 0; q < k; ++q) w[q] = words[q];
  uint32_t slot = gram_hash(w) & (uint32_t)(cap - 1);
  for (int probe = 0; probe < cap; ++probe) {
    const int32_t* key = keys + 4 * (size_t)slot;
    const int32_t k0 = key[0];
    if (k0 == -1) return 0.0;
    if (k0 == w[0] && key[1] == w[1] && key[2] == w[2] && key[3] == w[3]) return logs[slot];
    slot = (slot + 1) & (uint32_t)(cap - 1);
  }
  return 0.0;
}

__global__ __launch_bounds__(kThreads) void rewards_kernel(
    const int64_t* __restrict__ hyp, long ldh, const int32_t* __restrict__ vmap, int V, long eos,
    const int32_t* __restrict__ ref, long ldr, const int32_t* __restrict__ ref_len, const int32_t* __restrict__ df_keys,
    const double* __restrict__ df_logs, int df_cap, int metric, int nmax, double sigma, int L, int R,
    double* __restrict__ scores, long lds, float* __restrict__ delta, long ldd) {
  __shared__ int s_tok[kMaxL];          // word id of each token (-1: none)
  __shared__ int s_mc[kMaxL];           // words among tokens [0, t]
  __shared__ int s_hw[kMaxL + kMaxN];   // the compacted hypothesis words (+ padding read by gram_eq)
  __shared__ int s_rw[kMaxR + kMaxN];   // the reference words (+ padding)
  __shared__ int s_first[kMaxN][kMaxL], s_next[kMaxN][kMaxL], s_tr[kMaxN][kMaxL];   // per gram length k - 1
  __shared__ double s_dh[kMaxN][kMaxL];
  __shared__ double s_rc[kMaxN][kMaxR];  // squared reference weights (CIDEr), in reference position order
  __shared__ double s_val[kMaxL + 1][kMaxN];   // CIDEr: val[k] of the prefix of m words
  __shared__ int s_cor[kMaxL + 1][kMaxN];      // BLEU: clipped matches of the prefix of m words
  __shared__ double s_score[kMaxL + 1];
  __shared__ double s_normr[kMaxN];
  __shared__ int s_eos;

  const int b = blockIdx.x, tid = threadIdx.x;
  const bool cider = metric == BMHRL_REWARD_CIDER;
  const int Rb = clampi(ref_len[b], 0, R);
  if (tid == 0) s_eos = L;
  if (tid < kMaxN) s_hw[kMaxL + tid] = s_rw[kMaxR + tid] = -1;
  __syncthreads();
  for (int t = tid; t < L; t += kThreads) {
    const long v = (long)hyp[(size_t)b * ldh + t];
    s_tok[t] = (v >= 0 && v < V) ? vmap[v] : -1;
    if (cider && v == eos) atomicMin(&s_eos, t);
  }
  for (int r = tid; r < Rb; r += kThreads) s_rw[r] = ref[(size_t)b * ldr + r];
  __syncthreads();
  const int E = s_eos;                  // tokens [0, E) are scored
  for (int t = tid; t < L; t += kThreads) {
    const int last = t < E ? t : E - 1;
    int c = 0;
    for (int j = 0; j <= last; ++j) c += s_tok[j] >= 0;
    s_mc[t] = c;
    if (t < E && s_tok[t] >= 0) s_hw[c - 1] = s_tok[t];
  }
  __syncthreads();
  const int M = E > 0 ? s_mc[E - 1] : 0;

  // every gram length at once: work item q = (k - 1) * L + start position
  for (int q = tid; q < nmax * L; q += kThreads) {
    const int k = q / L + 1, i = q % L, Gh = M - k + 1, Gr = Rb - k + 1;
    if (i >= Gh) continue;
    const int* g = s_hw + i;
    bool first = true;
    int nxt = INT_MAX, tr = 0;
    for (int j = 0; j < i; ++j) first &= !gram_eq(s_hw + j, g, k);
    for (int j = Gh - 1; j > i; --j) nxt = gram_eq(s_hw + j, g, k) ? j : nxt;
    if (first) {
      for (int r = 0; r < Gr; ++r) tr += gram_eq(s_rw + r, g, k);
      s_dh[k - 1][i] = cider ? gram_log_df(g, k, df_keys, df_logs, df_cap) : 0.0;
    }
    s_first[k - 1][i] = first;
    s_next[k - 1][i] = nxt;
    s_tr[k - 1][i] = tr;
  }
  if (cider) {
    for (int q = tid; q < nmax * R; q += kThreads) {
      const int k = q / R + 1, r = q % R, Gr = Rb - k + 1;
      if (r >= Gr) continue;
      const int* g = s_rw + r;
      bool first = true;
      int cnt = 1;
      for (int j = 0; j < r; ++j) first &= !gram_eq(s_rw + j, g, k);
      double c2 = 0.0;
      if (first) {
        for (int j = r + 1; j < Gr; ++j) cnt += gram_eq(s_rw + j, g, k);
        const double w = (double)cnt * (0.0 - gram_log_df(g, k, df_keys, df_logs, df_cap));
        c2 = w * w;
      }
      s_rc[k - 1][r] = c2;
    }
  }
  __syncthreads();
  if (cider && tid < nmax) {            // the reference norms, summed in reference position order
    double n2 = 0.0;
    for (int r = 0; r < Rb - tid; ++r) n2 += s_rc[tid][r];
    s_normr[tid] = sqrt(n2);
  }
  __syncthreads();
  // work item q = (k - 1) * (M + 1) + m: gram length k over the prefix of m words
  for (int q = tid; q < nmax * (M + 1); q += kThreads) {
    const int k = q / (M + 1) + 1, m = q % (M + 1);
    const int* first = s_first[k - 1];
    const int* next = s_next[k - 1];
    const int* trk = s_tr[k - 1];
    const int p = m - k;                // last start position inside the prefix
    if (cider) {
      double val = 0.0, nh2 = 0.0;
      for (int i = 0; i <= p; ++i) {
        if (!first[i]) continue;
        int th = 0;
        for (int j = i; j <= p; j = next[j]) ++th;
        const double d = s_dh[k - 1][i];
        const double vh = (double)th * (0.0 - d), vr = (double)trk[i] * (0.0 - d);
        nh2 += vh * vh;
        val += (vr < vh ? vr : vh) * vr;
      }
      const double nh = sqrt(nh2), nr = s_normr[k - 1];
      if (nh != 0.0 && nr != 0.0) val /= nh * nr;
      const int lh = nmax >= 2 ? (m > 1 ? m - 1 : 0) : 0, lr = nmax >= 2 ? (Rb > 1 ? Rb - 1 : 0) : 0;
      const double dl = (double)(lh - lr);
      val *= pow(M_E, -(dl * dl) / (2.0 * (sigma * sigma)));
      s_val[m][k - 1] = val;
    } else {
      int cor = 0;
      for (int i = 0; i <= p; ++i) {
        if (!first[i]) continue;
        int th = 0;
        for (int j = i; j <= p; j = next[j]) ++th;
        cor += th < trk[i] ? th : trk[i];
      }
      s_cor[m][k - 1] = cor;
    }
  }
  __syncthreads();

  for (int m = tid; m <= M; m += kThreads) {
    double sc;
    if (cider) {
      double s = 0.0;
      for (int k = 0; k < nmax; ++k) s += s_val[m][k];
      sc = s / (double)nmax;
    } else {
      const double tiny = 1e-15, small = 1e-9;
      const double ratio = ((double)m + tiny) / ((double)Rb + small);
      const float wgt = (float)(1.0 / (double)nmax);
      double bl = 1.0;
      float acc = 0.0f;
      for (int k = 0; k < nmax; ++k) {
        const int guess = m - k > 0 ? m - k : 0;
        bl *= ((double)s_cor[m][k] + tiny) / ((double)guess + small);
        double bk = pow(bl, 1.0 / (double)(k + 1));
        if (ratio < 1.0) bk *= exp(1.0 - 1.0 / ratio);
        const float term = (float)bk * wgt;
        acc = k == 0 ? term : acc + term;
      }
      sc = (double)acc;
    }
    s_score[m] = sc;
  }
  __syncthreads();

  // the row over token positions: CIDEr pads behind the end token with the last scored prefix; an end token at position 0
  // gives the reference's float32 -0.1 everywhere
  const double eos0 = (double)-0.1f;
  for (int t = tid; t < L; t += kThreads) {
    double cur, prev = 0.0;
    if (E == 0) {
      cur = prev = eos0;
    } else {
      cur = s_score[s_mc[t < E ? t : E - 1]];
      if (t > 0) prev = s_score[s_mc[t - 1 < E ? t - 1 : E - 1]];
    }
    scores[(size_t)b * lds + t] = cur;
    float d;
    if (t == 0) d = (float)cur;
    else if (cider) d = (float)(cur - prev);
    else d = (float)cur - (float)prev;     // BLEU rows are float32: the difference is taken in float32
    delta[(size_t)b * ldd + t] = d;
  }
}

}  // namespace

extern "C" int bmhrl_rewards(const int64_t* hyp, int64_t ldh, const int32_t* vmap, int32_t V, int64_t eos,
                             const int32_t* ref, int64_t ldr, const int32_t* ref_len, const int32_t* df_keys,
                             const double* df_logs, int32_t df_cap, int32_t metric, int32_t n, double sigma, int32_t B,
                             int32_t L, int32_t R, double* scores, int64_t lds, float* delta, int64_t ldd,
                             bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(hyp && vmap && ref && ref_len && scores && delta);
  BMHRL_CHECK_ARG(metric == BMHRL_REWARD_CIDER || metric == BMHRL_REWARD_BLEU);
  BMHRL_CHECK_ARG(B > 0 && L >= 1 && L <= kMaxL && R >= 1 && R <= kMaxR && V >= 1 && n >= 1 && n <= kMaxN);
  BMHRL_CHECK_ARG(ldh >= L && ldr >= R && lds >= L && ldd >= L);
  if (metric == BMHRL_REWARD_CIDER) {
    BMHRL_CHECK_ARG(df_keys && df_logs && df_cap >= 2 && (df_cap & (df_cap - 1)) == 0);
    BMHRL_CHECK_ARG(sigma > 0.0);
  }
  hipLaunchKernelGGL(rewards_kernel, dim3(B), dim3(kThreads), 0, S_(stream), hyp, (long)ldh, vmap, V, (long)eos, ref,
                     (long)ldr, ref_len, df_keys, df_logs, df_cap, metric, n, sigma, L, R, scores, (long)lds, delta,
                     (long)ldd);
  return hip_status(hipGetLastError());
}
