// Consensus (minimum-Bayes-risk) choice among a clip's hypotheses (bmhrl_amd/decode.py, the consensus section, rules R1-R6):
// the mean 1..N-gram agreement of every hypothesis with the other hypotheses of its clip, read from the decoder's token
// history after the token loop.  `steps` is a host integer, so the launch sits behind the captured token step, not in it.
//
// One 256-thread workgroup per (clip, hypothesis i).  The clip's K word rows (int64 ids: a token compares by its id whatever
// its value), their token weights and their lengths go to LDS.  Then, for g = 1 .. N:
//   (a) one work item per (row k, position p): is p the first occurrence of its g-gram in k, and how often does the gram
//       occur in k (cnt[k][p]; 0 where p is no first occurrence, so the distinct grams of a row are the non-zero entries in
//       the order of their first occurrence); for row i also the gram's weight wi[p];
//   (b) lane k: the gram mass W_k^g, one product and one add per distinct gram of k in that order;
//   (c) one work item per (row j != i, position p of i): min(c_i, c_j) of i's gram at p, written over cnt[j][p] (row j's own
//       counts are not needed after (b));
//   (d) lane j: M_g(i, j) over i's positions in ascending order, t_g = M_g / max(W_i^g, W_j^g), added to the lane's u.
// A last lane adds u(i, j) for ascending j.  No atomics, and every floating-point sum has one owner that adds in the
// prescribed order, so the result does not depend on the launch geometry.  Work: (a) and (c) each compare K * l^2 grams per
// g (l: words per row) -- a few thousand at the 30-token captions this is for, 10^6 per workgroup at the 256-token limit.
//
// Contraction to FMA is off in this file: one product, then one add, as the rules prescribe.
#include "common.h"
#include "../../include/bmhrl_hip.h"

#pragma clang fp contract(off)

#define S_(x) ((hipStream_t)(x))

namespace {

constexpr int kThreads = 256;
constexpr int kMaxK = BMHRL_CONSENSUS_MAX_K;
constexpr int kMaxS = BMHRL_CONSENSUS_MAX_STEPS;
constexpr int kMaxN = BMHRL_CONSENSUS_MAX_N;
constexpr int kCntLd = kMaxS + 2;       // 129 dwords per row: lanes j = 0 .. K-1 reading cnt[j][p] hit K different banks

// words a[0, G) == b[0, G); both runs lie inside their rows.  G is a template argument so that the compares unroll and the
// scans below keep several LDS reads in flight (with a run-time g every compare waited for its own read)
template <int G>
__device__ __forceinline__ bool gram_eq(const int64_t (&a)[G], const int64_t* b) {
  bool eq = true;
#pragma unroll
  for (int q = 0; q < G; ++q) eq &= a[q] == b[q];
  return eq;
}

// R2: the fp32 weights of the gram's tokens widened, added in token order, divided by G last
template <int G>
__device__ __forceinline__ double gram_weight(const float* w) {
  double s = (double)w[0];
#pragma unroll
  for (int q = 1; q < G; ++q) s = s + (double)w[q];
  return s / (double)G;
}

// phases (a) - (d) of the file header for one gram length; u: lane j's sum of t_g(i, j)
template <int G>
__device__ __forceinline__ void gram_pass(const int64_t* tok, const float* tokw, unsigned short* cnt, double* wi, double* mass,
                                          const int* len, int K, int S, int i, bool weighted, double& u) {
  const int tid = threadIdx.x;
  const int items = K * S;
  const int ni = len[i] - G + 1;                  // grams of i (<= 0: none)
  for (int idx = tid; idx < items; idx += kThreads) {                                // (a)
    const int k = idx / S, p = idx % S;
    const int nk = len[k] - G + 1;
    const int64_t* row = tok + k * S;
    int c = 0;
    bool first = true;
    if (p < nk) {
      int64_t a[G];
#pragma unroll
      for (int q = 0; q < G; ++q) a[q] = row[p + q];
#pragma unroll 4
      for (int q = 0; q < nk; ++q) {
        const bool eq = gram_eq<G>(a, row + q);
        c += eq;
        first &= !(eq && q < p);
      }
      if (k == i) wi[p] = weighted ? gram_weight<G>(tokw + k * S + p) : 1.0;
    }
    cnt[k * kCntLd + p] = (unsigned short)((p < nk && first) ? c : 0);
  }
  __syncthreads();
  if (tid < K) {                                                                     // (b) R3
    const int nk = len[tid] - G + 1;
    double W = 0.0;
#pragma unroll 4
    for (int p = 0; p < nk; ++p) {                // no branch on cnt: a position that is no first occurrence adds w * 0 = +0,
      const double w = weighted ? gram_weight<G>(tokw + tid * S + p) : 1.0;          // which changes no bit of W >= 0, and
      W = W + w * (double)cnt[tid * kCntLd + p];  // the reads of the next positions need not wait for this one's
    }
    mass[tid] = W;
  }
  __syncthreads();
  for (int idx = tid; idx < items; idx += kThreads) {                                // (c)
    const int j = idx / S, p = idx % S;
    if (j == i) continue;
    const int ci = cnt[i * kCntLd + p];
    int c = 0;
    if (ci) {
      const int nj = len[j] - G + 1;
      const int64_t* row = tok + j * S;
      int64_t a[G];
#pragma unroll
      for (int q = 0; q < G; ++q) a[q] = tok[i * S + p + q];
#pragma unroll 4
      for (int q = 0; q < nj; ++q) c += gram_eq<G>(a, row + q);
    }
    cnt[j * kCntLd + p] = (unsigned short)min(ci, c);
  }
  __syncthreads();
  if (tid < K && tid != i) {                                                         // (d) R4, R5
    double M = 0.0;
#pragma unroll 4
    for (int p = 0; p < ni; ++p) M = M + wi[p] * (double)cnt[tid * kCntLd + p];      // (cnt[j][p] = 0 where cnt[i][p] is)
    const double mx = fmax(mass[i], mass[tid]);
    u = u + (mx > 0.0 ? M / mx : 0.0);
  }
  __syncthreads();                                // the next pass writes cnt and wi again
}

__global__ __launch_bounds__(kThreads) void consensus_kernel(const int64_t* __restrict__ hist, long ld, int K, int S,
                                                             int64_t end_idx, int N, const float* __restrict__ tw, int V,
                                                             double* __restrict__ util, double* __restrict__ pair) {
  __shared__ int64_t tok[kMaxK * kMaxS];          // row k: tok[k * S .. k * S + S)
  __shared__ float tokw[kMaxK * kMaxS];           // the tokens' weights (read only when tw is given)
  __shared__ unsigned short cnt[kMaxK * kCntLd];
  __shared__ double wi[kMaxS];
  __shared__ double mass[kMaxK];
  __shared__ double ud[kMaxK];
  __shared__ int len[kMaxK];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / K, i = blockIdx.x % K;
  const int items = K * S;
  const bool weighted = tw != nullptr;

  for (int idx = tid; idx < items; idx += kThreads) {
    const int k = idx / S, p = idx % S;
    const int64_t v = hist[((long)b * K + k) * ld + 1 + p];       // column 0 is the start token; columns > S are not read
    tok[idx] = v;
    if (weighted) tokw[idx] = (v >= 0 && v < V) ? tw[v] : 0.f;
  }
  __syncthreads();
  // R1: l_k = the position of the first end token, S without one (wave w: rows w, w + 4, ...)
  for (int k = tid >> 6; k < K; k += kThreads / WAVE) {
    int m = S;
    for (int p = tid & 63; p < S; p += WAVE)
      if (tok[k * S + p] == end_idx) m = min(m, p);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o, 64));
    if ((tid & 63) == 0) len[k] = m;
  }
  __syncthreads();

  double u = 0.0;                                 // lane j < K: the sum of t_g(i, j) so far, g ascending
  gram_pass<1>(tok, tokw, cnt, wi, mass, len, K, S, i, weighted, u);
  if (N >= 2) gram_pass<2>(tok, tokw, cnt, wi, mass, len, K, S, i, weighted, u);
  if (N >= 3) gram_pass<3>(tok, tokw, cnt, wi, mass, len, K, S, i, weighted, u);
  if (N >= 4) gram_pass<4>(tok, tokw, cnt, wi, mass, len, K, S, i, weighted, u);
  if (tid < K) {
    const double uij = tid == i ? 0.0 : u / (double)N;
    ud[tid] = uij;
    if (pair) pair[((long)b * K + i) * K + tid] = uij;
  }
  __syncthreads();
  if (tid == 0) {                                                                    // R6
    double s = 0.0;
    for (int j = 0; j < K; ++j)
      if (j != i) s = s + ud[j];
    util[(long)b * K + i] = K > 1 ? s / (double)(K - 1) : 0.0;
  }
}

}  // namespace

extern "C" int bmhrl_consensus(const int64_t* hist, int64_t ld, int32_t B, int32_t K, int32_t steps, int64_t end_idx,
                               int32_t N, const float* token_weight, int32_t V, double* util, double* pair,
                               bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(hist && util);
  BMHRL_CHECK_ARG(B >= 1 && K >= 1 && steps >= 0);
  BMHRL_CHECK_ARG(K <= kMaxK && steps <= kMaxS && N >= 1 && N <= kMaxN);
  BMHRL_CHECK_ARG(B <= INT32_MAX / kMaxK);
  BMHRL_CHECK_ARG(V >= 0 && !(token_weight && V == 0));
  BMHRL_CHECK_ARG(ld >= (int64_t)steps + 1);
  hipLaunchKernelGGL(consensus_kernel, dim3((unsigned)(B * K)), dim3(kThreads), 0, S_(stream), hist, (long)ld, K, steps, end_idx,
                     N, token_weight, V, util, pair);
  return hip_status(hipGetLastError());
}
