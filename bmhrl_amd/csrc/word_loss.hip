// The DETR word loss for gfx950: Hungarian matching of a caption's words to the detector's queries and
// the weighted cross entropy over the (B, Q, C = V + 1) class logits, in four ordinary launches on the caller's stream:
//   1. word_cost      one 256-thread block per (b, q) row: log-sum-exp of the row in ONE pass (online maximum), the logits at the
//                     caption's words, the "no word" logit, and the matching cost -cost_scale * p(word)
//   2. lsa_match      one wavefront per sample: shortest augmenting paths (Jonker-Volgenant) over the cost block in LDS
//   3. word_loss      one block: class map, row weights and the weighted mean, summed in fp64 in a fixed order
//   4. word_loss_bwd  one block per row: d loss / d logits, a streaming pass with nothing summed across threads
// No launch synchronises across blocks, none uses atomics; equal inputs give equal bits.
//
// Reference: loss/hungarian_matcher.py:42-59 (softmax, cost, scipy's linear_sum_assignment per sample),
// epoch_loops/captioning_bmrl_loops.py:1114-1129 (F.cross_entropy with weight eos_coef on the last class).
#include <cfloat>
#include "common.h"
#include "../../include/bmhrl_hip.h"

namespace {

constexpr int kMaxQ = BMHRL_WORD_LOSS_MAX_Q;   // 128: two query columns per lane of the match kernel
constexpr int kMaxL = BMHRL_WORD_LOSS_MAX_L;   // 64: one target row per lane
constexpr int kThreads = 256;

// A row of C floats at r, 4-byte aligned only (an odd leading dimension moves every row's alignment): `head` scalar
// elements up to the first 16-byte boundary, `nvec` float4, then the scalar tail [head + 4 * nvec, C).
struct RowSplit {
  int head, nvec;
};
__device__ __forceinline__ RowSplit split_row(const float* r, int C) {
  RowSplit s;
  s.head = min(C, (int)((16u - (unsigned)((uintptr_t)r & 15u)) & 15u) >> 2);
  s.nvec = (C - s.head) >> 2;
  return s;
}

// running (maximum, sum of exp(x - maximum)) of a thread's share of the row.  The terms are fp32 exponentials; they are ADDED
// in fp64, so the sum carries the terms' own rounding (relative 2^-24 each, nothing for the maximum's exp(0) = 1) and no
// rounding of the ~C additions: where one probability dominates, p - 1 in the backward is a difference of nearly equal
// numbers and the error of the sum is what is left of it.
__device__ __forceinline__ void online_add(float& m, double& s, float x) {
  if (x > m) {
    s *= (double)expf(m - x);
    m = x;
  }
  s += (double)expf(x - m);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__global__ __launch_bounds__(kThreads) void word_cost_kernel(const float* __restrict__ x, long ld, const int64_t* __restrict__ cap,
                                                             long ldc, int64_t pad, float cost_scale, int Q, int L, int C,
                                                             int* __restrict__ words, int* __restrict__ n_words,
                                                             float* __restrict__ lse_out, float* __restrict__ lse_lo_out,
                                                             float* __restrict__ none_out, float* __restrict__ gathered,
                                                             float* __restrict__ cost) {
  __shared__ float red[16];
  __shared__ double red64[kThreads / WAVE];
  __shared__ float lse_sh[2];
  __shared__ int w[kMaxL];
  __shared__ int n_sh;
  const int tid = threadIdx.x;
  const long row = blockIdx.x;
  const int b = (int)(row / Q), q = (int)(row % Q);

  // compaction (wave 0; L <= 64): the caption's entries that are words, in order.  pad_idx and every id outside [0, C - 2]
  // are dropped, so w[] only ever holds columns of the row.
  if (tid < WAVE) {
    const int64_t v = tid < L ? cap[(long)b * ldc + tid] : pad;
    const bool keep = tid < L && v != pad && v >= 0 && v <= (int64_t)C - 2;
    const unsigned long long mask = __ballot(keep);
    const int pos = __popcll(mask & ((1ull << tid) - 1ull));
    if (keep) w[pos] = (int)v;
    if (tid == 0) n_sh = __popcll(mask);
  }

  const float* r = x + row * ld;
  const RowSplit sp = split_row(r, C);
  float m = -FLT_MAX;
  double s = 0.0;
  if (tid < sp.head) online_add(m, s, r[tid]);
  const f32x4* rv = reinterpret_cast<const f32x4*>(r + sp.head);
#pragma unroll 4
  for (int i = tid; i < sp.nvec; i += kThreads) {
    const f32x4 v = rv[i];
    const float mx = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
    if (mx > m) {
      s *= (double)expf(m - mx);
      m = mx;
    }
    s += ((double)expf(v[0] - m) + (double)expf(v[1] - m)) + ((double)expf(v[2] - m) + (double)expf(v[3] - m));
  }
  const int tail = sp.head + 4 * sp.nvec + tid;
  if (tail < C) online_add(m, s, r[tail]);

  const float mb = block_max(m, red);                 // (its barriers also publish w[] and n_sh)
  const double sw = wave_sum_f64(s * (double)expf(m - mb));
  if ((tid & 63) == 0) red64[tid >> 6] = sw;
  __syncthreads();
  // lse = maximum + log(sum), formed in fp64 by one thread and kept as an fp32 pair: lse is the nearest float and lse_lo
  // what it misses, so exp((x - lse) - lse_lo) in the other launches sees the sum's precision, not the rounding of lse
  // to a float of the logits' magnitude
  if (tid == 0) {
    const double l = (double)mb + log((red64[0] + red64[1]) + (red64[2] + red64[3]));
    const float hi = (float)l;
    lse_sh[0] = hi;
    lse_sh[1] = (float)(l - (double)hi);
  }
  __syncthreads();
  const float lse = lse_sh[0], lse_lo = lse_sh[1];
  const int n = n_sh;
  if (tid == 0) {
    lse_out[row] = lse;
    lse_lo_out[row] = lse_lo;
    none_out[row] = r[C - 1];
  }
  if (tid < L) {
    float g = 0.f, c = 0.f;
    if (tid < n) {
      g = r[w[tid]];
      c = cost_scale * -expf((g - lse) - lse_lo);
    }
    gathered[row * L + tid] = g;
    cost[row * L + tid] = c;
    if (q == 0) words[(long)b * L + tid] = tid < n ? w[tid] : -1;
  }
  if (q == 0 && tid == 0) n_words[b] = n;
}

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// Rectangular minimum-cost assignment, one wavefront per sample: the n targets are inserted one by one, each by a
// shortest augmenting path over the reduced costs (the algorithm of scipy's linear_sum_assignment).  Lane l owns query
// columns l and l + 64 (dual v, path length, predecessor, assigned target) and target row l (dual u, assigned query).
// Duals and path lengths are fp64: sums of a few hundred fp32 entries are then exact to ~1e-16 relative, so the result is
// an optimum of the fp32 matrix as given.  Every arg-min takes the lowest query index among equals.
__global__ __launch_bounds__(WAVE) void lsa_match_kernel(const float* __restrict__ cost, long sb, long sq, long sl,
                                                         const int* __restrict__ n_of, int Q, int L,
                                                         int* __restrict__ query_of_target) {
  extern __shared__ float cl[];                       // cl[j * Q + q]: target-major, so a row scan reads consecutive floats
  const int lane = threadIdx.x;
  const int b = blockIdx.x;
  const int n = min(max(n_of[b], 0), min(L, Q));
  const float* cb = cost + (long)b * sb;
  for (int idx = lane; idx < n * Q; idx += WAVE) {
    const int j = idx / Q, q = idx - j * Q;
    cl[idx] = cb[(long)q * sq + (long)j * sl];
  }
  __syncthreads();

  const double inf = INFINITY;
  double v0 = 0.0, v1 = 0.0, u = 0.0;
  int r4c0 = -1, r4c1 = -1, c4r = -1;
  const bool has0 = lane < Q, has1 = lane + WAVE < Q;

  for (int cur = 0; cur < n; ++cur) {
    double sp0 = inf, sp1 = inf, min_val = 0.0;
    int path0 = -1, path1 = -1;
    bool sc0 = false, sc1 = false, sr = false;
    int i = cur, sink = -1;
    for (int it = 0; it < Q && sink < 0; ++it) {
      if (lane == i) sr = true;
      const double ui = __shfl(u, i, WAVE);
      const float* ci = cl + i * Q;
      double cand0 = inf, cand1 = inf;
      if (has0 && !sc0) {
        const double red = min_val + (double)ci[lane] - ui - v0;
        if (red < sp0) {
          sp0 = red;
          path0 = i;
        }
        cand0 = sp0;
      }
      if (has1 && !sc1) {
        const double red = min_val + (double)ci[lane + WAVE] - ui - v1;
        if (red < sp1) {
          sp1 = red;
          path1 = i;
        }
        cand1 = sp1;
      }
      double best = cand0;
      int bj = lane;
      if (cand1 < cand0) {
        best = cand1;
        bj = lane + WAVE;
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double ob = __shfl_xor(best, o, WAVE);
        const int oj = __shfl_xor(bj, o, WAVE);
        if (ob < best || (ob == best && oj < bj)) {
          best = ob;
          bj = oj;
        }
      }
      if (!(best < inf)) break;                       // only a non-finite cost gets here: the target stays unmatched
      min_val = best;
      const int j = uniform(bj);
      const int owner = j & (WAVE - 1);
      const int r = uniform(__shfl(j < WAVE ? r4c0 : r4c1, owner, WAVE));
      if (lane == owner) {
        if (j < WAVE) sc0 = true; else sc1 = true;
      }
      if (r < 0) sink = j; else i = r;
    }
    if (sink < 0) continue;

    // duals: u of the scanned rows, v of the scanned columns (the sink's own path length equals min_val)
    {
      const int c = c4r < 0 ? 0 : c4r;
      const double a0 = __shfl(sp0, c & (WAVE - 1), WAVE), a1 = __shfl(sp1, c & (WAVE - 1), WAVE);
      if (sr) u += lane == cur ? min_val : min_val - (c < WAVE ? a0 : a1);
      if (sc0) v0 -= min_val - sp0;
      if (sc1) v1 -= min_val - sp1;
    }
    // augment along the predecessors, from the sink back to the inserted row
    int j = sink;
    for (int it = 0; it <= n; ++it) {
      const int owner = j & (WAVE - 1);
      const int i2 = uniform(__shfl(j < WAVE ? path0 : path1, owner, WAVE));
      if (lane == owner) {
        if (j < WAVE) r4c0 = i2; else r4c1 = i2;
      }
      const int old = uniform(__shfl(c4r, i2, WAVE));
      if (lane == i2) c4r = j;
      if (i2 == cur) break;
      j = old;
    }
  }
  if (lane < L) query_of_target[(long)b * L + lane] = lane < n ? c4r : -1;
}

// Class map, row weights and the weighted mean.  One block; thread t takes rows t, t + 256, ... and the partial sums are
// combined by a fixed tree in fp64, so the two outputs have the same bits in every run.  A query named by several
// targets takes the last of them (a matching never does that; a caller's own indices might).
__global__ __launch_bounds__(kThreads) void word_loss_kernel(const int* __restrict__ words, const int* __restrict__ n_words,
                                                             const int* __restrict__ qot, const float* __restrict__ lse,
                                                             const float* __restrict__ lse_lo, const float* __restrict__ x_none,
                                                             const float* __restrict__ gathered, float eos_coef, int B, int Q,
                                                             int L, int C, int* __restrict__ tgt_class,
                                                             float* __restrict__ row_w, float* __restrict__ loss_scale) {
  __shared__ double num[kThreads], den[kThreads];
  const int tid = threadIdx.x;
  const long rows = (long)B * Q;
  double a = 0.0, d = 0.0;
  for (long row = tid; row < rows; row += kThreads) {
    const int b = (int)(row / Q), q = (int)(row % Q);
    const int n = min(max(n_words[b], 0), L);
    int hit = -1;
    for (int j = 0; j < n; ++j)
      if (qot[(long)b * L + j] == q) hit = j;
    int cls = C - 1;
    float wt = eos_coef, xt = x_none[row];
    if (hit >= 0) {
      const int word = words[(long)b * L + hit];
      if (word >= 0 && word <= C - 2) {               // (word_cost never writes another; a caller's own buffer might hold one)
        cls = word;
        wt = 1.f;
        xt = gathered[row * L + hit];
      }
    }
    tgt_class[row] = cls;
    row_w[row] = wt;
    a += (double)wt * (((double)lse[row] + (double)lse_lo[row]) - (double)xt);
    d += (double)wt;
  }
  num[tid] = a;
  den[tid] = d;
  __syncthreads();
  for (int o = kThreads / 2; o > 0; o >>= 1) {
    if (tid < o) {
      num[tid] += num[tid + o];
      den[tid] += den[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    loss_scale[0] = (float)(num[0] / den[0]);
    loss_scale[1] = (float)(1.0 / den[0]);
  }
}

// p - [target]: at the target's column p - 1 is formed as expm1, not as a rounded p minus 1 -- with a dominant p that
// difference would keep p's rounding (2^-25) against a result many times smaller
__device__ __forceinline__ float grad_term(float v, float l, float l2, bool target) {
  const float d = (v - l) - l2;
  return target ? expm1f(d) : expf(d);
}

__global__ __launch_bounds__(kThreads) void word_loss_bwd_kernel(const float* __restrict__ x, long ld, const float* __restrict__ lse,
                                                                 const float* __restrict__ lse_lo,
                                                                 const int* __restrict__ tgt_class,
                                                                 const float* __restrict__ row_w,
                                                                 const float* __restrict__ loss_scale,
                                                                 const float* __restrict__ g, float* __restrict__ dx, long ldd,
                                                                 int C) {
  const int tid = threadIdx.x;
  const long row = blockIdx.x;
  const float* r = x + row * ld;
  float* o = dx + row * ldd;
  const float l = lse[row], l2 = lse_lo[row];
  const int t = tgt_class[row];
  const float k = (float)((double)(g ? g[0] : 1.f) * (double)row_w[row] * (double)loss_scale[1]);      // one rounding
  const RowSplit sp = split_row(r, C);
  if (tid < sp.head) o[tid] = k * grad_term(r[tid], l, l2, tid == t);
  const f32x4* rv = reinterpret_cast<const f32x4*>(r + sp.head);
  const bool vec_out = (((uintptr_t)(o + sp.head)) & 15u) == 0;      // the output row may be aligned differently
#pragma unroll 4
  for (int i = tid; i < sp.nvec; i += kThreads) {
    const f32x4 v = rv[i];
    const int c = sp.head + 4 * i;
    f32x4 d;
#pragma unroll
    for (int e = 0; e < 4; ++e) d[e] = k * expf((v[e] - l) - l2);
    if ((unsigned)(t - c) < 4u) {                     // the one float4 of the row that holds the target's column
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c + e == t) d[e] = k * grad_term(v[e], l, l2, true);
    }
    if (vec_out) {
      *reinterpret_cast<f32x4*>(o + c) = d;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) o[c + e] = d[e];
    }
  }
  const int tail = sp.head + 4 * sp.nvec + tid;
  if (tail < C) o[tail] = k * grad_term(r[tail], l, l2, tail == t);
}

#define S_(x) ((hipStream_t)(x))

}  // namespace

#define WORD_LOSS_CHECK_SHAPE(B, Q, L, C)                                   \
  BMHRL_CHECK_ARG((B) > 0 && (Q) > 0 && (L) > 0 && (C) >= 2);               \
  BMHRL_CHECK_ARG((Q) <= kMaxQ && (L) <= kMaxL && (L) <= (Q));              \
  BMHRL_CHECK_ARG((int64_t)(B) * (Q) <= INT32_MAX)

extern "C" int bmhrl_word_cost(const float* logits, int64_t ld, const int64_t* captions, int64_t ldc, int64_t pad_idx,
                               float cost_scale, int32_t B, int32_t Q, int32_t L, int32_t C, int32_t* words, int32_t* n_words,
                               float* lse, float* lse_lo, float* x_none, float* gathered, float* cost, bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(logits && captions && words && n_words && lse && lse_lo && x_none && gathered && cost);
  WORD_LOSS_CHECK_SHAPE(B, Q, L, C);
  BMHRL_CHECK_ARG(ld >= C && ldc >= L);
  hipLaunchKernelGGL(word_cost_kernel, dim3((unsigned)(B * Q)), dim3(kThreads), 0, S_(stream), logits, (long)ld, captions,
                     (long)ldc, pad_idx, cost_scale, Q, L, C, words, n_words, lse, lse_lo, x_none,
                     gathered, cost);
  return hip_status(hipGetLastError());
}

extern "C" int bmhrl_lsa_match(const float* cost, int64_t sb, int64_t sq, int64_t sl, const int32_t* n, int32_t B, int32_t Q,
                               int32_t L, int32_t* query_of_target, bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(cost && n && query_of_target);
  BMHRL_CHECK_ARG(B > 0 && Q > 0 && L > 0);
  BMHRL_CHECK_ARG(Q <= kMaxQ && L <= kMaxL && L <= Q);
  BMHRL_CHECK_ARG(sb >= 0 && sq >= 1 && sl >= 1);
  hipLaunchKernelGGL(lsa_match_kernel, dim3((unsigned)B), dim3(WAVE), (size_t)L * Q * sizeof(float), S_(stream), cost, (long)sb,
                     (long)sq, (long)sl, n, Q, L, query_of_target);
  return hip_status(hipGetLastError());
}

extern "C" int bmhrl_word_loss(const int32_t* words, const int32_t* n_words, const int32_t* query_of_target, const float* lse,
                               const float* lse_lo, const float* x_none, const float* gathered, float eos_coef, int32_t B, int32_t Q, int32_t L,
                               int32_t C, int32_t* tgt_class, float* row_w, float* loss_scale, bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(words && n_words && query_of_target && lse && lse_lo && x_none && gathered && tgt_class && row_w && loss_scale);
  WORD_LOSS_CHECK_SHAPE(B, Q, L, C);
  hipLaunchKernelGGL(word_loss_kernel, dim3(1), dim3(kThreads), 0, S_(stream), words, n_words, query_of_target, lse, lse_lo,
                     x_none, gathered, eos_coef, B, Q, L, C, tgt_class, row_w, loss_scale);
  return hip_status(hipGetLastError());
}

extern "C" int bmhrl_word_loss_bwd(const float* logits, int64_t ld, const float* lse, const float* lse_lo,
                                   const int32_t* tgt_class, const float* row_w, const float* loss_scale, const float* g, float* dlogits, int64_t ldd,
                                   int32_t B, int32_t Q, int32_t C, bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(logits && lse && lse_lo && tgt_class && row_w && loss_scale && dlogits);
  BMHRL_CHECK_ARG(B > 0 && Q > 0 && C >= 2 && Q <= kMaxQ);
  BMHRL_CHECK_ARG((int64_t)B * Q <= INT32_MAX);
  BMHRL_CHECK_ARG(ld >= C && ldd >= C);
  hipLaunchKernelGGL(word_loss_bwd_kernel, dim3((unsigned)(B * Q)), dim3(kThreads), 0, S_(stream), logits, (long)ld, lse,
                     lse_lo, tgt_class, row_w, loss_scale, g, dlogits, (long)ldd, C);
  return hip_status(hipGetLastError());
}
