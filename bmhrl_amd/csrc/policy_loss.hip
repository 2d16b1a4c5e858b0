// Self-critical policy gradient on sampled rollouts (bmhrl_amd/scst.py): the per-token weights of a
// rollout batch from the reward launch's per-prefix table (rules R1-R7 in include/bmhrl_hip.h), and the REINFORCE / clipped-
// ratio loss with an optional entropy bonus on the log-probs of the training forward, forward row sums and the dense gradient.
//
// The advantage launch is ONE 256-thread block (a few hundred rows): every floating-point sum has one owner that adds in the
// order the rules fix, so the host restatement performs the same IEEE operations and results compare for equality (the
// convention of consensus.hip).  The loss kernels are HBM-bound row kernels in the style of loss.hip: one 256-thread block per
// (rollout, step) row of V log-probs, 16-byte loads and stores where the dispatcher's conditions hold, no atomics.
//
// Contraction to FMA is off in this file: one product, then one add, as the rules prescribe.
#include "common.h"
#include "../../include/bmhrl_hip.h"

#pragma clang fp contract(off)

#define S_(x) ((hipStream_t)(x))

namespace {

constexpr int kThreads = 256;

// `len`, `reward` and `adv` are written and read back across the barriers below (no __restrict__ on them)
__global__ __launch_bounds__(kThreads) void rollout_advantage_kernel(const int64_t* __restrict__ toks, long ldt, int B, int n, int m,
                                                                     int64_t end_idx, const double* __restrict__ scores, long lds,
                                                                     int mode, const double* __restrict__ base, int* len,
                                                                     double* reward, double* adv, float* __restrict__ weight,
                                                                     long ldw, double* __restrict__ stats) {
  __shared__ long long s_len[kThreads];
  __shared__ double s_sum[2];
  __shared__ long long s_N;
  const int tid = threadIdx.x;
  const long rows = (long)B * n;
  long long nl = 0;
  for (long i = tid; i < rows; i += kThreads) {                                       // R1, R2
    const int64_t* row = toks + i * ldt + 1;       // column 0 is the start token
    int l = m;
    for (int t = m - 1; t >= 0; --t)               // (from the back and without a break: the loads do not wait for one another)
      if (row[t] == end_idx) l = t + 1;
    len[i] = l;
    reward[i] = scores[i * lds + (l - 1)];
    nl += l;
  }
  s_len[tid] = nl;
  __syncthreads();
  for (long i = tid; i < rows; i += kThreads) {                                       // R3: b_i, parked in adv[i]
    const long clip = i / n;
    double b = 0.0;
    if (mode == 1) {
      double s = 0.0;
      for (int j = 0; j < n; ++j)
        if (clip * n + j != i) s = s + reward[clip * n + j];
      b = s / (double)(n - 1);
    } else if (mode == 2) {
      b = base[clip];
    }
    adv[i] = b;
  }
  __syncthreads();
  if (tid == 0) {                                                                     // R5, R7: sums in row order, one owner each
    long long N = 0;
    for (int k = 0; k < kThreads; ++k) N += s_len[k];
    s_N = N;
    double s = 0.0;
    for (long i = 0; i < rows; ++i) s = s + reward[i];
    s_sum[0] = s;
  }
  if (tid == WAVE) {                               // (another wave: the two serial sums run side by side)
    double s = 0.0;
    for (long i = 0; i < rows; ++i) s = s + adv[i];
    s_sum[1] = s;
  }
  __syncthreads();
  const long long N = s_N;
  if (tid == 0) {
    stats[0] = s_sum[0] / (double)rows;
    stats[1] = s_sum[1] / (double)rows;
    stats[2] = (double)N / (double)rows;
    stats[3] = (double)N;
  }
  // R4, R6: wave w takes the rows w, w + 4, ...: one division per row, the row's m weights written side by side
  for (long i = tid >> 6; i < rows; i += kThreads / WAVE) {
    const double a = reward[i] - adv[i];           // (every lane of the wave reads b_i before lane 0 replaces it: one instruction stream)
    const float w = (float)(a / (double)N);
    const int l = len[i];
    for (int t = tid & 63; t < m; t += WAVE) weight[i * ldw + t] = t < l ? w : 0.f;
    __builtin_amdgcn_wave_barrier();
    if ((tid & 63) == 0) adv[i] = a;
  }
}

// the policy term of one row and its derivative w.r.t. logp[a] (header: "policy term")
__device__ __forceinline__ void policy_term(float lpa, float w, const float* logq, long row, float clip, float& loss, float& grad) {
  if (!logq) {
    loss = -w * lpa;
    grad = -w;
    return;
  }
  const float rho = expf(lpa - logq[row]);
  const float un = rho * w;
  const float cl = fminf(fmaxf(rho, 1.f - clip), 1.f + clip) * w;
  const bool unclipped = un <= cl;                 // the minimum is the unclipped branch, ties included
  loss = -(unclipped ? un : cl);
  grad = unclipped ? -un : 0.f;
}

// p log p of one column; a column at -inf contributes 0 (expf(-inf) * -inf would be NaN)
__device__ __forceinline__ float plogp(float lp) { return lp == -INFINITY ? 0.f : expf(lp) * lp; }
// d(-H)/d logp_v = p_v (1 + logp_v)
__device__ __forceinline__ float dneg_entropy(float lp) { return lp == -INFINITY ? 0.f : expf(lp) * (1.f + lp); }

// entropy-less forward: a gather, one thread per row
__global__ void policy_gather_fwd_kernel(const float* __restrict__ logp, long ld, const int64_t* __restrict__ action,
                                         const float* __restrict__ weight, const float* __restrict__ logq, float clip,
                                         float* __restrict__ row_loss, float* __restrict__ row_entropy, long rows, int V) {
  const long row = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= rows) return;
  const int64_t a = action[row];
  float loss = 0.f, grad;
  if (a >= 0 && a < V) policy_term(logp[row * ld + a], weight[row], logq, row, clip, loss, grad);
  row_loss[row] = loss;
  row_entropy[row] = 0.f;
}

// forward with the entropy term: H_i = -sum_v p_v logp_v, every thread's partial sum and the exchange in fp64 (the terms are
// fp32 products; 10^4 of them added in fp32 would leave more than the 2^-22 the tests allow)
template <bool VEC>
__global__ __launch_bounds__(kThreads) void policy_entropy_fwd_kernel(const float* __restrict__ logp, long ld,
                                                                     const int64_t* __restrict__ action,
                                                                     const float* __restrict__ weight, const float* __restrict__ logq,
                                                                     float clip, const float* __restrict__ ent_weight,
                                                                     float* __restrict__ row_loss, float* __restrict__ row_entropy,
                                                                     int V) {
  __shared__ double red[kThreads / WAVE];
  const long row = blockIdx.x;
  const float* lp = logp + row * ld;
  double s = 0.0;
  if (VEC) {
    for (int c = 4 * threadIdx.x; c < V; c += 4 * kThreads) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(lp + c);
      s += (double)((plogp(v[0]) + plogp(v[1])) + (plogp(v[2]) + plogp(v[3])));
    }
  } else {
    for (int c = threadIdx.x; c < V; c += kThreads) s += (double)plogp(lp[c]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x != 0) return;
  const float H = -(float)((red[0] + red[1]) + (red[2] + red[3]));
  const int64_t a = action[row];
  float loss = 0.f, grad;
  if (a >= 0 && a < V) {
    policy_term(lp[a], weight[row], logq, row, clip, loss, grad);
    loss = loss - ent_weight[row] * H;
  }
  row_loss[row] = loss;
  row_entropy[row] = H;
}

// the dense gradient in one pass: every column of the row is written once -- zeros (or the entropy term) and the policy
// term at the action's column -- times gscale[0] * drow[row].  A row whose action is out of range is all zeros.
template <bool VEC, bool ENT>
__global__ __launch_bounds__(kThreads) void policy_loss_bwd_kernel(const float* __restrict__ logp, long ld,
                                                                  const int64_t* __restrict__ action, const float* __restrict__ weight,
                                                                  const float* __restrict__ logq, float clip,
                                                                  const float* __restrict__ ent_weight, const float* __restrict__ gscale,
                                                                  const float* __restrict__ drow, float* __restrict__ dlogp, long ldg,
                                                                  int V) {
  const long row = blockIdx.x;
  const float* lp = logp + row * ld;
  float* g = dlogp + row * ldg;
  const int64_t a64 = action[row];
  const bool live = a64 >= 0 && a64 < V;
  const int a = live ? (int)a64 : -1;
  const float scale = gscale[0] * drow[row];
  float loss, ga = 0.f;
  if (live) policy_term(logq ? lp[a] : 0.f, weight[row], logq, row, clip, loss, ga);
  const float beta = (ENT && live) ? ent_weight[row] : 0.f;
  if (VEC) {
    for (int c = 4 * threadIdx.x; c < V; c += 4 * kThreads) {
      f32x4 o = {0.f, 0.f, 0.f, 0.f};
      if (ENT && live) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(lp + c);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = beta * dneg_entropy(v[j]);
      }
      if (a >= c && a < c + 4) o[a - c] += ga;
      if (live) {
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (ENT || c + j == a) ? o[j] * scale : 0.f;
      }
      *reinterpret_cast<f32x4*>(g + c) = o;
    }
  } else {
    for (int c = threadIdx.x; c < V; c += kThreads) {
      float o = (ENT && live) ? beta * dneg_entropy(lp[c]) : 0.f;
      if (c == a) o += ga;
      g[c] = (live && (ENT || c == a)) ? o * scale : 0.f;
    }
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int bmhrl_rollout_advantage(const int64_t* toks, int64_t ldt, int32_t B, int32_t n, int32_t m, int64_t end_idx,
                                       const double* scores, int64_t lds, int32_t baseline, const double* base, int32_t* len,
                                       double* reward, double* adv, float* weight, int64_t ldw, double* stats,
                                       bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(toks && scores && len && reward && adv && weight && stats);
  BMHRL_CHECK_ARG(B >= 1 && n >= 1 && n <= BMHRL_ROLLOUT_MAX_N && m >= 1 && m <= BMHRL_REWARDS_MAX_L);
  BMHRL_CHECK_ARG(B <= INT32_MAX / BMHRL_ROLLOUT_MAX_N);
  BMHRL_CHECK_ARG(baseline == BMHRL_BASELINE_NONE || baseline == BMHRL_BASELINE_LEAVE_ONE_OUT || baseline == BMHRL_BASELINE_GIVEN);
  BMHRL_CHECK_ARG(!(baseline == BMHRL_BASELINE_LEAVE_ONE_OUT && n == 1));
  BMHRL_CHECK_ARG(!(baseline == BMHRL_BASELINE_GIVEN && !base));
  BMHRL_CHECK_ARG(ldt >= (int64_t)m + 1 && lds >= m && ldw >= m);
  hipLaunchKernelGGL(rollout_advantage_kernel, dim3(1), dim3(kThreads), 0, S_(stream), toks, (long)ldt, B, n, m, end_idx, scores,
                     (long)lds, baseline, base, len, reward, adv, weight, (long)ldw, stats);
  return hip_status(hipGetLastError());
}

extern "C" int bmhrl_policy_loss_fwd(const float* logp, int64_t ld, const int64_t* action, const float* weight, const float* logq,
                                     float clip, const float* ent_weight, float* row_loss, float* row_entropy, int64_t rows,
                                     int32_t V, bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(logp && action && weight && row_loss && row_entropy && rows > 0 && rows <= INT32_MAX && V > 0 && ld >= V);
  BMHRL_CHECK_ARG(clip >= 0.f && (clip > 0.f) == (logq != nullptr));
  if (!ent_weight) {
    hipLaunchKernelGGL(policy_gather_fwd_kernel, dim3((unsigned)((rows + kThreads - 1) / kThreads)), dim3(kThreads), 0, S_(stream),
                       logp, (long)ld, action, weight, logq, clip, row_loss, row_entropy, (long)rows, V);
    return hip_status(hipGetLastError());
  }
#define PLF(VEC_) hipLaunchKernelGGL(policy_entropy_fwd_kernel<VEC_>, dim3((unsigned)rows), dim3(kThreads), 0, S_(stream), logp,   \
                                     (long)ld, action, weight, logq, clip, ent_weight, row_loss, row_entropy, V)
  if (V % 4 == 0 && ld % 4 == 0 && aligned16(logp)) PLF(true); else PLF(false);
#undef PLF
  return hip_status(hipGetLastError());
}

extern "C" int bmhrl_policy_loss_bwd(const float* logp, int64_t ld, const int64_t* action, const float* weight, const float* logq,
                                     float clip, const float* ent_weight, const float* gscale, const float* drow, float* dlogp,
                                     int64_t ldg, int64_t rows, int32_t V, bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(logp && action && weight && gscale && drow && dlogp && rows > 0 && rows <= INT32_MAX && V > 0 && ld >= V &&
                  ldg >= V);
  BMHRL_CHECK_ARG(clip >= 0.f && (clip > 0.f) == (logq != nullptr));
  const bool vec = V % 4 == 0 && ld % 4 == 0 && ldg % 4 == 0 && aligned16(logp) && aligned16(dlogp);
#define PLB(VEC_, ENT_) hipLaunchKernelGGL((policy_loss_bwd_kernel<VEC_, ENT_>), dim3((unsigned)rows), dim3(kThreads), 0, S_(stream), \
                                           logp, (long)ld, action, weight, logq, clip, ent_weight, gscale, drow, dlogp, (long)ldg, V)
  if (vec) { if (ent_weight) PLB(true, true); else PLB(true, false); }
  else     { if (ent_weight) PLB(false, true); else PLB(false, false); }
#undef PLB
  return hip_status(hipGetLastError());
}
