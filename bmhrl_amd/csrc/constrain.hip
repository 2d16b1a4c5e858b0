// Constrained caption decoding (bmhrl_amd/decode.py, the constraints section): repetition penalty, no-repeat n-gram ban and
// minimum length applied in place to the step's fp32 log-probs, between the model's head and the token choice.  The step
// position t is a device word, so the launch sits inside the captured token step.
//
// One wave per row.  The row's t + 1 history tokens go to LDS; position j of the history (lane j, j + 64, ...) decides its
// own penalty -- applied only where j is the first occurrence of its token, so an id is multiplied once -- and its own ban
// (the n - 1 tokens from j equal the last n - 1: the token after them is banned).  At most t + 2 entries of the row are
// written, with plain stores and no atomics: every penalty address has one owner, and the bans and the end token all store
// the same -inf.  The three rules run in order behind barriers, so a banned token stays -inf whatever its penalty was.
#include "common.h"
#include "../../include/bmhrl_hip.h"

#define S_(x) ((hipStream_t)(x))

namespace {

constexpr int kThreads = WAVE;
constexpr int kMaxHist = BMHRL_LOGIT_RULES_MAX_HIST;

__global__ __launch_bounds__(kThreads) void logit_rules_kernel(float* __restrict__ logp, long ld, int V,
                                                               const int64_t* __restrict__ hist, long ld_hist,
                                                               const int64_t* __restrict__ tdev, int ngram, int min_len,
                                                               float penalty, int end_idx, int pad_idx) {
  __shared__ int64_t s[kMaxHist];
  const int row = blockIdx.x, tid = threadIdx.x;
  const long t = tdev[0];
  if (t < 0 || t + 1 > ld_hist || t + 1 > kMaxHist) return;       // (uniform) a position the history does not hold
  const int len = (int)t + 1;
  float* lp = logp + (long)row * ld;
  for (int j = tid; j < len; j += kThreads) s[j] = hist[(long)row * ld_hist + j];
  __syncthreads();
  if (penalty != 1.f) {
    for (int j = tid; j < len; j += kThreads) {
      const int64_t v = s[j];
      bool first = v >= 0 && v < V && v != pad_idx;
      for (int i = 0; first && i < j; ++i) first = s[i] != v;
      if (first) lp[v] = lp[v] * penalty;
    }
  }
  __syncthreads();
  if (ngram >= 1 && len >= ngram) {
    const int tail = len - ngram + 1;                             // the last n - 1 tokens: s[tail .. t]
    for (int j = tid; j <= len - ngram; j += kThreads) {
      bool match = true;
      for (int i = 0; match && i < ngram - 1; ++i) match = s[j + i] == s[tail + i];
      const int64_t v = s[j + ngram - 1];
      if (match && v >= 0 && v < V) lp[v] = -INFINITY;
    }
  }
  __syncthreads();
  if (tid == 0 && t < min_len) lp[end_idx] = -INFINITY;
}

}  // namespace

extern "C" int bmhrl_logit_rules(float* logp, int64_t ld, int32_t rows, int32_t V, const int64_t* hist, int64_t ld_hist,
                                 const int64_t* t, int32_t ngram, int32_t min_len, float penalty, int32_t end_idx,
                                 int32_t pad_idx, bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(logp && hist && t);
  BMHRL_CHECK_ARG(rows >= 1 && V >= 1 && ld >= V);
  BMHRL_CHECK_ARG(ld_hist >= 1 && ld_hist <= BMHRL_LOGIT_RULES_MAX_HIST);
  BMHRL_CHECK_ARG(ngram >= 0 && min_len >= 0 && penalty > 0.f && penalty < INFINITY);
  BMHRL_CHECK_ARG(end_idx >= 0 && end_idx < V && pad_idx >= 0 && pad_idx < V);
  hipLaunchKernelGGL(logit_rules_kernel, dim3((unsigned)rows), dim3(kThreads), 0, S_(stream), logp, (long)ld, V, hist,
                     (long)ld_hist, t, ngram, min_len, penalty, end_idx, pad_idx);
  return hip_status(hipGetLastError());
}
