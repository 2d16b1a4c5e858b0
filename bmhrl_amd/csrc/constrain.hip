// Constrained caption decoding (bmhrl_amd/decode.py, the constraints section): repetition penalty, no-repeat n-gram ban and
// minimum length applied in place to the step's fp32 log-probs, between the model's head and the token choice.  The step
// position t is a device word, so the launch sits inside the captured token step.
//
// One wave per row.  The row's t + 1 history tokens go to LDS; position j of the history (lane j, j + 64, ...) decides its
// own penalty -- applied only where j is the first occurrence of its token, so an id is multiplied once -- and its own ban
// (the n - 1 tokens from j equal the last n - 1: the token after them is banned).  At most t + 2 entries of the row are
// written, with plain stores and no atomics: every penalty address has one owner, and the bans and the end token all store
// the same -inf.  The three rules run in order behind barriers, so a banned token stays -inf whatever its penalty was.
//
// Paragraph-aware decoding (the context rules C1-C5 of the same section) is a second kernel, logit_rules_ctx_kernel: the
// plain one above it stays as it is.  Per clip a context of up to BMHRL_LOGIT_RULES_MAX_CTX int64 entries holds the tokens
// of the video's earlier captions; an entry is a word when 0 <= id < V and id != pad_idx, anything else is a gap (a
// sentence separator or filler).  All rows of a clip share its context: row r reads context row r / rows_per_ctx.
//  C1. ctx_penalty != 1: for every distinct word id v of the context, lp[v] = lp[v] * ctx_penalty -- one fp32 multiply, once
//      per id, after rule 1's multiply where an id is in both;
//  C2. ctx_ngram = n_c >= 1 and t >= n_c - 1: the tail is s[t-n_c+2 .. t], the last n_c - 1 generated tokens (never the start
//      token; empty for n_c = 1).  For every j in [0, C - n_c] whose window ctx[j .. j+n_c-1] is all words and whose first
//      n_c - 1 entries equal the tail, lp[ctx[j+n_c-1]] = -inf.  A window with a gap matches nothing, so no n-gram spans two
//      context sentences;
//  C3. the order is 1, C1, 2, C2, 3 in one launch, a barrier between the rules: a banned entry is -inf whatever was
//      multiplied into it;
//  C4 (off state) and C5 (refusals) are the decoders' business: they issue this launch only with context rules set and a
//      context present, in place of the plain launch, never next to it.
// Still one wave per row.  The context goes to LDS as int32 with gaps normalised to -1 (a word id is < V <= 65536).  C1 is
// exact and linear in C through a V-bit map in LDS that the wave clears first: every context position sets its id's bit
// with an LDS or-and-return, and the position that finds the bit clear owns the multiply.  Which position wins changes
// nothing: the id is multiplied exactly once by the same value, so two runs give equal bits.  C2's position p, the follower
// of the window that ends at it, compares the n_c - 1 entries before it with the tail from LDS.  Global memory sees plain
// stores only.  A lane keeps its 16 context positions in registers: the 16 loads are issued together (before t is known),
// and C1's multiplies are 16 independent loads, then 16 stores, not 16 round trips one after another -- the launch sits on
// the token step's critical path, where the wave's latency chain is what it costs.
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

constexpr int kMaxCtx = BMHRL_LOGIT_RULES_MAX_CTX;
constexpr int kCtxMaxV = BMHRL_LOGIT_RULES_CTX_MAX_V;
constexpr int kCtxPerLane = kMaxCtx / kThreads;                   // context positions per lane, kept in registers
static_assert(kCtxPerLane * kThreads == kMaxCtx && kCtxPerLane <= 32, "one bit per owned position in a 32-bit word");

__global__ __launch_bounds__(kThreads) void logit_rules_ctx_kernel(float* __restrict__ logp, long ld, int V,
                                                                   const int64_t* __restrict__ hist, long ld_hist,
                                                                   const int64_t* __restrict__ tdev, int ngram, int min_len,
                                                                   float penalty, int end_idx, int pad_idx,
                                                                   const int64_t* __restrict__ ctx, int C, int rows_per_ctx,
                                                                   int ctx_ngram, float ctx_penalty) {
  __shared__ int64_t s[kMaxHist];
  __shared__ int c[kMaxCtx];                                      // the context, gaps as -1
  __shared__ unsigned seen[kCtxMaxV / 32];                        // C1: one bit per token id
  const int row = blockIdx.x, tid = threadIdx.x;
  // the lane's context positions tid, tid + 64, ...: all loads in flight at once, and before t is known
  const int64_t* cx = ctx + (long)(row / rows_per_ctx) * C;
  int64_t raw[kCtxPerLane];
#pragma unroll
  for (int i = 0; i < kCtxPerLane; ++i) raw[i] = tid + i * kThreads < C ? cx[tid + i * kThreads] : -1;
  const long t = tdev[0];
  if (t < 0 || t + 1 > ld_hist || t + 1 > kMaxHist) return;       // (uniform) a position the history does not hold
  const int len = (int)t + 1;
  float* lp = logp + (long)row * ld;
  for (int j = tid; j < len; j += kThreads) s[j] = hist[(long)row * ld_hist + j];
  int w[kCtxPerLane];                                             // the lane's entries: a word id, -1 for a gap or past C
#pragma unroll
  for (int i = 0; i < kCtxPerLane; ++i) {
    w[i] = (raw[i] >= 0 && raw[i] < V && raw[i] != pad_idx) ? (int)raw[i] : -1;
    if (tid + i * kThreads < C) c[tid + i * kThreads] = w[i];
  }
  if (ctx_penalty != 1.f)
    for (int k = tid; k < (V + 31) / 32; k += kThreads) seen[k] = 0u;
  __syncthreads();
  if (penalty != 1.f) {                                           // rule 1
    for (int j = tid; j < len; j += kThreads) {
      const int64_t v = s[j];
      bool first = v >= 0 && v < V && v != pad_idx;
      for (int i = 0; first && i < j; ++i) first = s[i] != v;
      if (first) lp[v] = lp[v] * penalty;
    }
  }
  __syncthreads();
  if (ctx_penalty != 1.f) {                                       // C1: the position that finds its id's bit clear multiplies
    unsigned own = 0u;
#pragma unroll
    for (int i = 0; i < kCtxPerLane; ++i)
      if (w[i] >= 0) {
        const unsigned bit = 1u << (w[i] & 31);
        if (!(atomicOr(&seen[w[i] >> 5], bit) & bit)) own |= 1u << i;
      }
    float x[kCtxPerLane];                                         // the owned entries: loads together, then stores
#pragma unroll
    for (int i = 0; i < kCtxPerLane; ++i)
      if (own >> i & 1u) x[i] = lp[w[i]];
#pragma unroll
    for (int i = 0; i < kCtxPerLane; ++i)
      if (own >> i & 1u) lp[w[i]] = x[i] * ctx_penalty;
  }
  __syncthreads();
  if (ngram >= 1 && len >= ngram) {                               // rule 2
    const int tail = len - ngram + 1;                             // the last n - 1 tokens: s[tail .. t]
    for (int j = tid; j <= len - ngram; j += kThreads) {
      bool match = true;
      for (int i = 0; match && i < ngram - 1; ++i) match = s[j + i] == s[tail + i];
      const int64_t v = s[j + ngram - 1];
      if (match && v >= 0 && v < V) lp[v] = -INFINITY;
    }
  }
  __syncthreads();
  if (ctx_ngram >= 1 && len >= ctx_ngram) {                       // C2: t >= n_c - 1, so the tail starts at s[1] or later
    const int tail = len - ctx_ngram + 1;
#pragma unroll
    for (int i = 0; i < kCtxPerLane; ++i) {                       // position p is the follower of the window that ends at p
      const int p = tid + i * kThreads;
      bool match = w[i] >= 0 && p >= ctx_ngram - 1;
      for (int k = ctx_ngram - 2; match && k >= 0; --k) {         // the newest tail token first: most windows fail there
        const int u = c[p - ctx_ngram + 1 + k];
        match = u >= 0 && (int64_t)u == s[tail + k];
      }
      if (match) lp[w[i]] = -INFINITY;
    }
  }
  __syncthreads();
  if (tid == 0 && t < min_len) lp[end_idx] = -INFINITY;           // rule 3
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

extern "C" int bmhrl_logit_rules_ctx(float* logp, int64_t ld, int32_t rows, int32_t V, const int64_t* hist, int64_t ld_hist,
                                     const int64_t* t, int32_t ngram, int32_t min_len, float penalty, int32_t end_idx,
                                     int32_t pad_idx, const int64_t* ctx, int64_t ld_ctx, int32_t rows_per_ctx,
                                     int32_t ctx_ngram, float ctx_penalty, bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(logp && hist && t && ctx);
  BMHRL_CHECK_ARG(rows >= 1 && V >= 1 && V <= BMHRL_LOGIT_RULES_CTX_MAX_V && ld >= V);
  BMHRL_CHECK_ARG(ld_hist >= 1 && ld_hist <= BMHRL_LOGIT_RULES_MAX_HIST);
  BMHRL_CHECK_ARG(ngram >= 0 && min_len >= 0 && penalty > 0.f && penalty < INFINITY);
  BMHRL_CHECK_ARG(end_idx >= 0 && end_idx < V && pad_idx >= 0 && pad_idx < V);
  BMHRL_CHECK_ARG(ld_ctx >= 1 && ld_ctx <= BMHRL_LOGIT_RULES_MAX_CTX);
  BMHRL_CHECK_ARG(rows_per_ctx >= 1 && rows % rows_per_ctx == 0);
  BMHRL_CHECK_ARG(ctx_ngram >= 0 && ctx_penalty > 0.f && ctx_penalty < INFINITY);
  hipLaunchKernelGGL(logit_rules_ctx_kernel, dim3((unsigned)rows), dim3(kThreads), 0, S_(stream), logp, (long)ld, V, hist,
                     (long)ld_hist, t, ngram, min_len, penalty, end_idx, pad_idx, ctx, (int)ld_ctx, rows_per_ctx, ctx_ngram,
                     ctx_penalty);
  return hip_status(hipGetLastError());
}
