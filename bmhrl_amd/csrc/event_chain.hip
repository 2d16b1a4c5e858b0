// Event-chain selection for gfx950: from the (start, end, score) rows a video's proposals already
// are, the time-ordered chain of at most L events that maximises the sum of (score - cost) minus a penalty on the overlap
// of neighbours, exactly, by dynamic programming.  One launch for the batch, one 512-thread workgroup per video, on the
// caller's stream and with no host read: the input is bmhrl_proposal_select's / bmhrl_proposal_select_soft's (props, count)
// as they stand.
//
//   load     a thread owns rows tid and tid + 512: eligibility and gain, rows to LDS
//   rank     an eligible row's position is the number of eligible rows before it in (start, end, row) order (n^2 compares,
//            every thread reads every row once); the rows are scattered to their positions
//   levels   V[l][j] = max over linked i < j of (V[l-1][i] - (lambda * t_ij)) + g_j, a thread scanning the positions before
//            its own (positions tid and 1023 - tid: every thread scans about the same number).  Two alternating rows of V,
//            one barrier per level, the parents of every level kept as uint16.  A level that defined nothing ends the loop
//            (read from LDS behind the barrier: every thread takes the same exit)
//   answer   the 64-bit key (image(V) << 32) | ((32 - l) << 16) | (1023 - j) is largest for the largest V, then the smaller
//            l, then the earlier j; wave maxima, one LDS slot per wave.  Thread 0 walks the parents back and writes the
//            chain, every thread the zeros behind it.
//
// The definition (include/bmhrl_hip.h) is in fp32 in a stated order.  Nothing here may be contracted or reassociated:
#pragma clang fp contract(off)
#include <cmath>
#include "common.h"
#include "../../include/bmhrl_hip.h"

namespace {

constexpr int kThreads = 512;
constexpr int kMaxP = BMHRL_PROPOSAL_CHAIN_MAX_P;
constexpr int kMaxL = BMHRL_PROPOSAL_CHAIN_MAX_L;
constexpr int kRows = kMaxP / kThreads;                 // rows (and positions) a thread owns
constexpr int kWaves = kThreads / WAVE;
static_assert(kRows == 2 && kMaxP - 1 <= 0xFFFF && kMaxL <= 0xFFFF, "two rows per thread; parents are uint16");

#define S_(s) ((hipStream_t)(s))

// order-preserving image of a float, and back
__device__ __forceinline__ uint32_t order_key(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t u) {
  return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
}
// larger = larger value, then smaller level, then earlier position.  Never 0 for 1 <= l <= kMaxL: 0 marks "nothing".
__device__ __forceinline__ uint64_t answer_key(float v, int l, int pos) {
  return ((uint64_t)order_key(v) << 32) | (uint64_t)(((uint32_t)(kMaxL + 1 - l) << 16) | (uint32_t)(kMaxP - 1 - pos));
}

__device__ __forceinline__ uint64_t wave_max_key(uint64_t v) {
  for (int o = 32; o > 0; o >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, o, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), o, 64);
    const uint64_t w = ((uint64_t)hi << 32) | (uint64_t)lo;
    v = w > v ? w : v;
  }
  return v;
}

// (s1, e1, r1) before (s2, e2, r2)
__device__ __forceinline__ bool before(float s1, float e1, int r1, float s2, float e2, int r2) {
  return s1 < s2 || (s1 == s2 && (e1 < e2 || (e1 == e2 && r1 < r2)));
}

// grid (B), kThreads threads.  LDS: 16 KiB rows by position, 8 KiB raw rows, 8 KiB V, 62 KiB parents.
__global__ __launch_bounds__(kThreads) void event_chain_kernel(const float* __restrict__ props, const int* __restrict__ count,
                                                               int P, int L, float max_tiou, float overlap_weight,
                                                               float event_cost, float min_length,
                                                               float* __restrict__ events, int* __restrict__ chain,
                                                               int* __restrict__ length, float* __restrict__ value) {
  __shared__ float raw_s[kMaxP], raw_e[kMaxP];          // by row; an ineligible row has NaN in raw_s
  __shared__ float st[kMaxP], en[kMaxP], gn[kMaxP];     // by position
  __shared__ int rw[kMaxP];
  __shared__ float V[2][kMaxP];                         // V[l & 1][position]; -INFINITY = undefined
  __shared__ uint16_t parent[kMaxL - 1][kMaxP];         // parent[l - 2][position], l = 2 .. L
  __shared__ int defined[kMaxL + 1];                    // defined[l]: level l has a value
  __shared__ uint64_t slot[kWaves];
  const long b = blockIdx.x;
  const int tid = threadIdx.x;
  const float* in = props + b * (long)P * 3;
  int cnt = P;
  if (count) cnt = min(max(count[b], 0), P);

  // ---- load: eligibility and gain of the thread's rows
  float rs[kRows], re[kRows], rg[kRows];
  bool ok[kRows];
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    const int row = tid + r * kThreads;
    rs[r] = re[r] = rg[r] = 0.f;
    ok[r] = false;
    if (row < cnt) {
      const float s = in[row * 3 + 0], e = in[row * 3 + 1], score = in[row * 3 + 2];
      const float g = score - event_cost;
      rs[r] = s;
      re[r] = e;
      rg[r] = g;
      ok[r] = (e - s) > min_length && score == score && g > 0.f;
    }
    if (row < P) {                    // (P <= kMaxP: checked by the entry point)
      raw_s[row] = ok[r] ? rs[r] : NAN;
      raw_e[row] = re[r];
    }
  }
  if (tid <= kMaxL) defined[tid] = 0;
  __syncthreads();

  // ---- rank: the eligible rows before this one; n = all eligible rows.  A NaN start compares false with everything.
  int rank[kRows] = {0, 0};
  int n = 0;
  for (int k = 0; k < cnt; ++k) {
    const float s = raw_s[k], e = raw_e[k];
    n += s == s;
#pragma unroll
    for (int r = 0; r < kRows; ++r) rank[r] += before(s, e, k, rs[r], re[r], tid + r * kThreads);
  }
#pragma unroll
  for (int r = 0; r < kRows; ++r)
    if (ok[r]) {                      // rank < n <= cnt <= kMaxP: the order is total, so the ranks are 0 .. n - 1
      const int p = min(rank[r], kMaxP - 1);
      st[p] = rs[r];
      en[p] = re[r];
      gn[p] = rg[r];
      rw[p] = tid + r * kThreads;
      V[1][p] = rg[r];
    }
  __syncthreads();

  // ---- levels.  The thread's positions: tid and kMaxP - 1 - tid (where below n).
  int pos[kRows] = {tid, kMaxP - 1 - tid};
  float sj[kRows], ej[kRows], gj[kRows];
  uint64_t best = 0;
#pragma unroll
  for (int r = 0; r < kRows; ++r) {
    sj[r] = ej[r] = gj[r] = 0.f;
    if (pos[r] < n) {
      sj[r] = st[pos[r]];
      ej[r] = en[pos[r]];
      gj[r] = gn[pos[r]];
      const uint64_t key = answer_key(gj[r], 1, pos[r]);
      best = key > best ? key : best;
    }
  }
  for (int l = 2; l <= L; ++l) {
    const float* Vp = V[(l - 1) & 1];
    float* Vn = V[l & 1];
    bool any = false;
#pragma unroll
    for (int r = 0; r < kRows; ++r) {
      const int j = pos[r];
      if (j >= n) continue;
      float top = -INFINITY;
      int par = 0;
      for (int i = 0; i < j; ++i) {
        const float v = Vp[i], e1 = en[i];
        if (!(v > -INFINITY) || !(e1 <= ej[r])) continue;
        const float s1 = st[i], s2 = sj[r], e2 = ej[r];
        const float inter = fmaxf(fminf(e1, e2) - fmaxf(s1, s2), 0.f);
        float uni = (e1 - s1) + (e2 - s2) - inter;
        uni = fminf(fmaxf(e1, e2) - fminf(s1, s2), uni);
        const float t = inter / (uni + 1e-8f);
        if (!(t <= max_tiou)) continue;
        const float cand = (v - (overlap_weight * t)) + gj[r];
        if (cand > top) {
          top = cand;
          par = i;
        }
      }
      Vn[j] = top;
      if (top > -INFINITY) {
        parent[l - 2][j] = (uint16_t)par;
        const uint64_t key = answer_key(top, l, j);
        best = key > best ? key : best;
        any = true;
      }
    }
    if (any) defined[l] = 1;
    __syncthreads();
    if (!defined[l]) break;           // (the same word in every thread: a uniform exit)
  }

  // ---- answer
  best = wave_max_key(best);
  if ((tid & (WAVE - 1)) == 0) slot[tid / WAVE] = best;
  __syncthreads();
  best = slot[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) best = slot[w] > best ? slot[w] : best;
  int len = 0;
  if (best != 0) len = kMaxL + 1 - (int)(((uint32_t)best >> 16) & 0xFFFFu);
  len = min(max(len, 0), L);
  float* out = events + b * (long)L * 3;
  int* out_chain = chain + b * (long)L;
  if (tid == 0) {
    int p = kMaxP - 1 - (int)((uint32_t)best & 0xFFFFu);
    for (int l = len; l >= 1; --l) {
      p = min(max(p, 0), kMaxP - 1);
      const int row = min(max(rw[p], 0), P - 1);
      out[(l - 1) * 3 + 0] = in[row * 3 + 0];
      out[(l - 1) * 3 + 1] = in[row * 3 + 1];
      out[(l - 1) * 3 + 2] = in[row * 3 + 2];
      out_chain[l - 1] = row;
      if (l >= 2) p = parent[l - 2][p];
    }
    length[b] = len;
    if (value) value[b] = len > 0 ? key_value((uint32_t)(best >> 32)) : 0.f;
  }
  for (int j = len + tid; j < L; j += kThreads) {       // behind the chain
    out[j * 3 + 0] = 0.f;
    out[j * 3 + 1] = 0.f;
    out[j * 3 + 2] = 0.f;
    out_chain[j] = -1;
  }
}

}  // namespace

extern "C" int bmhrl_proposal_chain(const float* props, const int32_t* count, int32_t B, int32_t P, int32_t max_events,
                                    float max_tiou, float overlap_weight, float event_cost, float min_length, float* events,
                                    int32_t* chain, int32_t* length, float* value, bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(props && events && chain && length && B >= 1 && B <= 65535);
  BMHRL_CHECK_ARG(P >= 1 && P <= BMHRL_PROPOSAL_CHAIN_MAX_P && max_events >= 1 && max_events <= BMHRL_PROPOSAL_CHAIN_MAX_L);
  // (a NaN fails every comparison)
  BMHRL_CHECK_ARG(max_tiou >= 0.f && overlap_weight >= 0.f && event_cost >= 0.f && min_length >= 0.f);
  hipLaunchKernelGGL(event_chain_kernel, dim3((unsigned)B), dim3(kThreads), 0, S_(stream), props, count, P, max_events, max_tiou,
                     overlap_weight, event_cost, min_length, events, chain, length, value);
  return hip_status(hipGetLastError());
}
