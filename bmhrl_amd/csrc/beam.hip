// Beam-search caption decoding (bmhrl_amd/decode.py BeamDecoder): the per-token top-K selection over the K*V candidates of
// every sample, and the reorder of every per-beam state buffer by parent beam.  Both read the step position t from a
// device word, so they sit inside the decoder's captured token step.
//
// bmhrl_beam_select: one 1024-thread workgroup per sample.  Every lane walks 4-token chunks of the sample's K log-prob rows
// (16-byte loads when the rows allow it, four chunks in flight per lane) and keeps its own best KT >= K candidates as a
// sorted register list (fully unrolled insertion: the list never leaves registers).  Then K rounds of a block arg-max over
// the list heads -- wave64 xor-shuffles, one LDS step across the 16 waves -- pop the winners best first; the lane that
// owns a winner drops its head.  Candidate order is (score descending, flat index k*V + v ascending): the order of a
// stable sort of -score, so the result is bit-exact to the host restatement, ties included.
//
// bmhrl_beam_reorder: slot j of every per-beam buffer takes rows [0, t] of its parent beam.  A permutation in place is
// unsafe (a slot can be a parent of another slot), so the decoder runs it twice: phase 0 gathers the moved rows into a
// scratch image, phase 1 copies them back.  Slots whose parent is themselves move nothing in either phase.  The work is
// cut into 16 KiB chunks of one (buffer, slot) row; the grid covers every buffer's full row and chunks beyond the rows
// [0, t] of this step return at once.
#include <climits>
#include "common.h"
#include "../../include/bmhrl_hip.h"

#define S_(x) ((hipStream_t)(x))

namespace {

constexpr int kSelThreads = 1024;
constexpr int kSelWaves = kSelThreads / WAVE;
constexpr int kSelUnroll = 4;
constexpr int kMaxBeams = 16;

__device__ __forceinline__ bool beats(float sa, int ia, float sb, int ib) {
  return sa > sb || (sa == sb && ia < ib);
}

// sorted insertion as selects only (the list stays in registers): entries the candidate beats move down one place
template <int KT>
__device__ __forceinline__ void list_insert(float (&ls)[KT], int (&li)[KT], float s, int i) {
  if (!beats(s, i, ls[KT - 1], li[KT - 1])) return;
#pragma unroll
  for (int q = KT - 1; q > 0; --q) {
    const bool here = beats(s, i, ls[q], li[q]), above = beats(s, i, ls[q - 1], li[q - 1]);
    ls[q] = above ? ls[q - 1] : (here ? s : ls[q]);
    li[q] = above ? li[q - 1] : (here ? i : li[q]);
  }
  if (beats(s, i, ls[0], li[0])) { ls[0] = s; li[0] = i; }
}

template <int KT>
__global__ __launch_bounds__(kSelThreads) void beam_select_kernel(
    const float* __restrict__ logp, long ld, const float* scores_in, const uint8_t* fin_in, float* scores_out,
    uint8_t* fin_out, int32_t* __restrict__ parent, int64_t* __restrict__ tok, int64_t* __restrict__ hist, long ldh,
    int hist_cols, const int64_t* __restrict__ tdev, int32_t* __restrict__ last_live, int K, int V, int end_idx,
    int pad_idx) {
  __shared__ float s_score[kMaxBeams];
  __shared__ int s_fin[kMaxBeams];
  __shared__ float w_s[2][kSelWaves];
  __shared__ int w_i[2][kSelWaves];
  __shared__ float win_s[kMaxBeams];
  __shared__ int win_i[kMaxBeams];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const long row0 = (long)b * K;
  if (tid < K) {
    s_score[tid] = scores_in[row0 + tid];
    s_fin[tid] = fin_in[row0 + tid] != 0;
  }
  __syncthreads();

  float ls[KT];
  int li[KT];
#pragma unroll
  for (int q = 0; q < KT; ++q) { ls[q] = -INFINITY; li[q] = INT_MAX; }
  // a finished beam offers exactly one candidate: (k, pad) with its score unchanged
  if (tid < K && s_fin[tid]) list_insert<KT>(ls, li, s_score[tid], tid * V + pad_idx);

  const int nch = (V + 3) >> 2;              // 4-token chunks per row
  const int total = K * nch;
  const float* base = logp + row0 * ld;
  const bool vec = (ld & 3) == 0 && (reinterpret_cast<uintptr_t>(base) & 15) == 0;
  // a rotating window of kSelUnroll chunks per lane: the loads of the next chunks are in flight while one is ranked
  auto load = [&](int c, int& k, int& v0) {
    f32x4 x{0.f, 0.f, 0.f, 0.f};
    k = c < total ? c / nch : -1;
    if (k >= 0 && s_fin[k]) k = -1;
    v0 = k >= 0 ? (c - k * nch) * 4 : 0;
    if (k >= 0) {
      const float* p = base + (long)k * ld + v0;
      if (vec && v0 + 4 <= V) {
        x = *reinterpret_cast<const f32x4*>(p);
      } else {
        x[0] = p[0];
        if (v0 + 1 < V) x[1] = p[1];
        if (v0 + 2 < V) x[2] = p[2];
        if (v0 + 3 < V) x[3] = p[3];
      }
    }
    return x;
  };
  f32x4 x[kSelUnroll];
  int kk[kSelUnroll], vv[kSelUnroll];
#pragma unroll
  for (int u = 0; u < kSelUnroll; ++u) x[u] = load(tid + u * kSelThreads, kk[u], vv[u]);
#pragma unroll 1
  for (int c = tid; c < total; c += kSelThreads) {
    const f32x4 cur = x[0];
    const int k = kk[0], v0 = vv[0];
#pragma unroll
    for (int u = 0; u < kSelUnroll - 1; ++u) { x[u] = x[u + 1]; kk[u] = kk[u + 1]; vv[u] = vv[u + 1]; }
    x[kSelUnroll - 1] = load(c + kSelUnroll * kSelThreads, kk[kSelUnroll - 1], vv[kSelUnroll - 1]);
    if (k >= 0) {
      const float sc = s_score[k];
      const int i0 = k * V + v0;
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (v0 + e < V) list_insert<KT>(ls, li, sc + cur[e], i0 + e);
    }
  }

  // K rounds of a block arg-max over the list heads
  for (int j = 0; j < K; ++j) {
    float s = ls[0];
    int i = li[0];
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) {
      const float s2 = __shfl_xor(s, o, WAVE);
      const int i2 = __shfl_xor(i, o, WAVE);
      if (beats(s2, i2, s, i)) { s = s2; i = i2; }
    }
    if (lane == 0) { w_s[j & 1][wave] = s; w_i[j & 1][wave] = i; }
    __syncthreads();                         // (double-buffered: round j + 1 writes the other half)
    s = w_s[j & 1][0];
    i = w_i[j & 1][0];
#pragma unroll
    for (int w = 1; w < kSelWaves; ++w)
      if (beats(w_s[j & 1][w], w_i[j & 1][w], s, i)) { s = w_s[j & 1][w]; i = w_i[j & 1][w]; }
    if (i != INT_MAX && li[0] == i) {        // flat indices are unique: exactly one lane owns the winner
#pragma unroll
      for (int q = 0; q < KT - 1; ++q) { ls[q] = ls[q + 1]; li[q] = li[q + 1]; }
      ls[KT - 1] = -INFINITY;
      li[KT - 1] = INT_MAX;
    }
    if (tid == 0) { win_s[j] = s; win_i[j] = i; }
  }
  __syncthreads();

  if (tid < K) {
    const int idx = win_i[tid];
    const int p = idx / V, v = idx - p * V;
    const bool fin = s_fin[p] || v == end_idx;
    const long r = row0 + tid;
    scores_out[r] = win_s[tid];
    fin_out[r] = fin ? 1 : 0;
    parent[r] = p;
    tok[r] = v;
    const long t = tdev[0];
    if (t + 1 < hist_cols) hist[r * ldh + t + 1] = v;
    if (!fin) last_live[0] = (int32_t)(t + 1);          // every writer stores the same value
  }
}

constexpr int kReThreads = 256;
constexpr long kReChunk = (long)kReThreads * 16 * 4;   // bytes of one (buffer, slot) row a workgroup moves

__device__ __forceinline__ long chunks_of(long beam_bytes) { return (beam_bytes + kReChunk - 1) / kReChunk; }

__global__ __launch_bounds__(kReThreads) void beam_reorder_kernel(const bmhrl_beam_buffer* __restrict__ table, int n,
                                                                  const int32_t* __restrict__ parent, int rows, int K,
                                                                  const int64_t* __restrict__ tdev, int phase) {
  long blk = blockIdx.x;
  int e = 0;
  for (; e < n; ++e) {
    const long nb = (long)rows * chunks_of(table[e].beam_bytes);
    if (blk < nb) break;
    blk -= nb;
  }
  if (e == n) return;
  const bmhrl_beam_buffer d = table[e];
  const long nchunk = chunks_of(d.beam_bytes);
  const int j = (int)(blk / nchunk);
  const long c = blk - (long)j * nchunk;
  int p = parent[j];
  p = p < 0 ? 0 : (p >= K ? K - 1 : p);
  const int src_row = j - j % K + p;
  if (src_row == j) return;
  // exactly rows [0, t]: position t + 1 of a row may already hold the new beam's own value (the token history)
  long nbytes = d.beam_bytes;
  if (d.pos_bytes > 0) nbytes = min(nbytes, (tdev[0] + 1) * d.pos_bytes);
  const long lo = c * kReChunk, hi = min(nbytes, lo + kReChunk);
  if (lo >= hi) return;
  const char* src;
  char* dst;
  if (phase == 0) {
    src = static_cast<const char*>(d.state) + (long)src_row * d.beam_bytes;
    dst = static_cast<char*>(d.scratch) + (long)j * d.beam_bytes;
  } else {
    src = static_cast<const char*>(d.scratch) + (long)j * d.beam_bytes;
    dst = static_cast<char*>(d.state) + (long)j * d.beam_bytes;
  }
  const bool vec = ((reinterpret_cast<uintptr_t>(d.state) | reinterpret_cast<uintptr_t>(d.scratch) | (uintptr_t)d.beam_bytes) & 15) == 0;
  long body = lo;                          // (chunks start at multiples of 16 KiB: 16-byte aligned when the rows are)
  if (vec) {
    const uint4* s4 = reinterpret_cast<const uint4*>(src + lo);
    uint4* d4 = reinterpret_cast<uint4*>(dst + lo);
    const int n16 = (int)((hi - lo) >> 4);
    uint4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = threadIdx.x + u * kReThreads;
      if (q < n16) v[u] = s4[q];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = threadIdx.x + u * kReThreads;
      if (q < n16) d4[q] = v[u];
    }
    body = lo + ((long)n16 << 4);
  }
  for (long q = body + threadIdx.x; q < hi; q += kReThreads) dst[q] = src[q];
}

}  // namespace

extern "C" int bmhrl_beam_select(const float* logp, int64_t ld, const float* scores_in, const uint8_t* finished_in,
                                 float* scores_out, uint8_t* finished_out, int32_t* parent, int64_t* tok, int64_t* hist,
                                 int64_t ldh, int32_t hist_cols, const int64_t* t, int32_t* last_live, int32_t B, int32_t K,
                                 int32_t V, int32_t end_idx, int32_t pad_idx, bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(logp && scores_in && finished_in && scores_out && finished_out && parent && tok && hist && t && last_live);
  BMHRL_CHECK_ARG(B > 0 && K >= 1 && K <= kMaxBeams && V >= K && ld >= V && ldh >= hist_cols && hist_cols >= 1);
  BMHRL_CHECK_ARG((int64_t)K * V < INT_MAX && pad_idx >= 0 && pad_idx < V);
  const dim3 grid(B), block(kSelThreads);
#define LAUNCH(KT)                                                                                                        \
  hipLaunchKernelGGL(beam_select_kernel<KT>, grid, block, 0, S_(stream), logp, (long)ld, scores_in, finished_in,        \
                     scores_out, finished_out, parent, tok, hist, (long)ldh, hist_cols, t, last_live, K, V, end_idx, pad_idx)
  if (K == 1) LAUNCH(1);
  else if (K == 2) LAUNCH(2);
  else if (K <= 4) LAUNCH(4);
  else if (K <= 8) LAUNCH(8);
  else LAUNCH(16);
#undef LAUNCH
  return hip_status(hipGetLastError());
}

extern "C" int bmhrl_beam_reorder(const bmhrl_beam_buffer* table, int32_t n_buffers, int64_t n_blocks, const int32_t* parent,
                                  int32_t rows, int32_t K, const int64_t* t, int32_t phase, bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(table && parent && t && n_buffers > 0 && rows > 0 && K >= 1 && rows % K == 0);
  BMHRL_CHECK_ARG(n_blocks > 0 && n_blocks < INT_MAX && (phase == 0 || phase == 1));
  hipLaunchKernelGGL(beam_reorder_kernel, dim3((unsigned)n_blocks), dim3(kReThreads), 0, S_(stream), table, n_buffers, parent,
                     rows, K, t, phase);
  return hip_status(hipGetLastError());
}
