// Beam-search caption decoding (bmhrl_amd/decode.py BeamDecoder and GroupBeamDecoder): the per-token top-K selection over the
// K*V candidates of every sample, plain or in groups, and the reorder of every per-beam state buffer by parent beam.  All read
// the step position t from a device word, so they sit inside the decoder's captured token step.
//
// bmhrl_beam_select and bmhrl_group_beam_select are two instantiations of one body, select_kernel<KT, kGroups>: one
// 1024-thread workgroup per sample, one launch per token step.  The sample's scores and flags go to LDS before anything is
// written (the outputs may alias them).  The K beams form G groups of K' = K / G that choose one after another (rules G1-G4 of
// decode.py's "group beam search" section); the plain select is G = 1 with the grouped-only places compiled out, so its group
// loop folds away and K' = K.  Per group:
//   * every lane walks 4-token chunks of the group's K' log-prob rows (16-byte loads when the rows allow it, four chunks in
//     flight per lane) and keeps its own best KT >= K' candidates as a sorted register list (fully unrolled insertion: the
//     list never leaves registers), keyed on (a, k*V + v); a = s = score + log-prob in the plain select and
//     a = s - penalty * c in the grouped one (rule G3), c counting the earlier groups' beams that have just chosen the token;
//   * K' rounds of a block arg-max over the list heads -- wave64 xor-shuffles, one LDS step across the 16 waves -- pop the
//     group's winners best first; the lane that owns a winner drops its head.  Candidate order is (a descending, flat index
//     k*V + v ascending): the order of a stable sort of -a, so the result is bit-exact to the host restatement, ties included;
//   * (grouped only) the winners that are candidates of a live beam enter a table of (token, count) -- at most K - K' <= 15
//     entries -- and set the token's bit in an LDS bitmap (rule G2).
// The next group's pass reads one bitmap word per chunk and walks the table only for tokens whose bit is set, so the common
// candidate costs no compare chain.  The bitmap has 16384 bits; token v owns bit v mod 16384, so a larger vocabulary shares
// bits and a shared bit only sends a token through the table walk, which is exact.
// The penalty steers the choice only (rule G4): a winner's score is recomputed as score[parent] + logp[parent][v], the same
// single fp32 add as in the pass, so it is s bit for bit in both instantiations.  No atomics, no floating-point sum across
// lanes.
//
// bmhrl_beam_reorder: slot j of every per-beam buffer takes rows [0, t] of its parent beam.  A permutation in place is
// unsafe (a slot can be a parent of another slot), so the decoder runs it twice: phase 0 gathers the moved rows into a
// scratch image, phase 1 copies them back.  Slots whose parent is themselves move nothing in either phase.  The work is
// cut into 16 KiB chunks of one (buffer, slot) row; the grid covers every buffer's full row and chunks beyond the rows
// [0, t] of this step return at once.
//
// Contraction to FMA is off in the whole file.  Only the grouped pass needs it (penalty * c, then the subtract); the plain
// pass forms no product that feeds a sum and the reorder kernel moves bytes, so nothing changes for them.
#include <climits>
#include <cmath>
#include "common.h"
#include "../../include/bmhrl_hip.h"

#pragma clang fp contract(off)

#define S_(x) ((hipStream_t)(x))

namespace {

constexpr int kSelThreads = 1024;
constexpr int kSelWaves = kSelThreads / WAVE;
constexpr int kSelUnroll = 4;
constexpr int kMaxBeams = 16;
constexpr int kMapBits = 16384;               // bits of the chosen-token bitmap (a power of two, a multiple of 32)
constexpr int kMapWords = kMapBits / 32;

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

// kGroups false: the plain select.  n_groups and penalty are not read, G is the constant 1 and K' = K.
template <int KT, bool kGroups>
__global__ __launch_bounds__(kSelThreads) void select_kernel(
    const float* __restrict__ logp, long ld, const float* scores_in, const uint8_t* fin_in, float* scores_out,
    uint8_t* fin_out, int32_t* __restrict__ parent, int64_t* __restrict__ tok, int64_t* __restrict__ hist, long ldh,
    int hist_cols, const int64_t* __restrict__ tdev, int32_t* __restrict__ last_live, int K, int n_groups, int V, int end_idx,
    int pad_idx, float penalty) {
  __shared__ float s_score[kMaxBeams];
  __shared__ int s_fin[kMaxBeams];
  __shared__ float w_s[2][kSelWaves];
  __shared__ int w_i[2][kSelWaves];
  __shared__ int win_i[kMaxBeams];
  // grouped only (the plain instantiation does not touch them, so they take no LDS there)
  __shared__ unsigned s_map[kMapWords];        // bit (v mod kMapBits): an earlier group's live beam chose a token of that class
  __shared__ int s_ptok[kMaxBeams];            // the tokens earlier groups' live beams chose at this step ...
  __shared__ int s_pcnt[kMaxBeams];            // ... and how many beams chose each (c of rule G2)
  __shared__ int s_np;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
  const int G = kGroups ? n_groups : 1;
  const int Kp = K / G;
  const long row0 = (long)b * K;
  if (tid < K) {
    s_score[tid] = scores_in[row0 + tid];
    s_fin[tid] = fin_in[row0 + tid] != 0;
  }
  if constexpr (kGroups) {
    if (tid < kMapWords) s_map[tid] = 0u;
    if (tid == 0) s_np = 0;
  }
  __syncthreads();

  const int nch = (V + 3) >> 2;              // 4-token chunks per row
  const int total = Kp * nch;                // chunks of one group
  const float* base = logp + row0 * ld;
  const bool vec = (ld & 3) == 0 && (reinterpret_cast<uintptr_t>(base) & 15) == 0;

  for (int g = 0; g < G; ++g) {
    const int k0 = g * Kp;                   // the group's first beam
    float ls[KT];
    int li[KT];
#pragma unroll
    for (int q = 0; q < KT; ++q) { ls[q] = -INFINITY; li[q] = INT_MAX; }
    // a finished beam offers exactly one candidate: (k, pad) with its score unchanged, never penalised
    if (tid < Kp && s_fin[k0 + tid]) list_insert<KT>(ls, li, s_score[k0 + tid], (k0 + tid) * V + pad_idx);

    int np = 0;                              // table entries of groups 0 .. g-1
    if constexpr (kGroups) np = s_np;
    // a rotating window of kSelUnroll chunks per lane: the loads of the next chunks are in flight while one is ranked
    auto load = [&](int c, int& k, int& v0) {
      f32x4 x{0.f, 0.f, 0.f, 0.f};
      k = c < total ? k0 + c / nch : -1;
      if (k >= 0 && s_fin[k]) k = -1;
      v0 = k >= 0 ? (c - (k - k0) * nch) * 4 : 0;
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
        unsigned marks = 0u;
        // v0 is a multiple of 4: the chunk's four bits lie in one word of the bitmap
        if constexpr (kGroups) marks = (s_map[(v0 & (kMapBits - 1)) >> 5] >> (v0 & 31)) & 0xFu;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (v0 + e < V) {
            const float s = sc + cur[e];
            float a = s;
            if constexpr (kGroups) {
              if ((marks >> e) & 1u) {
                int cnt = 0;
                for (int q = 0; q < np; ++q)
                  if (s_ptok[q] == v0 + e) cnt = s_pcnt[q];
                if (cnt > 0) {
                  const float pen = penalty * (float)cnt;     // one multiply, then one subtract (rule G3)
                  a = s - pen;
                }
              }
            }
            list_insert<KT>(ls, li, a, i0 + e);
          }
      }
    }

    // K' rounds of a block arg-max over the list heads
    for (int j = 0; j < Kp; ++j) {
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
      if (tid == 0) win_i[k0 + j] = i;
    }
    __syncthreads();
    // the group's choices that were candidates of a live beam count against the groups after it (rule G2)
    if constexpr (kGroups) {
      if (g + 1 < G) {
        if (tid == 0) {
          int n = s_np;
          for (int j = 0; j < Kp; ++j) {
            const int idx = win_i[k0 + j];
            if (idx == INT_MAX) continue;
            const int p = idx / V, v = idx - p * V;
            if (s_fin[p]) continue;
            int q = 0;
            while (q < n && s_ptok[q] != v) ++q;
            if (q < n) {
              ++s_pcnt[q];
            } else if (n < kMaxBeams) {
              s_ptok[n] = v;
              s_pcnt[n] = 1;
              ++n;
              s_map[(v & (kMapBits - 1)) >> 5] |= 1u << (v & 31);
            }
          }
          s_np = n;
        }
        __syncthreads();
      }
    }
  }

  if (tid < K) {
    const int idx = win_i[tid];
    const long r = row0 + tid;
    if (idx != INT_MAX) {                      // (always: a group has at least K' candidates, K' <= V)
      const int p = idx / V, v = idx - p * V;
      const bool fin = s_fin[p] || v == end_idx;
      // the score is s, not a: the same single add as in the pass (a finished parent keeps its score)
      scores_out[r] = s_fin[p] ? s_score[p] : s_score[p] + base[(long)p * ld + v];
      fin_out[r] = fin ? 1 : 0;
      parent[r] = p;
      tok[r] = v;
      const long t = tdev[0];
      if (t + 1 < hist_cols) hist[r * ldh + t + 1] = v;
      if (!fin) last_live[0] = (int32_t)(t + 1);          // every writer stores the same value
    }
  }
}

// the launch both entry points share, after their own argument checks: KT follows K' = K / G, not K
template <bool kGroups>
int launch_select(const float* logp, int64_t ld, const float* scores_in, const uint8_t* finished_in, float* scores_out,
                  uint8_t* finished_out, int32_t* parent, int64_t* tok, int64_t* hist, int64_t ldh, int32_t hist_cols,
                  const int64_t* t, int32_t* last_live, int32_t B, int32_t K, int32_t G, int32_t V, int32_t end_idx,
                  int32_t pad_idx, float penalty, bmhrl_stream_t stream) {
  const dim3 grid(B), block(kSelThreads);
  const int Kp = K / G;
#define LAUNCH(KT)                                                                                                        \
  hipLaunchKernelGGL((select_kernel<KT, kGroups>), grid, block, 0, S_(stream), logp, (long)ld, scores_in, finished_in,  \
                     scores_out, finished_out, parent, tok, hist, (long)ldh, hist_cols, t, last_live, K, G, V, end_idx,  \
                     pad_idx, penalty)
  if (Kp == 1) LAUNCH(1);
  else if (Kp == 2) LAUNCH(2);
  else if (Kp <= 4) LAUNCH(4);
  else if (Kp <= 8) LAUNCH(8);
  else LAUNCH(16);
#undef LAUNCH
  return hip_status(hipGetLastError());
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
  return launch_select<false>(logp, ld, scores_in, finished_in, scores_out, finished_out, parent, tok, hist, ldh, hist_cols, t,
                              last_live, B, K, 1, V, end_idx, pad_idx, 0.f, stream);
}

// G = 1 launches the grouped instantiation too: it is what tests/test_group_beam_gpu.py compares with the plain one
extern "C" int bmhrl_group_beam_select(const float* logp, int64_t ld, const float* scores_in, const uint8_t* finished_in,
                                       float* scores_out, uint8_t* finished_out, int32_t* parent, int64_t* tok,
                                       int64_t* hist, int64_t ldh, int32_t hist_cols, const int64_t* t, int32_t* last_live,
                                       int32_t B, int32_t K, int32_t V, int32_t end_idx, int32_t pad_idx, int32_t G,
                                       float diversity_penalty, bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(logp && scores_in && finished_in && scores_out && finished_out && parent && tok && hist && t && last_live);
  BMHRL_CHECK_ARG(B > 0 && K >= 1 && K <= kMaxBeams && G >= 1 && K % G == 0 && V >= K / G);
  BMHRL_CHECK_ARG(ld >= V && ldh >= hist_cols && hist_cols >= 1);
  BMHRL_CHECK_ARG((int64_t)K * V < INT_MAX && pad_idx >= 0 && pad_idx < V);
  BMHRL_CHECK_ARG(diversity_penalty >= 0.f && diversity_penalty < INFINITY);     // (a NaN fails the first comparison)
  return launch_select<true>(logp, ld, scores_in, finished_in, scores_out, finished_out, parent, tok, hist, ldh, hist_cols, t,
                             last_live, B, K, G, V, end_idx, pad_idx, diversity_penalty, stream);
}

extern "C" int bmhrl_beam_reorder(const bmhrl_beam_buffer* table, int32_t n_buffers, int64_t n_blocks, const int32_t* parent,
                                  int32_t rows, int32_t K, const int64_t* t, int32_t phase, bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(table && parent && t && n_buffers > 0 && rows > 0 && K >= 1 && rows % K == 0);
  BMHRL_CHECK_ARG(n_blocks > 0 && n_blocks < INT_MAX && (phase == 0 || phase == 1));
  hipLaunchKernelGGL(beam_reorder_kernel, dim3((unsigned)n_blocks), dim3(kReThreads), 0, S_(stream), table, n_buffers, parent,
                     rows, K, t, phase);
  return hip_status(hipGetLastError());
}
