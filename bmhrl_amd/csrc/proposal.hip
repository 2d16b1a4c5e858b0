// Temporal proposal generation for gfx950: what the anchor heads of the proposal generator need
// around their convolutions, on the caller's stream and with no host synchronisation:
//   proposal_assign  two launches: clear the owner map, then one thread per target row (best anchor by the centre-less tIoU of
//                    lengths, an integer atomic max of the row index on its cell: the LARGEST row owns a cell whatever order
//                    the rows arrive in; the row that finds the cell empty counts it)
//   proposal_head    one launch per head: decode (centre, length, confidence), the four loss terms and d total / d x.  One
//                    thread per (b, s, a) cell of a 16 x 16 tile; block sums in a fixed order, one partial row per block (write-through stores,
//                    drained before the block takes its ticket), and the block whose ticket is last reads the rows past
//                    its L1 and adds them in index order in fp64 -- equal inputs give equal bits
//   proposal_select  top-k by confidence + corner coordinates + trimming + greedy NMS for all videos of a batch.  Candidates
//                    are 64-bit keys (order-preserving image of conf, ~row index): all distinct, so a plain descending sort
//                    IS "conf descending, ties to the smaller row".  Each pass sorts chunks of 4096 keys in LDS and keeps
//                    the k largest of a chunk; passes repeat on the survivors until one chunk is left, which the last kernel
//                    sorts, gathers, trims and suppresses (k-step greedy loop, the inner comparison across the lanes).
//   proposal_select_soft  the same passes keeping a pool of m <= 1024 keys, then a last kernel that picks k times by the
//                    CURRENT score and lowers the scores of overlapping rows (Soft-NMS).
//
// Reference: utilities/proposal_utils.py (tiou_vectorized, select_topk_predictions, get_corner_coords, trim_proposals,
// non_max_suppresion), in fp32 and in its order of operations.  Nothing here may be contracted or reassociated:
#pragma clang fp contract(off)
#include <cfloat>
#include "common.h"
#include "../../include/bmhrl_hip.h"

namespace {

constexpr int kChunk = 4096;          // keys sorted per block (32 KiB of LDS)
constexpr int kSortThreads = 512;
constexpr int kHeadThreads = 256;
constexpr int kTile = 16;             // kTile * kTile == kHeadThreads cells per tile
constexpr int kHeadMaxBlocks = BMHRL_PROPOSAL_HEAD_BLOCKS;

#define S_(s) ((hipStream_t)(s))

// ------------------------------------------------------------------------------------------------ assignment
__global__ __launch_bounds__(256) void assign_clear_kernel(int* __restrict__ owner, long total, int* __restrict__ counts) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < total) owner[i] = -1;
  if (i == 0) {
    counts[0] = 0;
    counts[1] = (int)total;
  }
}

// tIoU of the segments (centre 0, length la) and (centre 0, length lb), the reference's arithmetic term for term
__device__ __forceinline__ float tiou_lengths(float la, float lb) {
  const float s1 = 0.f - la / 2.f, e1 = 0.f + la / 2.f;
  const float s2 = 0.f - lb / 2.f, e2 = 0.f + lb / 2.f;
  const float inter = fmaxf(fminf(e1, e2) - fmaxf(s1, s2), 0.f);
  float uni = (e1 - s1) + (e2 - s2) - inter;
  uni = fminf(fmaxf(e1, e2) - fminf(s1, s2), uni);
  return inter / (uni + 1e-8f);
}

__global__ __launch_bounds__(256) void assign_kernel(const float* __restrict__ targets, int n, const float* __restrict__ anchors,
                                                     int A, float cell_sec, int B, int S, int* __restrict__ owner,
                                                     float* __restrict__ tx, float* __restrict__ tw, int* __restrict__ counts) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const float vb = targets[4 * (long)r], centre = targets[4 * (long)r + 1], length = targets[4 * (long)r + 2];
  const float g = centre / cell_sec, w = length / cell_sec;
  const float fl = floorf(g);
  int best = 0;
  float best_t = -1.f;
  for (int a = 0; a < A; ++a) {
    const float t = tiou_lengths(anchors[a] / cell_sec, w);
    if (t > best_t) {                 // strict: ties stay with the smaller a
      best_t = t;
      best = a;
    }
  }
  tx[r] = g - fl;
  tw[r] = logf(w / (anchors[best] / cell_sec) + 1e-16f);
  // (comparisons written so that a NaN fails them)
  if (!(vb >= 0.f && vb < (float)B && fl >= 0.f && fl < (float)S)) return;
  const int b = (int)vb, cell = (int)fl;
  // a cell goes from -1 to owned exactly once, whoever arrives first: integer counts, independent of the order
  if (atomicMax(&owner[((long)b * A + best) * S + cell], r) < 0) {
    atomicAdd(&counts[0], 1);
    atomicSub(&counts[1], 1);
  }
}

// ------------------------------------------------------------------------------------------------ head
__device__ __forceinline__ float sigmoid_f(float z) {
  const float e = expf(-fabsf(z));
  return z >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}
__device__ __forceinline__ float softplus_f(float z) { return fmaxf(z, 0.f) + log1pf(expf(-fabsf(z))); }

// One block works on 16 x 16 (position, anchor) tiles of one video, tile after tile (grid stride): x and dx are (s, a)-major,
// pred and owner (a, s)-major, so the tile is read and computed with the anchor as the fastest thread index (48 contiguous
// floats of x / dx per position) and its predictions leave through LDS with the position fastest (48 contiguous floats per
// anchor).  A thread's four sums run over its tiles in tile order: with the grid fixed by the shape, a fixed order.
__global__ __launch_bounds__(kHeadThreads) void head_kernel(const float* __restrict__ x, const float* __restrict__ anchors,
                                                            float cell_sec, int S, int A, int nts, int nta, long n_tiles,
                                                            float* __restrict__ pred, long n_total, long row_off,
                                                            const int* __restrict__ owner, const float* __restrict__ tx,
                                                            const float* __restrict__ tw, const int* __restrict__ counts,
                                                            float obj_coeff, float noobj_coeff, const float* __restrict__ dscale,
                                                            float* __restrict__ dx, float* __restrict__ sums, float* partials,
                                                            unsigned* counter) {
  __shared__ float p_sh[kTile][kTile * 3 + 1];       // [anchor][position * 3 + channel], odd row stride
  __shared__ int own_sh[kTile][kTile + 1];           // [anchor][position]
  __shared__ float red[4][kHeadThreads / WAVE];
  __shared__ double fin[4][kHeadThreads];
  __shared__ int last_sh;
  const int tid = threadIdx.x;
  float t_x = 0.f, t_w = 0.f, t_obj = 0.f, t_noobj = 0.f;
  float inv_obj = 0.f, inv_noobj = 0.f;
  if (owner) {
    const int n_obj = counts[0], n_noobj = counts[1];
    inv_obj = n_obj > 0 ? 1.f / (float)n_obj : 0.f;
    inv_noobj = n_noobj > 0 ? 1.f / (float)n_noobj : 0.f;
  }
  const float g = (dx && dscale) ? dscale[0] : 1.f;
  for (long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const int s0 = (int)(t % nts) * kTile, a0 = (int)((t / nts) % nta) * kTile;
    const long b = t / ((long)nts * nta);
    if (owner) {                      // the tile of the owner map, position fastest
      const int sl = tid % kTile, al = tid / kTile;
      const int s = s0 + sl, a = a0 + al;
      own_sh[al][sl] = (s < S && a < A) ? owner[(b * A + a) * S + s] : -1;
    }
    __syncthreads();
    {                                 // decode, loss terms and gradient, anchor fastest
      const int al = tid % kTile, sl = tid / kTile;
      const int s = s0 + sl, a = a0 + al;
      if (s < S && a < A) {
        const long xo = ((b * S + s) * A + a) * 3;
        const float c = x[xo], l = x[xo + 1], o = x[xo + 2];
        const float sc = sigmoid_f(c);
        p_sh[al][sl * 3 + 0] = (sc + (float)s) * cell_sec;
        p_sh[al][sl * 3 + 1] = anchors[a] * expf(l);
        p_sh[al][sl * 3 + 2] = sigmoid_f(o);
        if (owner) {
          const int r = own_sh[al][sl];
          float d_c = 0.f, d_l = 0.f, d_o;
          if (r >= 0) {
            const float ex = sc - tx[r], ew = l - tw[r];
            t_x += ex * ex;
            t_w += ew * ew;
            t_obj += softplus_f(-o);
            d_c = 2.f * ex * sc * (1.f - sc) * inv_obj;
            d_l = 2.f * ew * inv_obj;
            d_o = -obj_coeff * sigmoid_f(-o) * inv_obj;
          } else {
            t_noobj += softplus_f(o);
            d_o = noobj_coeff * sigmoid_f(o) * inv_noobj;
          }
          if (dx) {
            dx[xo] = g * d_c;
            dx[xo + 1] = g * d_l;
            dx[xo + 2] = g * d_o;
          }
        }
      }
    }
    __syncthreads();
    for (int e = tid; e < kTile * kTile * 3; e += kHeadThreads) {      // the tile's predictions, position fastest
      const int al = e / (kTile * 3), rem = e % (kTile * 3);
      const int s = s0 + rem / 3, a = a0 + al;
      if (s < S && a < A) pred[(b * n_total + row_off + (long)a * S + s) * 3 + rem % 3] = p_sh[al][rem];
    }
    __syncthreads();                  // (the next tile overwrites both LDS tiles)
  }
  if (!owner) return;                 // inference: predictions only (uniform over the grid)

  // level 1: the block's four sums, lanes by xor shuffles and the waves in index order
  t_x = wave_sum(t_x);
  t_w = wave_sum(t_w);
  t_obj = wave_sum(t_obj);
  t_noobj = wave_sum(t_noobj);
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = t_x;
    red[1][tid >> 6] = t_w;
    red[2][tid >> 6] = t_obj;
    red[3][tid >> 6] = t_noobj;
  }
  __syncthreads();
  if (tid < 4) {
    float t = red[tid][0];
    for (int w = 1; w < kHeadThreads / WAVE; ++w) t += red[tid][w];
    __hip_atomic_store(&partials[(long)blockIdx.x * 4 + tid], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // the four write-through stores above are wave 0's: its agent-scope release drains them before its lane 0 takes the ticket
  if (tid < WAVE) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  if (tid == 0) {
    const unsigned ticket = atomicAdd(counter, 1u);
    last_sh = ticket == gridDim.x - 1;
  }
  __syncthreads();
  if (!last_sh) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");

  // level 2 (the last block to arrive): the blocks' rows in index order, in fp64
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (long j = tid; j < (long)gridDim.x; j += kHeadThreads)
#pragma unroll
    for (int q = 0; q < 4; ++q)
      acc[q] += (double)__hip_atomic_load(&partials[j * 4 + q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
  for (int q = 0; q < 4; ++q) fin[q][tid] = acc[q];
  __syncthreads();
  if (tid < 4) {
    double t = 0.0;
    for (int j = 0; j < kHeadThreads; ++j) t += fin[tid][j];
    const int n = counts[tid == 3 ? 1 : 0];
    fin[tid][0] = n > 0 ? t / (double)n : 0.0;
  }
  __syncthreads();
  if (tid == 0) {
    const double lx = fin[0][0], lw = fin[1][0], lo = fin[2][0], ln = fin[3][0];
    sums[0] = (float)lx;
    sums[1] = (float)lw;
    sums[2] = (float)lo;
    sums[3] = (float)ln;
    sums[4] = (float)(lx + lw + (double)obj_coeff * lo + (double)noobj_coeff * ln);
  }
}

// ------------------------------------------------------------------------------------------------ select
// float -> unsigned whose order is the float's (negative values below positive ones)
__device__ __forceinline__ uint32_t order_key(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// larger key = higher confidence, then SMALLER row.  Never 0 (that would need row 2^32 - 1): 0 marks "no candidate".
__device__ __forceinline__ uint64_t make_key(float conf, uint32_t row) {
  return ((uint64_t)order_key(conf) << 32) | (uint64_t)(0xFFFFFFFFu - row);
}

// descending bitonic sort of n (a power of two <= kChunk) keys in LDS by the whole block
__device__ __forceinline__ void sort_desc(uint64_t* keys, int n) {
  for (int size = 2; size <= n; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int t = threadIdx.x; t < (n >> 1); t += blockDim.x) {
        const int lo = 2 * t - (t & (stride - 1));
        const int hi = lo + stride;
        const bool desc = (lo & size) == 0;
        const uint64_t a = keys[lo], b = keys[hi];
        if ((a < b) == desc) {
          keys[lo] = b;
          keys[hi] = a;
        }
      }
    }
  }
  __syncthreads();
}

__device__ __forceinline__ int pow2_at_least(int n) {
  int p = 64;
  while (p < n) p <<= 1;
  return p;
}

// chunk c of video b: m candidates, either rows of pred (keys_in == nullptr) or keys of an earlier pass (0 = none)
__device__ __forceinline__ int load_chunk(uint64_t* keys, const float* __restrict__ pred, const uint64_t* __restrict__ keys_in,
                                          long b, long m, long c) {
  const long begin = c * kChunk;
  const int cn = (int)min((long)kChunk, m - begin);
  const int ns = pow2_at_least(cn);
  for (int t = threadIdx.x; t < ns; t += blockDim.x) {
    uint64_t kv = 0;
    if (t < cn) {
      const long j = begin + t;
      kv = keys_in ? keys_in[b * m + j] : make_key(pred[(b * m + j) * 3 + 2], (uint32_t)j);
    }
    keys[t] = kv;
  }
  return ns;
}

// grid (chunks, B): the k largest keys of a chunk, in order; k entries per chunk (0 behind the chunk's own)
__global__ __launch_bounds__(kSortThreads) void select_pass_kernel(const float* __restrict__ pred,
                                                                   const uint64_t* __restrict__ keys_in, long m, int k,
                                                                   uint64_t* __restrict__ keys_out) {
  __shared__ uint64_t keys[kChunk];
  const long b = blockIdx.y, c = blockIdx.x;
  const int ns = load_chunk(keys, pred, keys_in, b, m, c);
  sort_desc(keys, ns);
  uint64_t* out = keys_out + (b * gridDim.x + c) * k;
  for (int t = threadIdx.x; t < k; t += blockDim.x) out[t] = t < ns ? keys[t] : 0;
}

// grid (B): the last chunk -- sort, gather, corners, trim, greedy NMS, compaction
__global__ __launch_bounds__(kSortThreads) void select_final_kernel(const float* __restrict__ pred, long n,
                                                                    const uint64_t* __restrict__ keys_in, long m,
                                                                    const float* __restrict__ durations, int k, float nms_tiou,
                                                                    float* __restrict__ props, int* __restrict__ count) {
  __shared__ uint64_t keys[kChunk];
  __shared__ float st[BMHRL_PROPOSAL_MAX_K], en[BMHRL_PROPOSAL_MAX_K], cf[BMHRL_PROPOSAL_MAX_K];
  __shared__ int alive[BMHRL_PROPOSAL_MAX_K];
  const long b = blockIdx.x;
  const int tid = threadIdx.x;
  const int ns = load_chunk(keys, keys_in ? nullptr : pred, keys_in, b, keys_in ? m : n, 0);
  sort_desc(keys, ns);
  const float dur = durations[b];
  if (tid < k) {
    const uint64_t kv = tid < ns ? keys[tid] : 0;
    int ok = 0;
    float s = 0.f, e = 0.f, c = 0.f;
    if (kv != 0) {
      const long row = (long)(0xFFFFFFFFu - (uint32_t)kv);
      if (row < n) {                  // (always: keys only ever hold rows of this video)
        const float* p = pred + (b * n + row) * 3;
        const float centre = p[0], length = p[1];
        c = p[2];
        s = centre - length / 2.f;
        e = centre + length / 2.f;
        s = fminf(fmaxf(s, 0.f), dur);
        e = fminf(e, dur);
        ok = 1;
      }
    }
    st[tid] = s;
    en[tid] = e;
    cf[tid] = c;
    alive[tid] = ok;
  }
  __syncthreads();
  if (nms_tiou >= 0.f) {
    for (int i = 0; i < k - 1; ++i) {
      if (alive[i] && tid > i && tid < k && alive[tid]) {
        const float s1 = st[i], e1 = en[i], s2 = st[tid], e2 = en[tid];
        const float inter = fmaxf(fminf(e1, e2) - fmaxf(s1, s2), 0.f);
        float uni = (e1 - s1) + (e2 - s2) - inter;
        uni = fminf(fmaxf(e1, e2) - fminf(s1, s2), uni);
        const float t = inter / (uni + 1e-8f);
        if (!(t < nms_tiou)) alive[tid] = 0;
      }
      __syncthreads();
    }
  }
  if (tid < k) {
    int pos = 0, total = 0;
    for (int j = 0; j < k; ++j) {
      pos += (j < tid) & alive[j];
      total += alive[j];
    }
    float* out = props + (b * k) * 3;
    if (alive[tid]) {
      out[pos * 3 + 0] = st[tid];
      out[pos * 3 + 1] = en[tid];
      out[pos * 3 + 2] = cf[tid];
    }
    if (tid >= total) {               // rows behind the survivors
      out[tid * 3 + 0] = 0.f;
      out[tid * 3 + 1] = 0.f;
      out[tid * 3 + 2] = 0.f;
    }
    if (tid == 0) count[b] = total;
  }
}

inline long chunks_of(long m) { return (m + kChunk - 1) / kChunk; }

// ------------------------------------------------------------------------------------------------ soft select
// DESIGN.md section 35.  A pool of m <= 1024 rows per video; a pick is the arg-max of the CURRENT scores (ties to the
// smaller rank), and the rows that overlap the pick are retired (hard) or lose score (linear, Gaussian) instead.
constexpr int kSoftRows = BMHRL_PROPOSAL_SOFT_MAX_M / kSortThreads;      // pool rows a thread owns: tid and tid + 512

// the float whose order_key is the upper half of a key
__device__ __forceinline__ float key_score(uint64_t key) {
  const uint32_t u = (uint32_t)(key >> 32);
  return __uint_as_float((u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
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

// grid (B): the last chunk -- sort, gather the pool, corners, trim, then at most k picks.  A thread keeps the current scores
// of its (at most two) pool rows in registers; start / end / row of the whole pool are in LDS.  One barrier per pick: the
// eight wave maxima go to slot[pick & 1] and every thread reduces them itself, so a slot is written again only behind the
// barrier of the pick between, which no thread passes before it has read the slot.
__global__ __launch_bounds__(kSortThreads) void select_soft_kernel(const float* __restrict__ pred, long n,
                                                                   const uint64_t* __restrict__ keys_in, long mk,
                                                                   const float* __restrict__ durations, int m, int k, int method,
                                                                   float tiou_thresh, float sigma, float min_score,
                                                                   float* __restrict__ props, int* __restrict__ rows,
                                                                   int* __restrict__ count) {
  __shared__ uint64_t keys[kChunk];
  __shared__ float st[BMHRL_PROPOSAL_SOFT_MAX_M], en[BMHRL_PROPOSAL_SOFT_MAX_M];
  __shared__ int rw[BMHRL_PROPOSAL_SOFT_MAX_M];
  __shared__ uint64_t slot[2][kSortThreads / WAVE];
  const long b = blockIdx.x;
  const int tid = threadIdx.x;
  const int ns = load_chunk(keys, keys_in ? nullptr : pred, keys_in, b, keys_in ? mk : n, 0);
  sort_desc(keys, ns);
  const float dur = durations[b];
  float sc[kSoftRows];
  bool alive[kSoftRows];
#pragma unroll
  for (int r = 0; r < kSoftRows; ++r) {
    const int j = tid + r * kSortThreads;                   // the row's rank
    sc[r] = 0.f;
    alive[r] = false;
    if (j < m) {
      const uint64_t kv = j < ns ? keys[j] : 0;
      float s = 0.f, e = 0.f;
      int row = -1;
      if (kv != 0) {
        const long rr = (long)(0xFFFFFFFFu - (uint32_t)kv);
        if (rr < n) {                 // (always: keys only ever hold rows of this video)
          const float* p = pred + (b * n + rr) * 3;
          const float centre = p[0], length = p[1];
          sc[r] = p[2];
          s = centre - length / 2.f;
          e = centre + length / 2.f;
          s = fminf(fmaxf(s, 0.f), dur);
          e = fminf(e, dur);
          row = (int)rr;
          alive[r] = true;
        }
      }
      st[j] = s;
      en[j] = e;
      rw[j] = row;
    }
  }
  __syncthreads();
  float* out = props + (b * k) * 3;
  int* out_rows = rows ? rows + b * k : nullptr;
  int picked = 0;
  for (; picked < k; ++picked) {
    uint64_t best = 0;
#pragma unroll
    for (int r = 0; r < kSoftRows; ++r)
      if (alive[r]) {
        const uint64_t key = ((uint64_t)order_key(sc[r]) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)(tid + r * kSortThreads));
        best = key > best ? key : best;
      }
    best = wave_max_key(best);
    uint64_t* sl = slot[picked & 1];
    if ((tid & (WAVE - 1)) == 0) sl[tid / WAVE] = best;
    __syncthreads();
    best = sl[0];
#pragma unroll
    for (int w = 1; w < kSortThreads / WAVE; ++w) best = sl[w] > best ? sl[w] : best;
    if (best == 0) break;             // nothing alive (the same key in every thread: a uniform exit)
    const float score = key_score(best);
    if (score < min_score) break;
    const int pick = (int)(0xFFFFFFFFu - (uint32_t)best);
    const float s1 = st[pick], e1 = en[pick];
    if (tid == 0) {
      out[picked * 3 + 0] = s1;
      out[picked * 3 + 1] = e1;
      out[picked * 3 + 2] = score;
      if (out_rows) out_rows[picked] = rw[pick];
    }
#pragma unroll
    for (int r = 0; r < kSoftRows; ++r) {
      const int j = tid + r * kSortThreads;
      if (!alive[r]) continue;
      if (j == pick) {
        alive[r] = false;
        continue;
      }
      const float s2 = st[j], e2 = en[j];
      const float inter = fmaxf(fminf(e1, e2) - fmaxf(s1, s2), 0.f);
      float uni = (e1 - s1) + (e2 - s2) - inter;
      uni = fminf(fmaxf(e1, e2) - fminf(s1, s2), uni);
      const float t = inter / (uni + 1e-8f);
      if (!(t < tiou_thresh)) {
        if (method == BMHRL_NMS_HARD) {
          alive[r] = false;
        } else if (method == BMHRL_NMS_LINEAR) {
          sc[r] = sc[r] * (1.f - t);
        } else if (t != 0.f) {        // (t == 0, a disjoint row: exp(-0) is exactly 1 and the product the score's own bits)
          const float w32 = (float)exp(-((double)t * (double)t) / (double)sigma);
          sc[r] = sc[r] * w32;
        }
      }
    }
  }
  for (int j = picked + tid; j < k; j += kSortThreads) {    // behind the picks
    out[j * 3 + 0] = 0.f;
    out[j * 3 + 1] = 0.f;
    out[j * 3 + 2] = 0.f;
    if (out_rows) out_rows[j] = -1;
  }
  if (tid == 0) count[b] = picked;
}

}  // namespace

extern "C" int bmhrl_proposal_assign(const float* targets, int32_t n_targets, const float* anchors, int32_t A, float cell_sec,
                                     int32_t B, int32_t S, int32_t* owner, float* tx, float* tw, int32_t* counts,
                                     bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(anchors && owner && counts && n_targets >= 0 && A >= 1 && B >= 1 && S >= 1 && cell_sec > 0.f);
  BMHRL_CHECK_ARG(n_targets == 0 || (targets && tx && tw));
  BMHRL_CHECK_ARG((int64_t)B * A * S <= INT32_MAX);
  const long total = (long)B * A * S;
  hipLaunchKernelGGL(assign_clear_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, S_(stream), owner, total, counts);
  if (n_targets > 0)
    hipLaunchKernelGGL(assign_kernel, dim3((unsigned)((n_targets + 255) / 256)), dim3(256), 0, S_(stream), targets, n_targets,
                       anchors, A, cell_sec, B, S, owner, tx, tw, counts);
  return hip_status(hipGetLastError());
}

extern "C" int bmhrl_proposal_head(const float* x, const float* anchors, float cell_sec, int32_t B, int32_t S, int32_t A,
                                   float* pred, int64_t n_total, int64_t row_off, const int32_t* owner, const float* tx,
                                   const float* tw, const int32_t* counts, float obj_coeff, float noobj_coeff,
                                   const float* dscale, float* dx, float* sums, float* partials, uint32_t* counter,
                                   bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(x && anchors && pred && B >= 1 && S >= 1 && A >= 1 && cell_sec > 0.f);
  BMHRL_CHECK_ARG((int64_t)B * A * S <= INT32_MAX && row_off >= 0 && row_off + (int64_t)A * S <= n_total);
  if (owner)
    BMHRL_CHECK_ARG(counts && sums && partials && counter && ((uintptr_t)counter & 15) == 0);   // (tx / tw: read where a cell is owned)
  else
    BMHRL_CHECK_ARG(!dx);                                     // no targets: nothing to differentiate
  const int nts = (S + kTile - 1) / kTile, nta = (A + kTile - 1) / kTile;
  const long n_tiles = (long)B * nts * nta;
  const unsigned blocks = (unsigned)(n_tiles < kHeadMaxBlocks ? n_tiles : kHeadMaxBlocks);
  if (owner) {                        // the ticket word starts every call at zero (a memset node when the call is captured)
    const hipError_t e = hipMemsetAsync(counter, 0, 16, S_(stream));
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(head_kernel, dim3(blocks), dim3(kHeadThreads), 0, S_(stream), x, anchors, cell_sec, S, A, nts, nta, n_tiles,
                     pred, (long)n_total, (long)row_off, owner, tx, tw, counts, obj_coeff, noobj_coeff, dscale, dx, sums, partials,
                     counter);
  return hip_status(hipGetLastError());
}

extern "C" int bmhrl_proposal_select(const float* pred, int32_t B, int64_t N, const float* durations, int32_t k, float nms_tiou,
                                     float* props, int32_t* count, uint64_t* workspace, int64_t workspace_elems,
                                     bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(pred && durations && props && count && B >= 1 && B <= 65535);
  BMHRL_CHECK_ARG(k >= 1 && k <= BMHRL_PROPOSAL_MAX_K && N >= 1 && N <= BMHRL_PROPOSAL_MAX_N);
  BMHRL_CHECK_ARG(nms_tiou == nms_tiou);
  // the passes: m candidates -> chunks_of(m) * k, until one chunk is left; buffers alternate between the two halves
  long need0 = 0, need1 = 0;
  {
    long m = N;
    for (int pass = 0; m > kChunk; ++pass) {
      const long out = chunks_of(m) * k;
      if (pass & 1) need1 = need1 > out ? need1 : out; else need0 = need0 > out ? need0 : out;
      m = out;
    }
  }
  BMHRL_CHECK_ARG(need0 == 0 || (workspace && workspace_elems >= (int64_t)B * (need0 + need1)));
  uint64_t* buf[2] = {workspace, workspace ? workspace + (long)B * need0 : nullptr};
  const uint64_t* keys_in = nullptr;
  long m = N;
  for (int pass = 0; m > kChunk; ++pass) {
    const long nc = chunks_of(m);
    hipLaunchKernelGGL(select_pass_kernel, dim3((unsigned)nc, (unsigned)B), dim3(kSortThreads), 0, S_(stream), pred, keys_in, m, k,
                       buf[pass & 1]);
    keys_in = buf[pass & 1];
    m = nc * k;
  }
  hipLaunchKernelGGL(select_final_kernel, dim3((unsigned)B), dim3(kSortThreads), 0, S_(stream), pred, (long)N, keys_in, m, durations,
                     k, nms_tiou, props, count);
  return hip_status(hipGetLastError());
}

extern "C" int bmhrl_proposal_select_soft(const float* pred, int32_t B, int64_t N, const float* durations, int32_t m, int32_t k,
                                          int32_t method, float tiou_thresh, float sigma, float min_score, float* props,
                                          int32_t* rows, int32_t* count, uint64_t* workspace, int64_t workspace_elems,
                                          bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(pred && durations && props && count && B >= 1 && B <= 65535);
  BMHRL_CHECK_ARG(N >= 1 && N <= BMHRL_PROPOSAL_MAX_N && m >= 1 && m <= BMHRL_PROPOSAL_SOFT_MAX_M && k >= 1 && k <= m);
  BMHRL_CHECK_ARG(method == BMHRL_NMS_HARD || method == BMHRL_NMS_LINEAR || method == BMHRL_NMS_GAUSSIAN);
  BMHRL_CHECK_ARG(tiou_thresh == tiou_thresh && min_score == min_score && (method != BMHRL_NMS_GAUSSIAN || sigma > 0.f));
  // stage one is bmhrl_proposal_select's, keeping m keys per chunk: chunks_of(c) * m candidates per pass until one chunk is left
  long need0 = 0, need1 = 0;
  {
    long c = N;
    for (int pass = 0; c > kChunk; ++pass) {
      const long out = chunks_of(c) * m;
      if (pass & 1) need1 = need1 > out ? need1 : out; else need0 = need0 > out ? need0 : out;
      c = out;
    }
  }
  BMHRL_CHECK_ARG(need0 == 0 || (workspace && workspace_elems >= (int64_t)B * (need0 + need1)));
  uint64_t* buf[2] = {workspace, workspace ? workspace + (long)B * need0 : nullptr};
  const uint64_t* keys_in = nullptr;
  long c = N;
  for (int pass = 0; c > kChunk; ++pass) {
    const long nc = chunks_of(c);
    hipLaunchKernelGGL(select_pass_kernel, dim3((unsigned)nc, (unsigned)B), dim3(kSortThreads), 0, S_(stream), pred, keys_in, c, m,
                       buf[pass & 1]);
    keys_in = buf[pass & 1];
    c = nc * m;
  }
  hipLaunchKernelGGL(select_soft_kernel, dim3((unsigned)B), dim3(kSortThreads), 0, S_(stream), pred, (long)N, keys_in, c, durations,
                     m, k, method, tiou_thresh, sigma, min_score, props, rows, count);
  return hip_status(hipGetLastError());
}
