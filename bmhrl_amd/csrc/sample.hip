// Sampled caption decoding (bmhrl_amd/decode.py SampleDecoder): one step of the sampling rules for every row -- temperature,
// top-k / top-p truncation over the order (log-prob descending, ties to the smaller token id), one counter-RNG draw over the
// kept tokens in token-id order.  The step position t is a device word, so the launch sits inside the captured token step.
//
// One 512-thread workgroup per row (two waves per SIMD: up to 256 VGPRs; 1024 threads measured 1.4x slower with the select);
// lane i holds the NV contiguous tokens [i*NV, i*NV + NV) in registers, so every prefix in token-id order is a lane-local
// running sum plus one block exclusive scan of the lane totals.  Every reduction is a fixed
// tree (wave64 xor / up shuffles, then the 8 wave partials summed in wave order from LDS): no atomics, the same input and seed
// give bit-identical outputs.
//
// The truncation is a radix select on the order-preserving uint32 key of lp, 8 passes of 4-bit digits from the top.  A pass
// counts, for the tokens whose key matches the digits chosen so far, (count, q-mass) per digit (see digit_totals), reduced
// across the wave by a reduce-scatter butterfly (17 shuffles instead of 16 x 6) and across the 8 waves from LDS; wave 0
// walks the digits (a suffix scan and a ballot) and broadcasts its decision through LDS.
// Walking the digits from 15 down, the chosen digit is the first whose inclusive (count, mass) reaches the remaining k or the
// remaining p * sum(q): one pass structure serves top-k, top-p and both (the cut of "both" is the shorter prefix).  A digit
// holding a single token ends the select early.  After the last pass the cut key is exact; a block prefix count of that key
// in token-id order settles the ties.  Fast paths: arg-max for T = 0 / k = 1 / rows without a finite entry, no select at
// all for k = 0 and p = 1.
#include <climits>
#include "common.h"
#include "../../include/bmhrl_hip.h"

#define S_(x) ((hipStream_t)(x))

namespace {

constexpr int kThreads = 512;
constexpr int kWaves = kThreads / WAVE;
constexpr int kDigits = 16;                 // 4-bit digits, 8 passes over the 32-bit key

struct SampleSmem {
  float hist[kDigits][kThreads];            // per-lane q mass per digit (private columns)
  float red[kWaves][2 * kDigits];           // per-wave (count, mass) per digit
  int dec_d, dec_reached;                   // the digit walk's decision: digit, reached; its count, count / mass before
  float dec_f[3];
  float fw[kWaves];                         // per-wave float partials (max, sums, scans)
  int iw[kWaves][2];                        // per-wave int partials (scans, arg reductions)
  unsigned kw[kWaves];
};

// larger lp -> larger key; -0 was folded into +0 and NaN into -inf by the caller
__device__ __forceinline__ unsigned order_key(float x) {
  const unsigned b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ float q_of(float x, float M, float temperature) { return expf((x - M) / temperature); }

// inclusive wave scan (fixed order), then the exclusive block offset of this lane; *total: the block sum
__device__ __forceinline__ float block_excl_scan(float v, SampleSmem& sm, float* total) {
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  float x = v;
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) {
    const float y = __shfl_up(x, o, WAVE);
    if (lane >= o) x += y;
  }
  float ex = __shfl_up(x, 1, WAVE);
  if (lane == 0) ex = 0.f;
  __syncthreads();
  if (lane == WAVE - 1) sm.fw[wave] = x;
  __syncthreads();
  float off = 0.f, all = 0.f;
#pragma unroll
  for (int w = 0; w < kWaves; ++w) {
    if (w < wave) off += sm.fw[w];
    all += sm.fw[w];
  }
  *total = all;
  return off + ex;
}

__device__ __forceinline__ int block_excl_scan_int(int v, SampleSmem& sm) {
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
  int x = v;
#pragma unroll
  for (int o = 1; o < WAVE; o <<= 1) {
    const int y = __shfl_up(x, o, WAVE);
    if (lane >= o) x += y;
  }
  __syncthreads();
  if (lane == WAVE - 1) sm.iw[wave][0] = x;
  __syncthreads();
  int off = 0;
#pragma unroll
  for (int w = 0; w < kWaves; ++w)
    if (w < wave) off += sm.iw[w][0];
  return off + x - v;
}

// block (value, id) arg-max, ties to the smaller id; every thread gets the winner's id
__device__ __forceinline__ int block_argmax(float v, int i, SampleSmem& sm) {
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) {
    const float v2 = __shfl_xor(v, o, WAVE);
    const int i2 = __shfl_xor(i, o, WAVE);
    if (beats(v2, i2, v, i)) { v = v2; i = i2; }
  }
  __syncthreads();
  if (lane == 0) { sm.fw[wave] = v; sm.iw[wave][0] = i; }
  __syncthreads();
  v = sm.fw[0];
  i = sm.iw[0][0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w)
    if (beats(sm.fw[w], sm.iw[w][0], v, i)) { v = sm.fw[w]; i = sm.iw[w][0]; }
  return i;
}

// block (min, max) of two ints
__device__ __forceinline__ void block_min_max(int& mn, int& mx, SampleSmem& sm) {
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) {
    mn = min(mn, __shfl_xor(mn, o, WAVE));
    mx = max(mx, __shfl_xor(mx, o, WAVE));
  }
  __syncthreads();
  if (lane == 0) { sm.iw[wave][0] = mn; sm.iw[wave][1] = mx; }
  __syncthreads();
  mn = sm.iw[0][0];
  mx = sm.iw[0][1];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) { mn = min(mn, sm.iw[w][0]); mx = max(mx, sm.iw[w][1]); }
}

__device__ __forceinline__ unsigned block_max_u32(unsigned v, SampleSmem& sm) {
  const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
#pragma unroll
  for (int o = WAVE / 2; o > 0; o >>= 1) v = max(v, (unsigned)__shfl_xor((int)v, o, WAVE));
  __syncthreads();
  if (lane == 0) sm.kw[wave] = v;
  __syncthreads();
  v = sm.kw[0];
#pragma unroll
  for (int w = 1; w < kWaves; ++w) v = max(v, sm.kw[w]);
  return v;
}

// 16 values per lane -> lane l holds the wave total of value l >> 2 (reduce-scatter: halves exchanged at offsets 32..4,
// then plain xor-2 / xor-1 adds): 17 shuffles instead of 16 x 6
__device__ __forceinline__ float wave_reduce_scatter16(float (&v)[kDigits]) {
  const int lane = threadIdx.x & (WAVE - 1);
#pragma unroll
  for (int h = kDigits / 2, o = 32; h >= 1; h >>= 1, o >>= 1) {
    const bool up = (lane & o) != 0;
#pragma unroll
    for (int i = 0; i < h; ++i) {
      const float keep = up ? v[h + i] : v[i];
      const float give = up ? v[i] : v[h + i];
      v[i] = keep + __shfl_xor(give, o, WAVE);
    }
  }
  float r = v[0] + __shfl_xor(v[0], 2, WAVE);
  return r + __shfl_xor(r, 1, WAVE);
}

// per-digit totals of the tokens whose key matches prefix under mask: counts (what 0) or q mass (what 1), written as the
// wave's partials to sm.red[wave][what * 16 + d].  Counts: one byte per digit in two packed 64-bit words per lane.  Mass: a
// private 16-bin column of sm.hist per lane (row stride 512 floats: every access of a wave hits 64 distinct banks whatever
// the digits), summed in token order.  Compares of every token against every digit would need 16 * NV lane masks.
template <int NV>
__device__ __forceinline__ void digit_totals(const float (&x)[NV], const float (&q)[NV], int v0, int V, unsigned prefix,
                                             unsigned mask, int shift, int what, SampleSmem& sm) {
  const int tid = threadIdx.x;
  float acc[kDigits];
  if (what == 0) {
    uint64_t lo = 0, hi = 0;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const unsigned key = order_key(x[j]);
      const bool in = v0 + j < V && (key & mask) == prefix;
      const unsigned dg = (key >> shift) & (kDigits - 1);
      const uint64_t one = in ? (1ull << (8 * (dg & 7))) : 0ull;
      lo += dg < 8 ? one : 0ull;
      hi += dg < 8 ? 0ull : one;
    }
#pragma unroll
    for (int d = 0; d < kDigits; ++d) acc[d] = (float)(((d < 8 ? lo : hi) >> (8 * (d & 7))) & 0xffu);
  } else {
#pragma unroll
    for (int d = 0; d < kDigits; ++d) sm.hist[d][tid] = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const unsigned key = order_key(x[j]);
      if (v0 + j < V && (key & mask) == prefix) sm.hist[(key >> shift) & (kDigits - 1)][tid] += q[j];
    }
#pragma unroll
    for (int d = 0; d < kDigits; ++d) acc[d] = sm.hist[d][tid];
  }
  const float part = wave_reduce_scatter16(acc);
  const int lane = tid & (WAVE - 1), wave = tid / WAVE;
  if ((lane & 3) == 0) sm.red[wave][what * kDigits + (lane >> 2)] = part;
}

template <int NV>
__global__ __launch_bounds__(kThreads) void sample_step_kernel(
    const float* __restrict__ logp, long ld, int V, float temperature, int top_k, float top_p, uint64_t seed,
    const uint64_t* __restrict__ seed_dev, const int64_t* __restrict__ tdev, long row_offset, int end_idx, int pad_idx,
    uint8_t* __restrict__ finished, int64_t* __restrict__ tok, int64_t* __restrict__ out, long ld_out,
    float* __restrict__ sum_logp, float* __restrict__ step_logp, float* __restrict__ step_logq) {
  __shared__ SampleSmem sm;
  const int row = blockIdx.x, tid = threadIdx.x;
  const long t = tdev[0];
  const bool hist = t >= 0 && t + 1 < ld_out;
  const long hcol = (long)row * ld_out + t;
  if (finished[row]) {                      // (uniform over the block)
    if (tid == 0) {
      tok[row] = pad_idx;
      if (hist) {
        out[hcol + 1] = pad_idx;
        if (step_logp) step_logp[hcol] = 0.f;
        if (step_logq) step_logq[hcol] = 0.f;
      }
    }
    return;
  }
  const float* lp = logp + (long)row * ld;
  const int v0 = tid * NV;
  float x[NV];
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    float a = v0 + j < V ? lp[v0 + j] : -INFINITY;
    a = a != a ? -INFINITY : a + 0.f;       // NaN ranks as -inf; -0 + 0 = +0 (one key per value)
    x[j] = a;
  }

  float mx = -INFINITY;
#pragma unroll
  for (int j = 0; j < NV; ++j) mx = fmaxf(mx, x[j]);
  const float M = block_max(mx, sm.fw);

  int pick;
  float logq;
  if (temperature == 0.f || top_k == 1 || M == -INFINITY) {
    float bv = -INFINITY;
    int bi = INT_MAX;
#pragma unroll
    for (int j = 0; j < NV; ++j)
      if (v0 + j < V && beats(x[j], v0 + j, bv, bi)) { bv = x[j]; bi = v0 + j; }
    pick = block_argmax(bv, bi, sm);
    logq = 0.f;
  } else {
    float q[NV];
    float qs = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      q[j] = v0 + j < V ? q_of(x[j], M, temperature) : 0.f;
      qs += q[j];
    }
    const bool by_k = top_k > 0 && top_k < V;
    const bool by_p = top_p < 1.f;
    bool kept[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) kept[j] = v0 + j < V;
    if (by_k || by_p) {
      float S = 0.f;
      block_excl_scan(qs, sm, &S);
      // remaining count / mass before the cut, the key prefix chosen so far and its mask
      float k_rem = by_k ? (float)top_k : INFINITY;
      float m_rem = by_p ? top_p * S : INFINITY;
      unsigned prefix = 0u, mask = 0u;
      unsigned cut_key = 0u;
      float cut_count = 0.f;
      bool single = false;
#pragma unroll 1
      for (int shift = 28; shift >= 0; shift -= 4) {
        digit_totals<NV>(x, q, v0, V, prefix, mask, shift, 0, sm);
        if (by_p) digit_totals<NV>(x, q, v0, V, prefix, mask, shift, 1, sm);
        __syncthreads();
        if (tid < WAVE) {
          // wave 0: lane d < 16 holds digit d's totals; suffix sums from the top digit down, then the highest digit whose
          // inclusive (count, mass) reaches (k_rem, m_rem) -- or, when rounding left the mass short, the lowest
          // non-empty digit
          float c = 0.f, m = 0.f;
          if (tid < kDigits) {
#pragma unroll
            for (int w = 0; w < kWaves; ++w) {
              c += sm.red[w][tid];
              if (by_p) m += sm.red[w][kDigits + tid];
            }
          }
          float ci = c, mi = m;
#pragma unroll
          for (int o = 1; o < kDigits; o <<= 1) {
            const float c2 = __shfl_down(ci, o, WAVE), m2 = __shfl_down(mi, o, WAVE);
            if (tid + o < kDigits) { ci += c2; mi += m2; }
          }
          float ce = __shfl_down(ci, 1, WAVE), me = __shfl_down(mi, 1, WAVE);
          if (tid + 1 >= kDigits) { ce = 0.f; me = 0.f; }
          const uint64_t hit = __ballot(tid < kDigits && c != 0.f && (ci >= k_rem || mi >= m_rem));
          const uint64_t some = __ballot(tid < kDigits && c != 0.f);
          const int chosen = hit ? 63 - __builtin_clzll(hit) : (some ? __builtin_ctzll(some) : -1);
          if (tid == (chosen < 0 ? 0 : chosen)) {
            sm.dec_d = chosen;
            sm.dec_reached = hit != 0;
            sm.dec_f[0] = c;
            sm.dec_f[1] = ce;
            sm.dec_f[2] = me;
          }
        }
        __syncthreads();
        const int chosen = sm.dec_d;
        const bool reached = sm.dec_reached;
        const float c_here = sm.dec_f[0], c_before = sm.dec_f[1], m_before = sm.dec_f[2];
        if (chosen < 0) break;                                 // (no token matched: cannot happen)
        k_rem -= c_before;
        m_rem -= m_before;
        if (!reached) {                    // rounding left the mass short: the cut is the last token of the lowest digit
          k_rem = c_here;
          m_rem = INFINITY;
        }
        prefix |= (unsigned)chosen << shift;
        mask |= (unsigned)(kDigits - 1) << shift;
        cut_count = c_here;
        if (c_here == 1.f) { single = true; break; }
      }
      if (single) {
        unsigned km = 0u;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
          const unsigned key = order_key(x[j]);
          if (v0 + j < V && (key & mask) == prefix) km = max(km, key);
        }
        cut_key = block_max_u32(km, sm);
#pragma unroll
        for (int j = 0; j < NV; ++j) kept[j] = kept[j] && order_key(x[j]) >= cut_key;
      } else {
        cut_key = prefix;
        // ties at the cut key: the first n_cut of them in token-id order
        const float q_cut = expf((__uint_as_float((cut_key & 0x80000000u) ? (cut_key & 0x7fffffffu) : ~cut_key) - M) / temperature);
        float n_cut = fminf(k_rem, cut_count);
        if (by_p && m_rem < INFINITY) n_cut = fminf(n_cut, q_cut > 0.f ? ceilf(m_rem / q_cut) : cut_count);
        n_cut = fmaxf(n_cut, 1.f);
        int ties = 0;
#pragma unroll
        for (int j = 0; j < NV; ++j) ties += (v0 + j < V && order_key(x[j]) == cut_key) ? 1 : 0;
        int rank = block_excl_scan_int(ties, sm);
#pragma unroll
        for (int j = 0; j < NV; ++j) {
          const unsigned key = order_key(x[j]);
          bool k_ = v0 + j < V && key > cut_key;
          if (v0 + j < V && key == cut_key) k_ = (float)(rank++) < n_cut;
          kept[j] = k_;
        }
      }
    }
    // the draw: kept q in token-id order, the first positive-q token whose inclusive sum exceeds u * kept_mass
    float lsum = 0.f;
#pragma unroll
    for (int j = 0; j < NV; ++j) lsum += kept[j] ? q[j] : 0.f;
    float kept_mass = 0.f;
    const float off = block_excl_scan(lsum, sm, &kept_mass);
    const uint64_t s = seed + (seed_dev ? seed_dev[0] : 0ull);
    const float thr = uniform01(s, ((uint64_t)(row_offset + row) << 16) + (uint64_t)t) * kept_mass;
    int first = INT_MAX, last = -1;
    float run = off;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
      const bool cand = kept[j] && q[j] > 0.f;
      run += kept[j] ? q[j] : 0.f;
      if (cand) {
        last = v0 + j;
        if (run > thr && first == INT_MAX) first = v0 + j;
      }
    }
    block_min_max(first, last, sm);
    pick = first != INT_MAX ? first : last;
    logq = (lp[pick] - M) / temperature - logf(kept_mass);
  }
  if (tid == 0) {
    const float lv = lp[pick];
    sum_logp[row] += lv;
    tok[row] = pick;
    if (pick == end_idx) finished[row] = 1;
    if (hist) {
      out[hcol + 1] = pick;
      if (step_logp) step_logp[hcol] = lv;
      if (step_logq) step_logq[hcol] = logq;
    }
  }
}

}  // namespace

extern "C" int bmhrl_sample_step(const float* logp, int64_t ld, int32_t rows, int32_t V, float temperature, int32_t top_k,
                                 float top_p, uint64_t seed, const uint64_t* seed_dev, const int64_t* t, int64_t row_offset,
                                 int32_t end_idx, int32_t pad_idx, uint8_t* finished, int64_t* tok, int64_t* out, int64_t ld_out,
                                 float* sum_logp, float* step_logp, float* step_logq, bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(logp && t && finished && tok && out && sum_logp);
  BMHRL_CHECK_ARG(rows > 0 && V >= 1 && V <= BMHRL_SAMPLE_MAX_V && ld >= V && ld_out >= 1 && row_offset >= 0);
  BMHRL_CHECK_ARG(temperature >= 0.f && temperature < INFINITY && top_k >= 0 && top_p > 0.f && top_p <= 1.f);
  BMHRL_CHECK_ARG(pad_idx >= 0 && pad_idx < V);
  const int nv = (V + kThreads - 1) / kThreads;
#define LAUNCH(NV_)                                                                                                        \
  hipLaunchKernelGGL(sample_step_kernel<NV_>, dim3((unsigned)rows), dim3(kThreads), 0, S_(stream), logp, (long)ld, V,       \
                     temperature, top_k, top_p, seed, seed_dev, t, (long)row_offset, end_idx, pad_idx, finished, tok, out,    \
                     (long)ld_out, sum_logp, step_logp, step_logq)
  if (nv <= 2) LAUNCH(2);
  else if (nv <= 4) LAUNCH(4);
  else if (nv <= 8) LAUNCH(8);
  else if (nv <= 16) LAUNCH(16);
  else if (nv <= 20) LAUNCH(20);
  else if (nv <= 24) LAUNCH(24);
  else LAUNCH(32);
#undef LAUNCH
  return hip_status(hipGetLastError());
}
