// Segment crop for gfx950: cuts and pads the feature rows of P temporal segments out of the full-length
// stacks of V videos that are resident on the device -- what the loader does on the host, clip by clip, from the feature
// files (captioning_datasets/load_features.py:14-35 `crop_a_segment`, then the padding of a batch).  One ordinary launch on
// the caller's stream per feature stack, no host read.
//
//   bounds   per segment, in IEEE float64 and term for term as bmhrl_amd/loader.py crop_bounds: a = trunc(S * (start /
//            duration)), b likewise (the quotient first), the a == b step, then Python's slice(a, b).indices(S).  Computed by
//            one thread per (segment, row tile) and handed to the block through LDS.
//   copy     a pure copy: a (segment, row tile) pair is a contiguous run of the output and, for its copied rows, a contiguous
//            run of the source; every output element is stored exactly once, 16 bytes per lane where D % 4 == 0 and both
//            bases are 16-byte aligned, 4 bytes per lane otherwise.
//   status   two integer counters, zeroed by a one-wave launch in front, bumped by the thread that owns a segment's first tile.
//
// The division must be IEEE and nothing may be contracted:
#pragma clang fp contract(off)
#include <cfloat>
#include <climits>
#include <cmath>
#include "common.h"
#include "../../include/bmhrl_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;      // memory-bound: a bounded grid strides over the tiles
constexpr int kTileFloats = 4096;     // 16 KiB of output per tile (rows per tile = max(1, kTileFloats / D))

#define S_(s) ((hipStream_t)(s))

// trunc(S * q) as Python's int(), limited to the int32 range (no change to the slice below while S <= 2^24); false when
// Python would raise (a non-finite product)
__device__ __forceinline__ bool trunc_index(double S, double q, long* out) {
  const double x = S * q;
  if (!(fabs(x) <= DBL_MAX)) return false;
  *out = (long)fmin(fmax(trunc(x), (double)INT_MIN), (double)INT_MAX);
  return true;
}

// Python's clamp of one end of slice(a, b) with step 1 over S rows
__device__ __forceinline__ long slice_end(long i, long S) {
  if (i < 0) {
    i += S;
    return i < 0 ? 0 : i;
  }
  return i > S ? S : i;
}

// (lo, n) of segment p; *invalid is set where the segment has no defined crop (n = 0 then)
__device__ __forceinline__ void segment_bounds(const int* __restrict__ src_len, const double* __restrict__ durations, int V,
                                               int S_pad, const int* __restrict__ seg_video,
                                               const double* __restrict__ seg_times, long p, int* v_out, int* lo_out, int* n_out,
                                               int* invalid) {
  *v_out = 0;
  *lo_out = 0;
  *n_out = 0;
  *invalid = 1;
  const int v = seg_video[p];
  if (v < 0 || v >= V) return;
  const int S = src_len[v];
  if (S < 0 || S > S_pad) return;      // rows past the stack are never read
  const double duration = durations[v], start = seg_times[2 * p], end = seg_times[2 * p + 1];
  if (!(duration > 0.0)) return;
  const double qa = start / duration, qb = end / duration;
  if (!(fabs(qa) <= DBL_MAX) || !(fabs(qb) <= DBL_MAX)) return;
  long a, b;
  if (!trunc_index((double)S, qa, &a) || !trunc_index((double)S, qb, &b)) return;
  *invalid = 0;
  if (a == b) {
    if (a == S)
      a -= 1;
    else
      b += 1;
  }
  const long lo = slice_end(a, S), hi = slice_end(b, S);
  if (hi > lo) {
    *v_out = v;
    *lo_out = (int)lo;
    *n_out = (int)(hi - lo);
  }
}

// The counters start every call at zero.  A one-wave launch, not a memset: captured in a graph, the 8-byte memset node was
// seen to leave the bytes 0x01 in both words on replay; a kernel node in front of the crop is ordered
// like any other.
__global__ __launch_bounds__(WAVE) void status_clear_kernel(int* __restrict__ status) {
  if (threadIdx.x < 2) status[threadIdx.x] = 0;
}

template <typename T>
__device__ __forceinline__ T splat(float x);
template <>
__device__ __forceinline__ float splat<float>(float x) { return x; }
template <>
__device__ __forceinline__ f32x4 splat<f32x4>(float x) { return f32x4{x, x, x, x}; }

// T = f32x4: Du = D / 4 units of 16 bytes per row; T = float: Du = D.  A tile is `rows` rows of one segment: rows * Du
// consecutive units of out, of which the first `copy` come from consecutive units of src.
template <typename T>
__global__ __launch_bounds__(kThreads) void crop_kernel(const T* __restrict__ src, const int* __restrict__ src_len,
                                                        const double* __restrict__ durations, int V, int S_pad, int Du,
                                                        const int* __restrict__ seg_video, const double* __restrict__ seg_times,
                                                        long P, float pad_value, int T_out, int rows, int tiles, T* __restrict__ out,
                                                        int* __restrict__ lengths, int* __restrict__ lo_out,
                                                        int* __restrict__ status) {
  __shared__ int sh[3];               // video, lo, n of the tile's segment
  const T pad = splat<T>(pad_value), zero = splat<T>(0.f);
  const long n_work = P * tiles;
  for (long w = blockIdx.x; w < n_work; w += gridDim.x) {
    const long p = w / tiles;
    const int tile = (int)(w % tiles);
    if (threadIdx.x == 0) {
      int v, lo, n, invalid;
      segment_bounds(src_len, durations, V, S_pad, seg_video, seg_times, p, &v, &lo, &n, &invalid);
      sh[0] = v;
      sh[1] = lo;
      sh[2] = n;
      if (tile == 0) {                // this thread owns the segment's scalars
        lengths[p] = n;
        if (lo_out) lo_out[p] = lo;
        if (n > T_out) atomicAdd(&status[0], 1);
        if (invalid) atomicAdd(&status[1], 1);
      }
    }
    __syncthreads();
    const int v = sh[0], lo = sh[1], n = sh[2];
    const int r0 = tile * rows;
    const int r1 = min(r0 + rows, T_out);                       // the tile's rows [r0, r1) of out[p]
    const int rc = min(max(min(n, T_out) - r0, 0), r1 - r0);    // of which copied
    const long units = (long)(r1 - r0) * Du, copy = (long)rc * Du;
    const long zeros = (n == 0 && tile == 0) ? Du : 0;          // an empty crop: one row of zeros, then padding
    const T* s = src + ((long)v * S_pad + lo + r0) * Du;        // (only units below `copy` are read)
    T* o = out + (p * T_out + r0) * Du;
    for (long e = threadIdx.x; e < units; e += kThreads) o[e] = e < copy ? s[e] : (e < zeros ? zero : pad);
    __syncthreads();                  // (the next tile overwrites sh)
  }
}

}  // namespace

extern "C" int bmhrl_crop_segments(const float* src, const int32_t* src_len, const double* durations, int32_t V, int32_t S_pad,
                                   int32_t D, const int32_t* seg_video, const double* seg_times, int32_t P, float pad_value,
                                   int32_t T_out, float* out, int32_t* lengths, int32_t* lo, int32_t* status,
                                   bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(src && src_len && durations && seg_video && seg_times && out && lengths && status);
  BMHRL_CHECK_ARG(V >= 1 && P >= 1 && D >= 1 && T_out >= 1 && S_pad >= 1);
  hipLaunchKernelGGL(status_clear_kernel, dim3(1), dim3(WAVE), 0, S_(stream), status);
  const bool wide = D % 4 == 0 && (((uintptr_t)src | (uintptr_t)out) & 15) == 0;
  const int rows = D >= kTileFloats ? 1 : kTileFloats / D;
  const int tiles = (T_out + rows - 1) / rows;
  const long n_work = (long)P * tiles;
  const unsigned blocks = (unsigned)(n_work < kMaxBlocks ? n_work : kMaxBlocks);
  if (wide)
    hipLaunchKernelGGL(crop_kernel<f32x4>, dim3(blocks), dim3(kThreads), 0, S_(stream), (const f32x4*)src, src_len, durations, V,
                       S_pad, D / 4, seg_video, seg_times, (long)P, pad_value, T_out, rows, tiles, (f32x4*)out, lengths, lo,
                       status);
  else
    hipLaunchKernelGGL(crop_kernel<float>, dim3(blocks), dim3(kThreads), 0, S_(stream), src, src_len, durations, V, S_pad, D,
                       seg_video, seg_times, (long)P, pad_value, T_out, rows, tiles, out, lengths, lo, status);
  return hip_status(hipGetLastError());
}
