// Global L2 norm of the trainer's gradient and the clip coefficient from it (train.FlatAdam.clip): two launches.
//
// grad_sq_partials_kernel walks the per-parameter table of bmhrl_adam_segments (7 int64 per parameter; word 6 names the
// gradient where autograd left it, 0 = the flat bucket at the parameter's offset).  One 256-thread block owns 4096
// consecutive elements of one parameter, as in the Adam pass.  The sum of squares of g * grad_scale is taken in ONE fixed
// order, whatever the scheduling:
//   thread:  elements base + tid + 256 k, k = 0..15, added in k order (the scalar path), or -- a whole block whose gradient
//            is 16-byte aligned -- four 16-byte loads, all requested before the first use, elements base + 4 tid + 1024 it + j
//            added in (it, j) order: 16 additions either way
//   wave:    six xor-shuffle levels (32, 16, 8, 4, 2, 1)
//   block:   the four wave sums added in wave order by thread 0 -> partials[block], fp32
// grad_norm_finish_kernel (one block) adds the partials in fp64: thread t takes the contiguous run t of the block indices in
// index order, thread 0 adds the 256 run sums in run order.  No floating-point atomic and no arrival order anywhere, so the
// two words it writes are the same bits in every run, with and without BMHRL_DETERMINISTIC.
#include "common.h"
#include "../../include/bmhrl_hip.h"

#define S_(x) ((hipStream_t)(x))

namespace {

constexpr int kWords = 7;            // table row of bmhrl_adam_segments
constexpr int kBlockElems = 4096;
constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void grad_sq_partials_kernel(const int64_t* __restrict__ seg, int n_seg,
                                                                    const float* __restrict__ g, float gscale,
                                                                    float* __restrict__ partials) {
  int lo = 0, hi = n_seg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (seg[mid * kWords + 5] <= (int64_t)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const int64_t* e = seg + lo * kWords;
  const long total = e[2] * e[3];
  const long base = ((long)blockIdx.x - e[5]) * kBlockElems;
  const long end = base + kBlockElems < total ? base + kBlockElems : total;
  const float* __restrict__ gp = e[6] ? reinterpret_cast<const float*>(e[6]) : g + e[0];
  float s = 0.f;
  if (end - base == kBlockElems && (reinterpret_cast<uintptr_t>(gp) & 15) == 0) {
    f32x4 gv[4];
#pragma unroll
    for (int it = 0; it < 4; ++it)
      gv[it] = *reinterpret_cast<const f32x4*>(gp + base + 4 * threadIdx.x + it * (kBlockElems / 4));
#pragma unroll
    for (int it = 0; it < 4; ++it)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float x = gv[it][j] * gscale;
        s += x * x;
      }
  } else {
    for (long i = base + threadIdx.x; i < end; i += kThreads) {
      const float x = gp[i] * gscale;
      s += x * x;
    }
  }
  s = wave_sum(s);
  __shared__ float red[kThreads / WAVE];
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(kThreads) void grad_norm_finish_kernel(const float* __restrict__ partials, int n,
                                                                    float* __restrict__ hyper) {
  __shared__ double runs[kThreads];
  const int per = (n + kThreads - 1) / kThreads;
  const int first = threadIdx.x * per, last = first + per < n ? first + per : n;
  double a = 0.0;
  for (int i = first; i < last; ++i) a += (double)partials[i];
  runs[threadIdx.x] = a;
  __syncthreads();
  if (threadIdx.x != 0) return;
  double sum = 0.0;
  for (int t = 0; t < kThreads; ++t) sum += runs[t];
  const float norm = (float)sqrt(sum);
  // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max = 1), where torch forms scalar / tensor as
  // reciprocal(tensor) * scalar.  A norm that is not finite gives NaN: the update that follows is visibly poisoned instead
  // of quietly scaled to zero.
  const float coef = isfinite(norm) ? fminf((1.0f / (norm + 1e-6f)) * hyper[1], 1.0f) : __builtin_nanf("");
  hyper[2] = coef;
  hyper[3] = norm;
}

}  // namespace

extern "C" int bmhrl_grad_norm(const int64_t* segments, int32_t n_segments, int32_t n_blocks, const float* grad, float grad_scale,
                               float* partials, int64_t partials_elems, float* hyper, bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(segments && n_segments > 0 && n_blocks > 0 && grad && partials && hyper);
  BMHRL_CHECK_ARG(partials_elems >= (int64_t)n_blocks);
  hipLaunchKernelGGL(grad_sq_partials_kernel, dim3((unsigned)n_blocks), dim3(kThreads), 0, S_(stream), segments, n_segments, grad,
                     grad_scale, partials);
  hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(kThreads), 0, S_(stream), partials, n_blocks, hyper);
  return hip_status(hipGetLastError());
}
