// Gradient accumulation over a window of micro-batches (train.FlatAdam.accumulate): one launch per micro-batch.
//
// accum_segments_kernel walks the per-parameter table of bmhrl_adam_segments (7 int64 per parameter; word 0 the offset in
// the flat bucket, words 2 x 3 the element count, word 5 the first block, word 6 the gradient where autograd left it, 0 = the
// flat bucket at the parameter's offset; words 1 and 4 are not read).  One 256-thread block owns 4096 consecutive elements
// of one parameter, as in the Adam pass and the norm launch.  ctl = two fp32 words in device memory, so that a captured
// micro-step serves every micro-batch of a window: ctl[0] = w, the weight of this micro-batch; ctl[1] != 0 marks the first
// micro-batch, whose result is a plain store (accum is not read: whatever the last window -- or nobody -- left there, NaN
// included, is gone), every other one is accum = fma(w, g, accum).
// Purely elementwise: no sum across threads, the same bits in every run with and without BMHRL_DETERMINISTIC.  A whole
// block whose gradient and accumulator are 16-byte aligned requests all of its 16-byte loads (four of g, four of accum per
// thread) before the first use and stores 16 bytes; tails and a gradient at a 4- / 8-byte alignment take the scalar loop.
// The padding between one parameter's end and the next offset is never written.
// The window's loss rides along: block 0, thread 0 forms loss_out = (first ? 0 : loss_out) + w * loss_in.
#include "common.h"
#include "../../include/bmhrl_hip.h"

#define S_(x) ((hipStream_t)(x))

namespace {

constexpr int kWords = 7;            // table row of bmhrl_adam_segments
constexpr int kBlockElems = 4096;
constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void accum_segments_kernel(const int64_t* __restrict__ seg, int n_seg,
                                                                  const float* __restrict__ g, float* __restrict__ acc,
                                                                  const float* __restrict__ ctl,
                                                                  const float* __restrict__ loss_in, float* __restrict__ loss_out) {
  const float w = ctl[0];
  const bool first = ctl[1] != 0.f;
  if (loss_out && blockIdx.x == 0 && threadIdx.x == 0) loss_out[0] = (first ? 0.f : loss_out[0]) + w * loss_in[0];
  int lo = 0, hi = n_seg - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (seg[mid * kWords + 5] <= (int64_t)blockIdx.x) lo = mid; else hi = mid - 1;
  }
  const int64_t* e = seg + lo * kWords;
  // (a grid larger than the table's block count maps the extra blocks to the last row, where end < base: nothing is done)
  const long total = e[2] * e[3];
  const long base = ((long)blockIdx.x - e[5]) * kBlockElems;
  const long end = base + kBlockElems < total ? base + kBlockElems : total;
  const float* __restrict__ gp = e[6] ? reinterpret_cast<const float*>(e[6]) : g + e[0];
  float* __restrict__ ap = acc + e[0];
  if (end - base == kBlockElems && ((reinterpret_cast<uintptr_t>(gp) | reinterpret_cast<uintptr_t>(ap)) & 15) == 0) {
    f32x4 gv[4], av[4];
    if (first) {
#pragma unroll
      for (int it = 0; it < 4; ++it)
        gv[it] = *reinterpret_cast<const f32x4*>(gp + base + 4 * threadIdx.x + it * (kBlockElems / 4));
#pragma unroll
      for (int it = 0; it < 4; ++it)
        *reinterpret_cast<f32x4*>(ap + base + 4 * threadIdx.x + it * (kBlockElems / 4)) = gv[it] * w;
    } else {
#pragma unroll
      for (int it = 0; it < 4; ++it) {
        gv[it] = *reinterpret_cast<const f32x4*>(gp + base + 4 * threadIdx.x + it * (kBlockElems / 4));
        av[it] = *reinterpret_cast<const f32x4*>(ap + base + 4 * threadIdx.x + it * (kBlockElems / 4));
      }
#pragma unroll
      for (int it = 0; it < 4; ++it) {
#pragma unroll
        for (int j = 0; j < 4; ++j) av[it][j] = fmaf(w, gv[it][j], av[it][j]);
        *reinterpret_cast<f32x4*>(ap + base + 4 * threadIdx.x + it * (kBlockElems / 4)) = av[it];
      }
    }
    return;
  }
  if (first) {
    for (long i = base + threadIdx.x; i < end; i += kThreads) ap[i] = w * gp[i];
  } else {
    for (long i = base + threadIdx.x; i < end; i += kThreads) ap[i] = fmaf(w, gp[i], ap[i]);
  }
}

}  // namespace

extern "C" int bmhrl_accum_segments(const int64_t* segments, int32_t n_segments, int32_t n_blocks, const float* grad, float* accum,
                                    const float* ctl, const float* loss_in, float* loss_out, bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(segments && n_segments > 0 && n_blocks > 0 && grad && accum && ctl);
  BMHRL_CHECK_ARG((loss_in == nullptr) == (loss_out == nullptr));
  hipLaunchKernelGGL(accum_segments_kernel, dim3((unsigned)n_blocks), dim3(kThreads), 0, S_(stream), segments, n_segments, grad,
                     accum, ctl, loss_in, loss_out);
  return hip_status(hipGetLastError());
}
