// Bootstrap resampling of per-video metric values for gfx950: R resamples of N videos, each a
// vector of N integer counts, and per resample and column the ratio of two count-weighted sums.  One launch on the
// caller's stream, no host read, no global atomics.
//
//   counts   a workgroup carries kRows consecutive rows of the output (row 0 = the observed statistic, every count 1; row
//            r >= 1 = resample r).  Its counts sit in LDS, N words per row: zeroed, then every thread makes its share of the
//            N draws of each row with an LDS integer add.  Integers: the order of the adds does not matter.
//   sums     a wave takes kCols columns of the workgroup's column block at a time.  Lane t reads videos t, t + 64, ... in
//            ascending order -- the 64 lanes read 512 consecutive bytes of each column -- one loaded value serves all kRows
//            count rows and one converted count all kCols columns.  Then the xor butterfly 32, 16, .. 1 per (row, column)
//            and lane 0 stores the ratios.
//   split    grid (ceil((R + 1) / kRows), ceil(M / kColBlock)).  Workgroups that share rows regenerate the same counts.
//
// The definition (include/bmhrl_hip.h) is in fp64 in a stated order.  Nothing here may be contracted or reassociated:
#pragma clang fp contract(off)
#include "common.h"
#include "../../include/bmhrl_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / WAVE;
constexpr int kColBlock = 128;                // columns of one workgroup
// The entry point takes as many rows per workgroup (4, 2 or 1) as keep its counts within kLdsBudget bytes: four
// workgroups per CU by LDS (bmhrl_bootstrap_rows answers what it takes).
constexpr int kLdsBudget = 40 * 1024;
// the columns a wave sums at a time (one read and conversion of a count serves them all)
constexpr int kCols = 4;

#define S_(s) ((hipStream_t)(s))

__device__ __forceinline__ double wave_sum_xor(double p) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) p = p + __shfl_xor(p, s, 64);
  return p;
}

// One wave, columns m .. m + kCols - 1 (those below m_end; the others repeat column m_end - 1 and store nothing), all kRows
// count rows: a count is read and converted once for the kCols columns, a value is loaded once for the kRows rows, and every
// (row, column) pair keeps its own lane sum in the definition's order.
template <int kRows, bool kWeighted>
__device__ __forceinline__ void column_sums(const double* __restrict__ values, const double* __restrict__ weights,
                                            const uint32_t* cnt, int N, int M, int R, long row0, int m, int m_end, int lane,
                                            double* __restrict__ stats) {
  const double* x[kCols];
  const double* w[kCols];
  double num[kRows][kCols], den[kRows][kCols];
#pragma unroll
  for (int q = 0; q < kCols; ++q) {
    const long col = min(m + q, m_end - 1);
    x[q] = values + col * N;
    w[q] = kWeighted ? weights + col * N : nullptr;
#pragma unroll
    for (int k = 0; k < kRows; ++k) num[k][q] = den[k][q] = 0.0;
  }
#pragma unroll 2
  for (int i = lane; i < N; i += WAVE) {
    double c[kRows], xv[kCols], wv[kCols];
#pragma unroll
    for (int q = 0; q < kCols; ++q) {
      xv[q] = x[q][i];
      wv[q] = kWeighted ? w[q][i] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < kRows; ++k) c[k] = (double)cnt[k * N + i];
#pragma unroll
    for (int k = 0; k < kRows; ++k)
#pragma unroll
      for (int q = 0; q < kCols; ++q) {
        num[k][q] = num[k][q] + (c[k] * xv[q]);
        if (kWeighted) den[k][q] = den[k][q] + (c[k] * wv[q]);
      }
  }
#pragma unroll
  for (int k = 0; k < kRows; ++k)
#pragma unroll
    for (int q = 0; q < kCols; ++q) {
      const long r = row0 + k;
      const double s_num = wave_sum_xor(num[k][q]);
      double stat;
      if (kWeighted) {
        const double s_den = wave_sum_xor(den[k][q]);
        stat = s_den == 0.0 ? 0.0 : s_num / s_den;
      } else {
        stat = s_num / (double)N;
      }
      if (lane == 0 && r <= R && m + q < m_end) stats[r * (long)M + (m + q)] = stat;
    }
}

// grid (row blocks, column blocks), kThreads threads, kRows * N words of dynamic LDS.  N <= BMHRL_BOOTSTRAP_MAX_N: checked
// by the entry point; every LDS index is a video index < N or k * N + one.
template <int kRows>
__global__ __launch_bounds__(kThreads) void bootstrap_kernel(const double* __restrict__ values, const double* __restrict__ weights,
                                                             int N, int M, int R, uint64_t seed, double* __restrict__ stats) {
  extern __shared__ __attribute__((aligned(16))) uint32_t cnt[];      // cnt[k * N + i]
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1), wave = tid / WAVE;
  const long row0 = (long)blockIdx.x * kRows;                          // rows row0 .. row0 + kRows - 1, those <= R

  // ---- counts
  for (int i = tid; i < kRows * N; i += kThreads) cnt[i] = (row0 == 0 && i < N) ? 1u : 0u;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kRows; ++k) {
    const long r = row0 + k;
    if (r == 0 || r > R) continue;             // (uniform: the observed row is all ones, a row past R stays zero, unwritten)
    for (int j = tid; j < N; j += kThreads) {
      const uint32_t h = hash_u32(seed, ((uint64_t)r << 32) | (uint64_t)(uint32_t)j);
      const uint32_t i = (uint32_t)(((uint64_t)h * (uint64_t)(uint32_t)N) >> 32);      // < N
      atomicAdd(&cnt[k * N + (int)i], 1u);
    }
  }
  __syncthreads();

  // ---- sums
  const int m_end = min(M, ((int)blockIdx.y + 1) * kColBlock);
  for (int m = (int)blockIdx.y * kColBlock + wave * kCols; m < m_end; m += kWaves * kCols) {
    if (weights)
      column_sums<kRows, true>(values, weights, cnt, N, M, R, row0, m, m_end, lane, stats);
    else
      column_sums<kRows, false>(values, nullptr, cnt, N, M, R, row0, m, m_end, lane, stats);
  }
}

template <int kRows>
int launch(const double* values, const double* weights, int N, int M, int R, uint64_t seed, double* stats, hipStream_t stream) {
  const unsigned row_blocks = (unsigned)(((long)R + 1 + kRows - 1) / kRows);
  const unsigned col_blocks = (unsigned)((M + kColBlock - 1) / kColBlock);
  const size_t lds = (size_t)kRows * N * sizeof(uint32_t);             // at most 64 KiB: one row of the largest N
  hipLaunchKernelGGL(bootstrap_kernel<kRows>, dim3(row_blocks, col_blocks), dim3(kThreads), lds, stream, values, weights, N, M, R,
                     seed, stats);
  return hip_status(hipGetLastError());
}

}  // namespace

extern "C" int bmhrl_bootstrap_rows(int32_t N, int32_t resamples) {
  BMHRL_CHECK_ARG(N >= 1 && N <= BMHRL_BOOTSTRAP_MAX_N && resamples >= 1 && resamples <= BMHRL_BOOTSTRAP_MAX_R);
  const long row_bytes = (long)N * (long)sizeof(uint32_t);
  if (4 * row_bytes <= kLdsBudget && resamples >= 3) return 4;
  if (2 * row_bytes <= kLdsBudget) return 2;
  return 1;
}

extern "C" int bmhrl_bootstrap_ratios(const double* values, const double* weights, int32_t N, int32_t M, int32_t resamples,
                                      uint64_t seed, double* stats, bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(values && stats);
  BMHRL_CHECK_ARG(N >= 1 && N <= BMHRL_BOOTSTRAP_MAX_N && M >= 1 && M <= BMHRL_BOOTSTRAP_MAX_M);
  BMHRL_CHECK_ARG(resamples >= 1 && resamples <= BMHRL_BOOTSTRAP_MAX_R);
  switch (bmhrl_bootstrap_rows(N, resamples)) {
    case 4: return launch<4>(values, weights, N, M, resamples, seed, stats, S_(stream));
    case 2: return launch<2>(values, weights, N, M, resamples, seed, stats, S_(stream));
    default: return launch<1>(values, weights, N, M, resamples, seed, stats, S_(stream));
  }
}
