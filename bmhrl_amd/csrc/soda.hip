// SODA_c dense-captioning evaluation (bmhrl_amd/evaluate.py soda_scores; the rules are in DESIGN.md section 25): the
// whole-sentence METEOR of every prediction of a (video, file) group against every reference of the group, and the
// time-ordered one-to-one assignment that maximises the sum of tIoU x METEOR, as two launches with nothing read back
// between them.
//
// bmhrl_meteor_matrix.  One workgroup per matrix row, that is per (group, prediction).  The workgroup fetches what the
// hypothesis's tokens bring along (word id, stem id, synonym row bounds: the vocabulary tables are read once per row, not
// once per cell) and compacts the words in LDS, as meteor.hip does.  Its waves then take the group's references in turn: a
// wave loads the reference's words and stems straight into the registers of the lanes that own the positions, evaluates
// which positions every hypothesis word's synonym set selects (one bit mask per word, in the wave's own slice of LDS) and
// aligns the whole hypothesis once with align_prefix (meteor_align.h) -- the alignment the per-prefix launch runs for its
// last prefix, so a cell has the bits of that launch's column L - 1.  Sentences and references are named by index
// (hyp_idx, ref_idx): no pair rows exist anywhere.
//
// bmhrl_soda_dp.  One wave per (group, threshold).  The lanes own the references (j = 64 q + lane, up to four per lane); a
// row of D[i][j] = max(D[i-1][j], D[i][j-1], D[i-1][j-1] + c[i][j]) is the prefix maximum over j of
// a[j] = max(D[i-1][j], D[i-1][j-1] + c[i][j]): one shuffle-up, one add, one max and a wave scan with max.  Rows run in
// sequence; the next row's scores and segment are loaded while the current one is scanned.  max is exact in any order and
// every add is the D + c of the plain double loop, so the result has that loop's bits.
//
// No atomics; nothing is written outside S / out.  Contraction to FMA is off in this file: every product and sum rounds
// as the reference's Python arithmetic does.
#include <math.h>
#include <vector>
#include "common.h"
#include "../../include/bmhrl_hip.h"

#pragma clang fp contract(off)

#include "meteor_align.h"

#define S_(x) ((hipStream_t)(x))

namespace {

constexpr int kRowThreads = 256;                     // matrix launch: at most four waves per row
constexpr int kDpWaves = 4;                          // DP launch: (group, threshold) items per workgroup
constexpr int kDpQ = BMHRL_SODA_MAX_REFS / WAVE;     // references per lane
static_assert(BMHRL_SODA_MAX_REFS % WAVE == 0, "whole waves of references");

__global__ __launch_bounds__(kRowThreads) void meteor_matrix_kernel(
    const int64_t* __restrict__ hyp, long ldh, const int32_t* __restrict__ vmap, const int32_t* __restrict__ vstem, int V,
    const int32_t* __restrict__ syn_off, const int32_t* __restrict__ syn_ids, int n_syn, const int32_t* __restrict__ ref,
    const int32_t* __restrict__ ref_stem, long ldr, const int32_t* __restrict__ ref_len, int L, int R,
    const int32_t* __restrict__ hyp_idx, const int32_t* __restrict__ ref_idx, const int32_t* __restrict__ hyp_off,
    const int32_t* __restrict__ ref_off, const int64_t* __restrict__ cell_off, int G, double alpha, double beta, double gamma,
    double* __restrict__ S) {
  __shared__ HypWords s_h;               // the tokens and the compacted hypothesis words (caption_text.h)
  __shared__ int s_g;
  extern __shared__ __attribute__((aligned(16))) u64 s_syn_all[];      // per wave: (L, kQ) synonym masks of the current cell

  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), nthreads = blockDim.x;
  const int wave = __builtin_amdgcn_readfirstlane(tid / WAVE), nwaves = nthreads / WAVE;
  if (tid == 0) s_g = group_of(hyp_off, G, row);
  stage_hyp_words(s_h, hyp + (size_t)hyp_idx[row] * ldh, L, nthreads, vmap, vstem, V, syn_off, n_syn);
  const int M = __builtin_amdgcn_readfirstlane(s_h.mc[L - 1]);
  const int g = __builtin_amdgcn_readfirstlane(s_g);
  const int r0 = ref_off[g], Rg = ref_off[g + 1] - r0;
  double* out = S + cell_off[g] + (long)(row - hyp_off[g]) * Rg;

  int hw[kP], hs[kP];
#pragma unroll
  for (int p = 0; p < kP; ++p) {
    const int h = p * WAVE + lane;
    hw[p] = h < M ? s_h.hw[h] : -1;
    hs[p] = h < M ? s_h.hs[h] : -1;
  }
  u64 (*syn)[kQ] = (u64 (*)[kQ])(s_syn_all + (size_t)wave * L * kQ);

  // no workgroup barrier below: the waves run different numbers of cells
  for (int j = wave; j < Rg; j += nwaves) {
    const size_t rrow = (size_t)ref_idx[r0 + j] * ldr;
    const int Rb = __builtin_amdgcn_readfirstlane(clampi(ref_len[ref_idx[r0 + j]], 0, R));
    const int nq = (Rb + WAVE - 1) / WAVE;
    // this lane's reference positions (those behind the reference start out used)
    int rw[kQ], rs[kQ];
    unsigned used0 = 0;
#pragma unroll
    for (int q = 0; q < kQ; ++q) {
      const int r = q * WAVE + lane;
      const bool ok = r < Rb;
      rw[q] = ok ? ref[rrow + r] : -1;
      rs[q] = ok && vstem ? ref_stem[rrow + r] : -1;
      used0 |= ok ? 0u : 1u << q;
    }
    double score = 0.0;
    if (M > 0 && Rb > 0) {
      if (syn_off) {
        for (int h = 0; h < M; ++h) {           // 64 ids of the word's row per load, one per lane
          const int w = s_h.hw[h], beg = s_h.hb[h], end = s_h.he[h];
          bool hit[kQ];
#pragma unroll
          for (int q = 0; q < kQ; ++q) hit[q] = rw[q] == w;
          for (int e0 = beg; e0 < end; e0 += WAVE) {
            const int mine = e0 + lane < end ? syn_ids[e0 + lane] : -1;
            const int n = end - e0 < WAVE ? end - e0 : WAVE;
            for (int i = 0; i < n; ++i) {
              const int id = __builtin_amdgcn_readlane(mine, i);
#pragma unroll
              for (int q = 0; q < kQ; ++q) hit[q] |= rw[q] == id;
            }
          }
#pragma unroll
          for (int q = 0; q < kQ; ++q) {
            if (q < nq) {                       // the groups of 64 behind the reference are never read
              const u64 bal = __ballot(hit[q] && !((used0 >> q) & 1u));
              if (lane == 0) syn[h][q] = bal;
            }
          }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");     // lane 0's masks, read by every lane of this wave
      }
      int matches, chunks;
      if (nq == 1)
        align_prefix<1>(M, nq, lane, vstem != nullptr, syn_off != nullptr, hw, hs, syn, rw, rs, used0, matches, chunks);
      else
        align_prefix<kQ>(M, nq, lane, vstem != nullptr, syn_off != nullptr, hw, hs, syn, rw, rs, used0, matches, chunks);
      score = meteor_score(matches, chunks, M, Rb, alpha, beta, gamma);
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");       // the masks are read before the next cell rewrites them
    }
    if (lane == 0) out[j] = score;
  }
}

// inclusive prefix maximum over the lanes of a wave
__device__ __forceinline__ double wave_prefix_max(double v, int lane) {
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const double o = __shfl_up(v, d, WAVE);
    if (lane >= d) v = fmax(v, o);
  }
  return v;
}

// NQ: the groups of 64 references the code covers
template <int NQ>
__device__ __forceinline__ double soda_dp_rows(const double* __restrict__ pseg, const double* __restrict__ rseg,
                                               const double* __restrict__ S, int P, int R, double thr, int lane) {
  double rs[NQ], re[NQ], D[NQ], sn[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int j = q * WAVE + lane;
    rs[q] = j < R ? rseg[2 * (size_t)j] : 0.0;
    re[q] = j < R ? rseg[2 * (size_t)j + 1] : 0.0;
    sn[q] = j < R ? S[j] : 0.0;
    D[q] = 0.0;
  }
  double ps_n = pseg[0], pe_n = pseg[1];
  for (int i = 0; i < P; ++i) {
    double s[NQ];
    const double ps = ps_n, pe = pe_n;
#pragma unroll
    for (int q = 0; q < NQ; ++q) s[q] = sn[q];
    if (i + 1 < P) {                            // the next row is in flight while this one is scanned
      ps_n = pseg[2 * (size_t)(i + 1)];
      pe_n = pseg[2 * (size_t)(i + 1) + 1];
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int j = q * WAVE + lane;
        sn[q] = j < R ? S[(size_t)(i + 1) * R + j] : 0.0;
      }
    }
    double carry = 0.0, below = 0.0;            // D[i][64 q - 1] and D[i-1][64 q - 1]
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int j = q * WAVE + lane;
      // evaluate.tiou(prediction, reference), in its order
      const double lo = fmax(rs[q], ps), hi = fmin(re[q], pe);
      const double d = hi - lo;
      const double inter = d > 0.0 ? d : 0.0;
      const double span = fmax(re[q], pe) - fmin(rs[q], ps);
      const double sum = ((re[q] - rs[q]) + pe) - ps;
      const double uni = fmin(span, sum);
      const double iou = inter / (uni + 1e-8);
      const double c = j < R ? (iou < thr ? 0.0 : iou) * s[q] : 0.0;
      double diag = __shfl_up(D[q], 1, WAVE);
      if (lane == 0) diag = below;
      below = __shfl(D[q], WAVE - 1, WAVE);
      const double a = fmax(D[q], diag + c);
      D[q] = fmax(wave_prefix_max(a, lane), carry);
      carry = __shfl(D[q], WAVE - 1, WAVE);
    }
  }
  double last = 0.0;
#pragma unroll
  for (int q = 0; q < NQ; ++q)
    if ((R - 1) / WAVE == q) last = __shfl(D[q], (R - 1) % WAVE, WAVE);
  return last;
}

__global__ __launch_bounds__(kDpWaves * WAVE) void soda_dp_kernel(
    const double* __restrict__ pred_seg, const double* __restrict__ ref_seg, const int32_t* __restrict__ hyp_off,
    const int32_t* __restrict__ ref_off, const int64_t* __restrict__ cell_off, const double* __restrict__ S,
    const double* __restrict__ tious, int G, int T, double* __restrict__ out) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const long item = (long)blockIdx.x * kDpWaves + wave;      // (group, threshold), thresholds of a group side by side
  if (item >= (long)G * T) return;
  const int g = (int)(item / T), t = (int)(item % T);
  const int p0 = hyp_off[g], P = hyp_off[g + 1] - p0, r0 = ref_off[g], R = ref_off[g + 1] - r0;
  double best = 0.0, prec = 0.0, rec = 0.0, f = 0.0;
  if (P > 0 && R > 0) {
    const double* ps = pred_seg + 2 * (size_t)p0;
    const double* rs = ref_seg + 2 * (size_t)r0;
    const double* Sg = S + cell_off[g];
    const double thr = tious[t];
    if (R <= WAVE) best = soda_dp_rows<1>(ps, rs, Sg, P, R, thr, lane);
    else if (R <= 2 * WAVE) best = soda_dp_rows<2>(ps, rs, Sg, P, R, thr, lane);
    else best = soda_dp_rows<kDpQ>(ps, rs, Sg, P, R, thr, lane);
    prec = best / (double)P;
    rec = best / (double)R;
    const double den = prec + rec;
    f = den == 0.0 ? 0.0 : ((2.0 * prec) * rec) / den;
  }
  if (lane == 0) {
    double* o = out + (size_t)item * 4;
    o[0] = best;
    o[1] = prec;
    o[2] = rec;
    o[3] = f;
  }
}

// the three offset arrays of a call, copied back: ascending from 0, spanning the index arrays, cells = P_g * R_g
struct Offsets {
  std::vector<int32_t> hyp, ref;
  std::vector<int64_t> cell;
};

int check_offsets(const Offsets& o, int G, int64_t n_pred, int64_t n_ref, int64_t n_cells, int max_refs) {
  BMHRL_CHECK_ARG(o.hyp[0] == 0 && o.ref[0] == 0 && o.cell[0] == 0);
  BMHRL_CHECK_ARG(o.hyp[G] == n_pred && o.ref[G] == n_ref && o.cell[G] == n_cells);
  for (int g = 0; g < G; ++g) {
    BMHRL_CHECK_ARG(o.hyp[g] <= o.hyp[g + 1] && o.ref[g] <= o.ref[g + 1]);
    BMHRL_CHECK_ARG(max_refs <= 0 || o.ref[g + 1] - o.ref[g] <= max_refs);
    BMHRL_CHECK_ARG(o.cell[g + 1] - o.cell[g] == (int64_t)(o.hyp[g + 1] - o.hyp[g]) * (int64_t)(o.ref[g + 1] - o.ref[g]));
  }
  return 0;
}

}  // namespace

extern "C" int bmhrl_meteor_matrix(const int64_t* hyp, int64_t ldh, int32_t Nh, int32_t L, const int32_t* vmap,
                                   const int32_t* vstem, int32_t V, const int32_t* syn_off, const int32_t* syn_ids,
                                   int32_t n_syn, const int32_t* ref, const int32_t* ref_stem, int64_t ldr,
                                   const int32_t* ref_len, int32_t Nr, int32_t R, const int32_t* hyp_idx, int32_t n_pred,
                                   const int32_t* ref_idx, int32_t n_ref, const int32_t* hyp_off, const int32_t* ref_off,
                                   const int64_t* cell_off, int32_t G, double alpha, double beta, double gamma, double* S,
                                   int64_t n_cells, bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(hyp && vmap && ref && ref_len && hyp_idx && ref_idx && hyp_off && ref_off && cell_off && S);
  BMHRL_CHECK_ARG(!vstem || ref_stem);
  BMHRL_CHECK_ARG((syn_off != nullptr) == (syn_ids != nullptr));
  BMHRL_CHECK_ARG(!syn_off || n_syn >= 0);
  BMHRL_CHECK_ARG(G > 0 && Nh >= 1 && Nr >= 1 && L >= 1 && L <= kMaxL && R >= 1 && R <= kMaxR && V >= 1);
  BMHRL_CHECK_ARG(ldh >= L && ldr >= R && n_pred >= 0 && n_ref >= 0 && n_cells >= 0);
  // the offsets and indices decide which rows a workgroup reads and which cells it writes: they are checked here, before
  // the launch (small copies back, one synchronisation)
  Offsets o;
  o.hyp.resize((size_t)G + 1);
  o.ref.resize((size_t)G + 1);
  o.cell.resize((size_t)G + 1);
  std::vector<int32_t> hi((size_t)n_pred), ri((size_t)n_ref);
  hipError_t e = hipMemcpyAsync(o.hyp.data(), hyp_off, o.hyp.size() * sizeof(int32_t), hipMemcpyDeviceToHost, S_(stream));
  if (e == hipSuccess)
    e = hipMemcpyAsync(o.ref.data(), ref_off, o.ref.size() * sizeof(int32_t), hipMemcpyDeviceToHost, S_(stream));
  if (e == hipSuccess)
    e = hipMemcpyAsync(o.cell.data(), cell_off, o.cell.size() * sizeof(int64_t), hipMemcpyDeviceToHost, S_(stream));
  if (e == hipSuccess && n_pred > 0)
    e = hipMemcpyAsync(hi.data(), hyp_idx, hi.size() * sizeof(int32_t), hipMemcpyDeviceToHost, S_(stream));
  if (e == hipSuccess && n_ref > 0)
    e = hipMemcpyAsync(ri.data(), ref_idx, ri.size() * sizeof(int32_t), hipMemcpyDeviceToHost, S_(stream));
  if (e == hipSuccess) e = hipStreamSynchronize(S_(stream));
  if (e != hipSuccess) return hip_status(e);
  if (int rc = check_offsets(o, G, n_pred, n_ref, n_cells, 0)) return rc;
  for (int32_t v : hi) BMHRL_CHECK_ARG(v >= 0 && v < Nh);
  for (int32_t v : ri) BMHRL_CHECK_ARG(v >= 0 && v < Nr);
  if (n_pred == 0 || n_cells == 0) return 0;             // no cell to write
  // a wave keeps (L, kQ) masks in LDS: four waves up to 128 tokens, two beyond (32 KiB at most)
  const int waves = L <= kMaxL / 2 ? kRowThreads / WAVE : kRowThreads / WAVE / 2;
  const size_t lds = (size_t)waves * L * kQ * sizeof(u64);
  hipLaunchKernelGGL(meteor_matrix_kernel, dim3(n_pred), dim3(waves * WAVE), lds, S_(stream), hyp, (long)ldh, vmap, vstem, V,
                     syn_off, syn_ids, n_syn, ref, ref_stem, (long)ldr, ref_len, L, R, hyp_idx, ref_idx, hyp_off, ref_off,
                     cell_off, G, alpha, beta, gamma, S);
  return hip_status(hipGetLastError());
}

extern "C" int bmhrl_soda_dp(const double* pred_seg, int32_t n_pred, const double* ref_seg, int32_t n_ref,
                             const int32_t* hyp_off, const int32_t* ref_off, const int64_t* cell_off, int32_t G,
                             const double* S, int64_t n_cells, const double* tious, int32_t T, double* out,
                             bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(pred_seg && ref_seg && hyp_off && ref_off && cell_off && S && tious && out);
  BMHRL_CHECK_ARG(G > 0 && T >= 1 && T <= BMHRL_SODA_MAX_T && n_pred >= 0 && n_ref >= 0 && n_cells >= 0);
  Offsets o;
  o.hyp.resize((size_t)G + 1);
  o.ref.resize((size_t)G + 1);
  o.cell.resize((size_t)G + 1);
  hipError_t e = hipMemcpyAsync(o.hyp.data(), hyp_off, o.hyp.size() * sizeof(int32_t), hipMemcpyDeviceToHost, S_(stream));
  if (e == hipSuccess)
    e = hipMemcpyAsync(o.ref.data(), ref_off, o.ref.size() * sizeof(int32_t), hipMemcpyDeviceToHost, S_(stream));
  if (e == hipSuccess)
    e = hipMemcpyAsync(o.cell.data(), cell_off, o.cell.size() * sizeof(int64_t), hipMemcpyDeviceToHost, S_(stream));
  if (e == hipSuccess) e = hipStreamSynchronize(S_(stream));
  if (e != hipSuccess) return hip_status(e);
  if (int rc = check_offsets(o, G, n_pred, n_ref, n_cells, BMHRL_SODA_MAX_REFS)) return rc;
  const long items = (long)G * T;
  hipLaunchKernelGGL(soda_dp_kernel, dim3((unsigned)((items + kDpWaves - 1) / kDpWaves)), dim3(kDpWaves * WAVE), 0, S_(stream),
                     pred_seg, ref_seg, hyp_off, ref_off, cell_off, S, tious, G, T, out);
  return hip_status(hipGetLastError());
}
