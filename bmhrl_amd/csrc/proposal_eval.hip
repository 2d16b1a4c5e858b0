// Proposal metrics (bmhrl_amd/evaluate.py segment_tables / detection_scores_device / pair_indices_device /
// proposal_recall; the rules are in DESIGN.md section 28): the tIoU of every prediction of a group against every reference
// of the group, evaluated once and left as the integers that detection precision / recall, AR@AN and the caption pairing
// are built from.
//
// A group names a run of predictions and a run of references (a (video, file) or a whole video).  Groups are small
// (ActivityNet: about 100 predictions, 4 references) and a cell costs about ten fp64 operations, so the arithmetic does
// not matter: the launches are laid out around their loads and stores -- a prediction's segment is loaded once, a
// reference's once per chunk of 64 predictions as one uniform load, and pred_hits is stored once, in wave-wide rows.
// (Measured in DESIGN.md section 28: at ActivityNet size a launch lasts tens of microseconds, the dependent loads of one
// wave, far from the HBM rate.)
//
// bmhrl_tiou_hits.  One wave per group, four per workgroup.  The lanes own the predictions i = 64 q + lane; the references
// are walked by the whole wave together (the segment is one uniform 16-byte load).  A cell's tIoU is computed once and
// compared with every threshold: the per-lane counts are pred_hits and stay in registers until the chunk's references are
// done, the ballot of the comparison over the wave gives the first passing prediction of the chunk, which lane t keeps for
// threshold t.  A reference's first rank is stored by chunk 0 and lowered by a later chunk only where it is still unset
// (the same lane re-reads its own word).  No atomics, no LDS, no sums across waves: equal inputs give equal bits.
//
// bmhrl_tiou_pairs.  The same ownership; a lane walks its prediction's references in order and writes the rows that pass
// behind pair_off[slot], or one -1.  A write outside [pair_off[slot], pair_off[slot + 1]) or outside pair_ref is dropped,
// so a pair_off that does not belong to the segments cannot make the kernel write out of bounds.
//
// Contraction to FMA is off in this file: tiou_f64 rounds as evaluate.tiou does.
#include <math.h>
#include "common.h"
#include "../../include/bmhrl_hip.h"

#pragma clang fp contract(off)

#include "tiou.h"

#define S_(x) ((hipStream_t)(x))

namespace {

constexpr int kWaves = 4;                            // groups per workgroup

struct Seg {
  double s, e;
};

// a group as the kernels use it: the runs and where the group's outputs start
struct GroupRow {
  int p0, P, r0, R;
  long po, ro;
  bool ok;
};

// Row g of the device tables.  The host copy of the table was checked before the launch; the device copy is checked
// again here against the same bounds (a handful of uniform compares), so tables that disagree cannot make a wave read or
// write outside the arrays: such a group writes nothing.
__device__ __forceinline__ GroupRow load_group(const int32_t* __restrict__ groups, const int64_t* __restrict__ out_off, int G,
                                               long g, int n_pred, int n_ref, long ldp, long ldr) {
  GroupRow r;
  r.p0 = groups[4 * g], r.P = groups[4 * g + 1], r.r0 = groups[4 * g + 2], r.R = groups[4 * g + 3];
  r.po = out_off[g], r.ro = out_off[(long)G + 1 + g];
  r.ok = r.p0 >= 0 && r.P >= 0 && r.r0 >= 0 && r.R >= 0 && (long)r.p0 + r.P <= n_pred && (long)r.r0 + r.R <= n_ref &&
         r.po >= 0 && r.ro >= 0 && r.po + r.P <= ldp && r.ro + r.R <= ldr;
  return r;
}

// TT: the thresholds the code covers (those behind T are +inf, which no tIoU reaches)
template <int TT>
__global__ __launch_bounds__(kWaves * WAVE) void tiou_hits_kernel(
    const Seg* __restrict__ pred_seg, int n_pred, const Seg* __restrict__ ref_seg, int n_ref,
    const int32_t* __restrict__ groups, const int64_t* __restrict__ out_off, int G, const double* __restrict__ tious, int T,
    int strict, int32_t* __restrict__ pred_hits, long ldp, int32_t* ref_first, long ldr) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const long g = (long)blockIdx.x * kWaves + wave;
  if (g >= G) return;
  const GroupRow gr = load_group(groups, out_off, G, g, n_pred, n_ref, ldp, ldr);
  if (!gr.ok) return;
  const int P = gr.P, R = gr.R;
  double thr[TT];
#pragma unroll
  for (int t = 0; t < TT; ++t) thr[t] = t < T ? tious[t] : INFINITY;
  const Seg* refs = ref_seg + gr.r0;
  const int nq = P > 0 ? (P + WAVE - 1) / WAVE : 1;             // a group without predictions still writes P to its references
  for (int q = 0; q < nq; ++q) {
    const int i = q * WAVE + lane;
    const bool live = i < P;
    Seg p = {0.0, 0.0};
    if (live) p = pred_seg[(long)gr.p0 + i];
    int cnt[TT];
#pragma unroll
    for (int t = 0; t < TT; ++t) cnt[t] = 0;
    for (int j = 0; j < R; ++j) {
      const Seg r = refs[j];
      const double iou = tiou_f64(p.s, p.e, r.s, r.e);
      int mine = P;
#pragma unroll
      for (int t = 0; t < TT; ++t) {
        const bool pass = live && (strict ? iou > thr[t] : iou >= thr[t]);
        cnt[t] += pass ? 1 : 0;
        const unsigned long long m = __ballot(pass);
        const int f = m ? q * WAVE + __builtin_ctzll(m) : P;
        if (lane == t) mine = f;
      }
      if (lane < T) {                                           // lane t: threshold t's row
        int32_t* first = ref_first + (long)lane * ldr + gr.ro + j;
        if (q == 0) *first = mine;
        else if (mine < P && *first == P) *first = mine;        // this lane's own earlier store
      }
    }
    if (live) {
      int32_t* o = pred_hits + gr.po + i;
#pragma unroll
      for (int t = 0; t < TT; ++t)
        if (t < T) o[(long)t * ldp] = cnt[t];
    }
  }
}

__global__ __launch_bounds__(kWaves * WAVE) void tiou_pairs_kernel(
    const Seg* __restrict__ pred_seg, int n_pred, const Seg* __restrict__ ref_seg, int n_ref,
    const int32_t* __restrict__ groups, const int64_t* __restrict__ out_off, int G, double tiou, long n_slots,
    const int64_t* __restrict__ pair_off, int32_t* __restrict__ pair_ref, long n_pairs) {
  const int lane = threadIdx.x & (WAVE - 1);
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / WAVE);
  const long g = (long)blockIdx.x * kWaves + wave;
  if (g >= G) return;
  const GroupRow gr = load_group(groups, out_off, G, g, n_pred, n_ref, n_slots, INT64_MAX);   // nothing is laid out by ro
  if (!gr.ok) return;
  const Seg* refs = ref_seg + gr.r0;
  for (int i = lane; i < gr.P; i += WAVE) {
    const Seg p = pred_seg[(long)gr.p0 + i];
    const long lo = pair_off[gr.po + i];
    long hi = pair_off[gr.po + i + 1];
    if (hi > n_pairs) hi = n_pairs;
    if (lo < 0 || lo >= hi) continue;                           // no room of its own: nothing is written
    long w = lo;
    for (int j = 0; j < gr.R; ++j) {
      const Seg r = refs[j];
      if (tiou_f64(p.s, p.e, r.s, r.e) >= tiou && w < hi) pair_ref[w++] = gr.r0 + j;
    }
    if (w == lo) pair_ref[lo] = -1;
  }
}

// the host copy of the group table: every run inside its array; the sums of the groups' own counts
int check_groups(const int32_t* groups, int G, int n_pred, int n_ref, int64_t& sum_p, int64_t& sum_r) {
  sum_p = sum_r = 0;
  for (int g = 0; g < G; ++g) {
    const int32_t p0 = groups[4 * g], P = groups[4 * g + 1], r0 = groups[4 * g + 2], R = groups[4 * g + 3];
    BMHRL_CHECK_ARG(p0 >= 0 && P >= 0 && r0 >= 0 && R >= 0);
    BMHRL_CHECK_ARG((int64_t)p0 + P <= n_pred && (int64_t)r0 + R <= n_ref);
    sum_p += P;
    sum_r += R;
  }
  return 0;
}

}  // namespace

extern "C" int bmhrl_tiou_hits(const double* pred_seg, int32_t n_pred, const double* ref_seg, int32_t n_ref,
                               const int32_t* groups_host, const int32_t* groups, const int64_t* out_off, int32_t G,
                               const double* tious, int32_t T, int32_t strict, int32_t* pred_hits, int64_t ld_pred,
                               int32_t* ref_first, int64_t ld_ref, bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(G >= 0 && n_pred >= 0 && n_ref >= 0 && T >= 1 && T <= BMHRL_TIOU_MAX_T && (strict == 0 || strict == 1));
  BMHRL_CHECK_ARG(tious && (pred_seg || n_pred == 0) && (ref_seg || n_ref == 0));
  if (G == 0) return 0;
  BMHRL_CHECK_ARG(groups_host && groups && out_off);
  int64_t sum_p, sum_r;
  if (int rc = check_groups(groups_host, G, n_pred, n_ref, sum_p, sum_r)) return rc;
  BMHRL_CHECK_ARG(ld_pred >= sum_p && ld_ref >= sum_r && (pred_hits || sum_p == 0) && (ref_first || sum_r == 0));
  const dim3 grid((unsigned)((G + kWaves - 1) / kWaves)), block(kWaves * WAVE);
  if (T <= 4)
    hipLaunchKernelGGL(tiou_hits_kernel<4>, grid, block, 0, S_(stream), (const Seg*)pred_seg, n_pred, (const Seg*)ref_seg,
                       n_ref, groups, out_off, G, tious, T, strict, pred_hits, (long)ld_pred, ref_first, (long)ld_ref);
  else
    hipLaunchKernelGGL(tiou_hits_kernel<BMHRL_TIOU_MAX_T>, grid, block, 0, S_(stream), (const Seg*)pred_seg, n_pred,
                       (const Seg*)ref_seg, n_ref, groups, out_off, G, tious, T, strict, pred_hits, (long)ld_pred, ref_first,
                       (long)ld_ref);
  return hip_status(hipGetLastError());
}

extern "C" int bmhrl_tiou_pairs(const double* pred_seg, int32_t n_pred, const double* ref_seg, int32_t n_ref,
                                const int32_t* groups_host, const int32_t* groups, const int64_t* out_off, int32_t G,
                                double tiou, const int64_t* pair_off, int64_t n_slots, int32_t* pair_ref, int64_t n_pairs,
                                bmhrl_stream_t stream) {
  BMHRL_CHECK_ARG(G >= 0 && n_pred >= 0 && n_ref >= 0 && n_slots >= 0 && n_pairs >= 0);
  BMHRL_CHECK_ARG((pred_seg || n_pred == 0) && (ref_seg || n_ref == 0));
  if (G == 0) return 0;
  BMHRL_CHECK_ARG(groups_host && groups && out_off && pair_off);
  int64_t sum_p, sum_r;
  if (int rc = check_groups(groups_host, G, n_pred, n_ref, sum_p, sum_r)) return rc;
  BMHRL_CHECK_ARG(n_slots == sum_p && (pair_ref || n_pairs == 0));
  if (sum_p == 0 || n_pairs == 0) return 0;
  hipLaunchKernelGGL(tiou_pairs_kernel, dim3((unsigned)((G + kWaves - 1) / kWaves)), dim3(kWaves * WAVE), 0, S_(stream),
                     (const Seg*)pred_seg, n_pred, (const Seg*)ref_seg, n_ref, groups, out_off, G, tiou, (long)n_slots, pair_off,
                     pair_ref, (long)n_pairs);
  return hip_status(hipGetLastError());
}
