// evaluate.tiou on the device: the temporal intersection over union of a prediction (s_i, e_i) and a reference (s, e) with
// the union capped by the sum of the two lengths and 1e-8 added to it, fp64, term for term in the order of the Python
// function -- so a translation unit that includes this with `#pragma clang fp contract(off)` in force and without
// fast-math gets that function's bits.  proposal_eval.hip uses it; the cell cost of soda.hip and the NMS loop of
// proposal.hip spell the same expression out and can adopt it.
#pragma once
#include <math.h>

__device__ __forceinline__ double tiou_f64(double s_i, double e_i, double s, double e) {
  const double d = fmin(e, e_i) - fmax(s, s_i);
  const double inter = d > 0.0 ? d : 0.0;                   // max(0, d)
  const double span = fmax(e, e_i) - fmin(s, s_i);
  const double sum = ((e - s) + e_i) - s_i;                 // end - start + end_i - start_i, left to right
  const double uni = fmin(span, sum);
  return inter / (uni + 1e-8);
}
