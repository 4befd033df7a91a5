// eval_problem.h — the problem layout of the detection evaluation (include/detops.h, "Detection evaluation"), shared by
// evaluate.hip and eval_oks.hip: dt_offset / gt_offset [P + 1] delimit a problem's rows and columns in the sorted arrays,
// iou_offset [P + 1] (int64) its D_p x G_p row-major matrix; a flat pair index finds its problem by bisection of
// iou_offset.  A pair index outside its problem's matrix (inconsistent offsets) decodes to p = -1: the caller writes 0 and
// reads nothing.
#pragma once
#include "detops_dtype.h"

namespace {

struct Pair {
  int p, d, g;        // problem, detection and ground truth (indices into the sorted arrays), or p = -1
};

__device__ __forceinline__ Pair pair_of(const int32_t* __restrict__ dt_offset, const int32_t* __restrict__ gt_offset,
                                        const int64_t* __restrict__ iou_offset, int P, int64_t idx) {
  Pair r;
  r.p = last_at_or_below(iou_offset, P, idx);   // the problem that owns flat pair `idx` (problems without pairs own nothing)
  const int d0 = dt_offset[r.p], g0 = gt_offset[r.p];
  const int D = dt_offset[r.p + 1] - d0, G = gt_offset[r.p + 1] - g0;
  const int64_t local = idx - iou_offset[r.p];
  if (D <= 0 || G <= 0 || local < 0 || local >= static_cast<int64_t>(D) * G) { r.p = -1; r.d = r.g = 0; return r; }
  r.d = d0 + static_cast<int>(local / G);
  r.g = g0 + static_cast<int>(local % G);
  return r;
}

bool bad_problem_args(const void* dt_offset, const void* gt_offset, const void* iou_offset, int P) {
  return P < 0 || (P > 0 && (!dt_offset || !gt_offset || !iou_offset));
}

}  // namespace
