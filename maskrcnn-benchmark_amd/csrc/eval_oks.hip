// eval_oks.hip — object keypoint similarity on the device, for gfx950 (MI355X).  The arithmetic is stated in
// include/detops.h ("Keypoint evaluation (OKS)"); maskrcnn_benchmark/_eval_cpu.py (eval_oks) is the same in numpy.
//
//   detops_eval_oks   keypoints of the sorted detections and ground truths -> the fp64 OKS matrix of every problem (the
//                     problem layout of detops_eval_iou: eval_problem.h) and the detections' keypoint-extent areas
//
// A batch holds hundreds of pairs of K = 17 keypoints: the work is latency, and nearly all of it is the K fp64 exp of a
// pair.  So a thread owns one TERM, not one pair: a pair is kMaxK consecutive lanes (half a wave), lane k computes
// exp(-e[k]), and lane 0 of the pair adds the terms that count in keypoint order, one after the other (the definition's
// order: the result has no reduction tree in it).  The ground truth's visible-keypoint count k1 is the popcount of the
// pair's half of one ballot.  A workgroup holds kPairs pairs; the workgroups behind the last pair compute the detections'
// areas, a thread per detection.  One launch, no atomics, every output element written exactly once.
#include "eval_problem.h"

namespace {

constexpr int kMaxK = DETOPS_EVAL_OKS_MAX_K;
constexpr int kBlock = 256;
constexpr int kPairs = kBlock / kMaxK;            // pairs of a workgroup
static_assert(kMaxK == 32 && kWave == 2 * kMaxK, "a pair is one half of a wave: its ballot bits are one 32-bit word");

__global__ void __launch_bounds__(kBlock)
eval_oks_kernel(const float* __restrict__ dt_kpts, const float* __restrict__ gt_kpts, const float* __restrict__ gt_boxes,
                const double* __restrict__ gt_area, const double* __restrict__ sigmas, int K,
                const int32_t* __restrict__ dt_offset, const int32_t* __restrict__ gt_offset,
                const int64_t* __restrict__ iou_offset, int P, int64_t D_total, int64_t total_pairs, unsigned pair_blocks,
                double* __restrict__ oks, double* __restrict__ dt_area) {
#pragma clang fp contract(off)
  __shared__ double term[kPairs][kMaxK];
  if (blockIdx.x >= pair_blocks) {                 // (uniform over the workgroup) the detections' areas
    const int64_t d = static_cast<int64_t>(blockIdx.x - pair_blocks) * kBlock + threadIdx.x;
    if (d >= D_total) return;
    const float* kp = dt_kpts + d * K * 3;
    float x0 = kp[0], x1 = kp[0], y0 = kp[1], y1 = kp[1];
    for (int k = 1; k < K; ++k) {                  // a NaN coordinate stays (numpy's min / max)
      const float x = kp[3 * k], y = kp[3 * k + 1];
      if (x < x0 || x != x) x0 = x;
      if (x > x1 || x != x) x1 = x;
      if (y < y0 || y != y) y0 = y;
      if (y > y1 || y != y) y1 = y;
    }
    const double w = static_cast<double>(x1) - static_cast<double>(x0);
    const double h = static_cast<double>(y1) - static_cast<double>(y0);
    dt_area[d] = w * h;
    return;
  }
  const int slot = threadIdx.x / kMaxK, k = threadIdx.x % kMaxK;
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kPairs + slot;
  const bool live = idx < total_pairs;
  Pair pr;
  pr.p = -1; pr.d = pr.g = 0;
  if (live) pr = pair_of(dt_offset, gt_offset, iou_offset, P, idx);
  const bool on = pr.p >= 0 && pr.d < D_total && k < K;
  float xd = 0.f, yd = 0.f, xg = 0.f, yg = 0.f, vg = 0.f;
  if (on) {
    const float* a = dt_kpts + (static_cast<int64_t>(pr.d) * K + k) * 3;      // (the detection's third column is not read)
    const float* b = gt_kpts + (static_cast<int64_t>(pr.g) * K + k) * 3;
    xd = a[0]; yd = a[1];
    xg = b[0]; yg = b[1]; vg = b[2];
  }
  const detops_u64 votes = __ballot(on && vg > 0.f);
  const unsigned visible = static_cast<unsigned>(votes >> (((threadIdx.x % kWave) / kMaxK) * kMaxK));
  const int k1 = __popc(visible);
  double t = 0.0;
  if (on) {
    const double XD = xd, YD = yd;
    double dx, dy;
    if (k1 > 0) {
      dx = XD - static_cast<double>(xg);
      dy = YD - static_cast<double>(yg);
    } else {
      // BoxList.convert("xywh") in fp32, then the box doubled around itself
      const float* box = gt_boxes + 4 * static_cast<int64_t>(pr.g);
      float bwf = box[2] - box[0]; bwf = bwf + 1.0f;
      float bhf = box[3] - box[1]; bhf = bhf + 1.0f;
      const double bx = box[0], by = box[1], bw = bwf, bh = bhf;
      const double x0 = bx - bw, x1 = bx + 2.0 * bw, y0 = by - bh, y1 = by + 2.0 * bh;
      dx = fmax(0.0, x0 - XD) + fmax(0.0, XD - x1);
      dy = fmax(0.0, y0 - YD) + fmax(0.0, YD - y1);
    }
    const double s2 = 2.0 * sigmas[k];
    const double var = s2 * s2;
    const double xx = dx * dx, yy = dy * dy;
    double e = xx + yy;
    e = e / var;
    e = e / (gt_area[pr.g] + 0x1p-52);
    e = e / 2.0;
    t = exp(-e);
  }
  term[slot][k] = t;
  __syncthreads();
  if (k != 0 || !live) return;
  double v = 0.0;
  if (pr.p >= 0 && pr.d < D_total) {
    double s = 0.0;
    for (int j = 0; j < K; ++j)
      if (k1 == 0 || ((visible >> j) & 1)) s = s + term[slot][j];
    v = s / static_cast<double>(k1 > 0 ? k1 : K);
  }
  oks[idx] = v;
}

}  // namespace

DETOPS_API int detops_eval_oks(const float* dt_kpts, const float* gt_kpts, const float* gt_boxes, const double* gt_area,
                               const double* sigmas, int K, const int32_t* dt_offset, const int32_t* gt_offset,
                               const int64_t* iou_offset, int P, int64_t D_total, int64_t total_pairs, double* oks,
                               double* dt_area, detops_stream_t stream) {
  if (K < 1 || D_total < 0 || total_pairs < 0 || bad_problem_args(dt_offset, gt_offset, iou_offset, P)) return DETOPS_EINVAL;
  if (K > kMaxK) return DETOPS_EUNSUPPORTED;
  if (total_pairs == 0 && D_total == 0) return 0;
  if (total_pairs > 0 && (P == 0 || !dt_kpts || !gt_kpts || !gt_boxes || !gt_area || !sigmas || !oks)) return DETOPS_EINVAL;
  if (D_total > 0 && (!dt_kpts || !dt_area)) return DETOPS_EINVAL;
  const int64_t pair_blocks = ceil_div64(total_pairs, kPairs), area_blocks = ceil_div64(D_total, kBlock);
  if (pair_blocks + area_blocks > 0x7fffffff) return DETOPS_EINVAL;
  hipLaunchKernelGGL(eval_oks_kernel, dim3(static_cast<unsigned>(pair_blocks + area_blocks)), dim3(kBlock), 0,
                     as_stream(stream), dt_kpts, gt_kpts, gt_boxes, gt_area, sigmas, K, dt_offset, gt_offset, iou_offset, P,
                     D_total, total_pairs, static_cast<unsigned>(pair_blocks), oks, dt_area);
  return launch_status();
}
