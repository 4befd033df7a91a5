// keypoint.hip — the keypoint head's targets, loss and decoding for gfx950 (MI355X).
//
//   detops_keypoint_targets            KeypointRCNNLossComputation.prepare_targets + keypoints_to_heat_map
//                                      (reference roi_heads/keypoint_head/loss.py:36-100, structures/keypoint.py:154-188)
//                                      for every slot of the batch in one launch
//   detops_keypoint_loss_f32           KeypointRCNNLossComputation.__call__ (loss.py:145-169): softmax cross-entropy over the
//                                      valid (ROI, keypoint) rows of the heatmap logits, value AND gradient in one pass
//                                      (a workgroup per row, or per ROI for channels-last logits), normalised by the
//                                      valid-row count counted on the device
//   detops_heatmaps_to_keypoints_f32   heatmaps_to_keypoints (roi_heads/keypoint_head/inference.py:40-94): bicubic resize of
//                                      each map to the box size, argmax and score, without materialising the resized map
//
// The reference runs the first two with two `nonzero` (device -> host syncs) and the third on the host (a copy of every
// heatmap, then cv2.resize + argmax in a Python loop over the detections).
#include <cmath>

#include "detops_dtype.h"

namespace {

constexpr int kBlock = 256;

// ---------------------------------------------------------------------------------------------------------- targets
// torch's `.floor().long()` of an fp32 value: NaN / inf / out-of-range convert to INT64_MIN (x86 cvttss2si), i.e. invalid
__device__ __forceinline__ int64_t floor_to_long(float v) {
  const float f = floorf(v);
  return (f >= -9.2e18f && f <= 9.2e18f) ? static_cast<int64_t>(f) : INT64_MIN;
}

// one thread per (slot p, keypoint k)
__global__ void __launch_bounds__(kBlock)
keypoint_targets_kernel(const float* __restrict__ boxes, const int64_t* __restrict__ matched, const int64_t* __restrict__ labels,
                        const float* __restrict__ gt_boxes, const float* __restrict__ gt_kps, int P, int G, int K, int M,
                        int64_t* __restrict__ heat, unsigned char* __restrict__ valid) {
#pragma clang fp contract(off)
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= static_cast<int64_t>(P) * K) return;
  const int p = static_cast<int>(i / K), k = static_cast<int>(i % K);
  const int64_t g = matched[p];
  bool ok = labels[p] > 0 && g >= 0 && g < G;
  if (ok) {
    // the matched ground truth has at least one labelled keypoint inside its own box (loss.py:93-98, _within_box :40-53)
    const float* gb = gt_boxes + g * 4;
    const float* kp = gt_kps + g * K * 3;
    bool any = false;
    for (int j = 0; j < K; ++j) {
      const float x = kp[3 * j], y = kp[3 * j + 1], v = kp[3 * j + 2];
      any |= (x >= gb[0]) && (x <= gb[2]) && (y >= gb[1]) && (y <= gb[3]) && (v > 0.f);
    }
    ok = any;
  }
  int64_t lin = 0;
  bool val = false;
  if (ok) {
    const float* b = boxes + static_cast<int64_t>(p) * 4;
    const float* kp = gt_kps + (g * K + k) * 3;
    const float x = kp[0], y = kp[1], v = kp[2];
    const float fm = static_cast<float>(M);
    // (x - x1) * (M / (x2 - x1)), each step one fp32 rounding (keypoint.py:158-176); the right / bottom edge maps to M - 1.
    // `M / tensor` with a Python number on the left is torch's Tensor.__rtruediv__ = reciprocal() * M: two roundings, which
    // differ from one correctly rounded division in ~1/4 of the widths (then a product on an integer floors differently)
    const float sx = (1.f / (b[2] - b[0])) * fm, sy = (1.f / (b[3] - b[1])) * fm;
    int64_t xi = floor_to_long((x - b[0]) * sx), yi = floor_to_long((y - b[1]) * sy);
    if (x == b[2]) xi = M - 1;
    if (y == b[3]) yi = M - 1;
    val = xi >= 0 && yi >= 0 && xi < M && yi < M && v > 0.f;
    lin = val ? yi * M + xi : 0;
  }
  heat[i] = lin;
  valid[i] = val ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------- loss
// One workgroup counts the valid rows once: inv_count[0] = 1 / max(#valid, 1), the normaliser without a host read
__global__ void __launch_bounds__(kBlock)
keypoint_loss_count_kernel(const unsigned char* __restrict__ valid, int n, float* __restrict__ inv_count) {
  __shared__ float s_red[kBlock / kWave];
  float c = 0.f;
  for (int i = threadIdx.x; i < n; i += kBlock) c += valid[i] ? 1.f : 0.f;
  c = block_sum<kBlock>(c, s_red);
  if (threadIdx.x == 0) inv_count[0] = 1.f / fmaxf(c, 1.f);
}

// (max, sum of exp(x - max)) pairs merged; an empty side (max = -inf) contributes nothing
__device__ __forceinline__ void lse_merge(float& m, float& s, float om, float os) {
  if (om == -INFINITY) return;
  if (m == -INFINITY) { m = om; s = os; return; }
  if (om > m) { s = s * expf(m - om) + os; m = om; }
  else s += os * expf(om - m);
}

// One workgroup per (ROI, keypoint) row r = p * K + k.  Pass 1: each thread's running (max, sum of exp) over the pixels
// t, t + kBlock, ..., merged across the wave and then the workgroup in a fixed order -> log-sum-exp.  Pass 2:
// d loss / d logits = (softmax - onehot(target)) / #valid.  An invalid row reads nothing and writes a zero gradient.
// partial[r] = the row's cross-entropy (0 when invalid).
__global__ void __launch_bounds__(kBlock)
keypoint_loss_kernel(const float* __restrict__ logits, int64_t lsP, int64_t lsK, int64_t lsH, int64_t lsW,
                     const int64_t* __restrict__ heat, const unsigned char* __restrict__ valid, int K, int H, int W,
                     const float* __restrict__ inv_count, float* __restrict__ grad, int64_t gsP, int64_t gsK, int64_t gsH,
                     int64_t gsW, float* __restrict__ partial) {
  __shared__ float s_m[kBlock / kWave], s_s[kBlock / kWave];
  __shared__ float s_lse;
  const int r = blockIdx.x;
  const int p = r / K, k = r % K;
  const int S = H * W;
  const int t = threadIdx.x;
  const int64_t tg = heat[r];
  const bool ok = valid[r] != 0 && tg >= 0 && tg < S;
  float* g = grad + p * gsP + k * gsK;
  if (!ok) {
    for (int i = t; i < S; i += kBlock) g[(i / W) * gsH + (i % W) * gsW] = 0.f;
    if (t == 0) partial[r] = 0.f;
    return;
  }
  const float* x = logits + p * lsP + k * lsK;
  float m = -INFINITY, s = 0.f;
  for (int i = t; i < S; i += kBlock) lse_merge(m, s, x[(i / W) * lsH + (i % W) * lsW], 1.f);
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const float om = __shfl_down(m, off), os = __shfl_down(s, off);
    lse_merge(m, s, om, os);
  }
  if ((t & (kWave - 1)) == 0) { s_m[t / kWave] = m; s_s[t / kWave] = s; }
  __syncthreads();
  if (t == 0) {
    float M = s_m[0], sum = s_s[0];
    for (int j = 1; j < kBlock / kWave; ++j) lse_merge(M, sum, s_m[j], s_s[j]);
    const float lse = M + logf(sum);
    s_lse = lse;
    partial[r] = lse - x[(tg / W) * lsH + (tg % W) * lsW];
  }
  __syncthreads();
  const float lse = s_lse, inv = inv_count[0];
  for (int i = t; i < S; i += kBlock) {
    const int y = i / W, xx = i % W;
    g[y * gsH + xx * gsW] = (expf(x[y * lsH + xx * lsW] - lse) - (i == tg ? 1.f : 0.f)) * inv;
  }
}

// Channels-last logits (keypoint stride 1): one workgroup per ROI p, thread t = q * K + k owns keypoint k and every Q-th
// pixel (Q = kBlock / K), so a wave reads contiguous memory — a workgroup per row would read at a stride of K floats.
// Same two passes as keypoint_loss_kernel; the partners of a keypoint are merged in thread order; partial[p * K + k].
__global__ void __launch_bounds__(kBlock)
keypoint_loss_roi_kernel(const float* __restrict__ logits, int64_t lsP, int64_t lsH, int64_t lsW,
                         const int64_t* __restrict__ heat, const unsigned char* __restrict__ valid, int K, int H, int W,
                         const float* __restrict__ inv_count, float* __restrict__ grad, int64_t gsP, int64_t gsK, int64_t gsH,
                         int64_t gsW, float* __restrict__ partial) {
  __shared__ float s_m[kBlock], s_s[kBlock];
  __shared__ float s_lse[kBlock];
  const int p = blockIdx.x;
  const int Q = kBlock / K;
  const int t = threadIdx.x;
  const bool active = t < Q * K;
  const int k = t % K, q = t / K;
  const int S = H * W;
  const int64_t r = static_cast<int64_t>(p) * K + k;
  const int64_t tg = active ? heat[r] : -1;
  const bool ok = active && valid[r] != 0 && tg >= 0 && tg < S;
  const float* x = logits + p * lsP + k;
  float m = -INFINITY, s = 0.f;
  if (ok)
    for (int i = q; i < S; i += Q) lse_merge(m, s, x[(i / W) * lsH + (i % W) * lsW], 1.f);
  s_m[t] = m;
  s_s[t] = s;
  __syncthreads();
  if (t < K) {
    float M = -INFINITY, sum = 0.f;
    for (int j = 0; j < Q; ++j) lse_merge(M, sum, s_m[j * K + t], s_s[j * K + t]);
    const float lse = M + logf(sum);
    s_lse[t] = lse;
    const int64_t rt = static_cast<int64_t>(p) * K + t;
    const int64_t tt = heat[rt];
    partial[rt] = (valid[rt] != 0 && tt >= 0 && tt < S) ? lse - x[(tt / W) * lsH + (tt % W) * lsW] : 0.f;   // t < K: k == t
  }
  __syncthreads();
  if (!active) return;
  const float lse = s_lse[k], inv = inv_count[0];
  float* g = grad + p * gsP + k * gsK;
  for (int i = q; i < S; i += Q) {
    const int y = i / W, xx = i % W;
    g[y * gsH + xx * gsW] = ok ? (expf(x[y * lsH + xx * lsW] - lse) - (i == tg ? 1.f : 0.f)) * inv : 0.f;
  }
}

// fixed-order sum of the per-row partials / max(#valid, 1)
__global__ void __launch_bounds__(kBlock)
keypoint_loss_finish_kernel(const float* __restrict__ partial, int n, const float* __restrict__ inv_count,
                            float* __restrict__ out) {
  __shared__ float s_red[kBlock / kWave];
  float v = 0.f;
  for (int i = threadIdx.x; i < n; i += kBlock) v += partial[i];
  v = block_sum<kBlock>(v, s_red);
  if (threadIdx.x == 0) out[0] = v * inv_count[0];
}

// ---------------------------------------------------------------------------------------------------------- decoding
constexpr int kMaxMap = 4096;          // heatmap pixels staged in LDS (56 x 56 = 3136)
constexpr int kMaxSide = 1 << 13;      // resized side cap (8192 px): keeps the loops bounded

// OpenCV's INTER_CUBIC taps of one output coordinate: source (d + 0.5) * (in / out) - 0.5 in double, rounded to float
// (imgproc/resize.cpp), A = -0.75 coefficients in float, tap indices clamped to the border
__device__ __forceinline__ void cubic_taps(int d, double scale, int n, int* idx, float* c) {
#pragma clang fp contract(off)
  const float f = static_cast<float>((static_cast<double>(d) + 0.5) * scale - 0.5);
  const float fl = floorf(f);
  const int s = static_cast<int>(fl);
  const float u = f - fl;
  const float A = -0.75f;
  c[0] = ((A * (u + 1.f) - 5.f * A) * (u + 1.f) + 8.f * A) * (u + 1.f) - 4.f * A;
  c[1] = ((A + 2.f) * u - (A + 3.f)) * u * u + 1.f;
  c[2] = ((A + 2.f) * (1.f - u) - (A + 3.f)) * (1.f - u) * (1.f - u) + 1.f;
  c[3] = 1.f - c[0] - c[1] - c[2];
#pragma unroll
  for (int j = 0; j < 4; ++j) idx[j] = min(max(s - 1 + j, 0), n - 1);
}

// numpy argmax order: a NaN wins (the first one), else the larger value, ties to the lower flat index
__device__ __forceinline__ bool better(float v, int64_t i, float bv, int64_t bi) {
  const bool vn = v != v, bn = bv != bv;
  if (vn || bn) return vn && (!bn || i < bi);
  return v > bv || (v == bv && i < bi);
}

// One workgroup per (detection n, keypoint k): the map in LDS, every thread walks the resized map's pixels in row-major
// order with a running (max, index), then the wave and the workgroup reduce with the lowest index winning ties.
__global__ void __launch_bounds__(kBlock)
heatmaps_to_keypoints_kernel(const float* __restrict__ maps, int64_t sN, int64_t sK, int64_t sH, int64_t sW,
                             const float* __restrict__ boxes, int K, int H, int W, float* __restrict__ kps,
                             float* __restrict__ scores) {
#pragma clang fp contract(off)
  __shared__ float s_map[kMaxMap];
  __shared__ float s_v[kBlock / kWave];
  __shared__ int64_t s_i[kBlock / kWave];
  const int n = blockIdx.x / K, k = blockIdx.x % K;
  const float* src = maps + n * sN + k * sK;
  for (int i = threadIdx.x; i < H * W; i += kBlock) s_map[i] = src[(i / W) * sH + (i % W) * sW];
  const float* b = boxes + static_cast<int64_t>(n) * 4;
  const float bw = fmaxf(b[2] - b[0], 1.f), bh = fmaxf(b[3] - b[1], 1.f);
  const float cw = ceilf(bw), ch = ceilf(bh);
  // a NaN side resizes to 1 pixel, a side beyond kMaxSide to kMaxSide (no real detection comes near either)
  const int ow = cw < static_cast<float>(kMaxSide) ? static_cast<int>(cw) : (cw == cw ? kMaxSide : 1);
  const int oh = ch < static_cast<float>(kMaxSide) ? static_cast<int>(ch) : (ch == ch ? kMaxSide : 1);
  const double scx = static_cast<double>(W) / ow, scy = static_cast<double>(H) / oh;
  __syncthreads();
  float best = -INFINITY;
  int64_t bidx = INT64_MAX;
  const int64_t total = static_cast<int64_t>(ow) * oh;
  for (int64_t i = threadIdx.x; i < total; i += kBlock) {
    const int oy = static_cast<int>(i / ow), ox = static_cast<int>(i % ow);
    int xi[4], yi[4];
    float cx[4], cy[4];
    cubic_taps(ox, scx, W, xi, cx);
    cubic_taps(oy, scy, H, yi, cy);
    float h[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {          // horizontal pass over the four source rows, then the vertical pass
      const float* row = s_map + yi[j] * W;
      h[j] = ((cx[0] * row[xi[0]] + cx[1] * row[xi[1]]) + cx[2] * row[xi[2]]) + cx[3] * row[xi[3]];
    }
    const float v = ((cy[0] * h[0] + cy[1] * h[1]) + cy[2] * h[2]) + cy[3] * h[3];
    if (better(v, i, best, bidx)) { best = v; bidx = i; }
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const float ov = __shfl_down(best, off);
    const int64_t oi = __shfl_down(bidx, off);
    if (better(ov, oi, best, bidx)) { best = ov; bidx = oi; }
  }
  if ((threadIdx.x & (kWave - 1)) == 0) { s_v[threadIdx.x / kWave] = best; s_i[threadIdx.x / kWave] = bidx; }
  __syncthreads();
  if (threadIdx.x != 0) return;
  best = s_v[0];
  bidx = s_i[0];
  for (int j = 1; j < kBlock / kWave; ++j)
    if (better(s_v[j], s_i[j], best, bidx)) { best = s_v[j]; bidx = s_i[j]; }
  if (bidx == INT64_MAX) bidx = 0;   // every value -inf: numpy's argmax is 0
  const int64_t xint = bidx % ow, yint = bidx / ow;
  // (x_int + 0.5) * width_correction + x1: numpy evaluates it in float64 with the float32 correction w / ceil(w)
  // (inference.py:75-88), the result is stored as float32
  const double wcorr = static_cast<double>(bw / cw), hcorr = static_cast<double>(bh / ch);
  const double x = (static_cast<double>(xint) + 0.5) * wcorr + static_cast<double>(b[0]);
  const double y = (static_cast<double>(yint) + 0.5) * hcorr + static_cast<double>(b[1]);
  float* o = kps + (static_cast<int64_t>(n) * K + k) * 3;
  o[0] = static_cast<float>(x);
  o[1] = static_cast<float>(y);
  o[2] = 1.f;
  scores[static_cast<int64_t>(n) * K + k] = best;
}

}  // namespace

DETOPS_API int detops_keypoint_targets(const float* boxes, const int64_t* matched, const int64_t* labels, const float* gt_boxes,
                                       const float* gt_keypoints, int P, int G, int K, int M, int64_t* heatmaps,
                                       unsigned char* valid, detops_stream_t stream) {
  if (P < 0 || G < 0 || K <= 0 || M <= 0 || static_cast<int64_t>(M) * M > INT32_MAX) return DETOPS_EINVAL;
  if (P == 0) return 0;
  if (!boxes || !matched || !labels || !heatmaps || !valid || (G > 0 && (!gt_boxes || !gt_keypoints))) return DETOPS_EINVAL;
  const int64_t n = static_cast<int64_t>(P) * K;
  hipLaunchKernelGGL(keypoint_targets_kernel, dim3(static_cast<unsigned>(ceil_div64(n, kBlock))), dim3(kBlock), 0,
                     as_stream(stream), boxes, matched, labels, gt_boxes, gt_keypoints, P, G, K, M, heatmaps, valid);
  return launch_status();
}

DETOPS_API size_t detops_keypoint_loss_workspace_bytes(int P, int K) {
  return (P <= 0 || K <= 0) ? 0 : (static_cast<size_t>(P) * K + 1) * sizeof(float);
}

DETOPS_API int detops_keypoint_loss_f32(const float* logits, const int64_t* logit_strides, const int64_t* heatmaps,
                                        const unsigned char* valid, int P, int K, int H, int W, float* grad_logits,
                                        const int64_t* grad_strides, float* loss1, void* workspace, size_t workspace_bytes,
                                        detops_stream_t stream) {
  if (P <= 0 || K <= 0 || H <= 0 || W <= 0 || static_cast<int64_t>(P) * K > INT32_MAX ||
      static_cast<int64_t>(H) * W > INT32_MAX)
    return DETOPS_EINVAL;
  if (!logits || !logit_strides || !heatmaps || !valid || !grad_logits || !grad_strides || !loss1 || !workspace ||
      workspace_bytes < detops_keypoint_loss_workspace_bytes(P, K))
    return DETOPS_EINVAL;
  const int64_t* ls = logit_strides;
  const int64_t* gs = grad_strides;
  const int rows = P * K;
  hipStream_t st = as_stream(stream);
  float* inv_count = static_cast<float*>(workspace);
  float* partial = inv_count + 1;
  hipLaunchKernelGGL(keypoint_loss_count_kernel, dim3(1), dim3(kBlock), 0, st, valid, rows, inv_count);
  if (ls[1] == 1 && K <= kBlock)
    hipLaunchKernelGGL(keypoint_loss_roi_kernel, dim3(P), dim3(kBlock), 0, st, logits, ls[0], ls[2], ls[3], heatmaps, valid, K, H,
                       W, inv_count, grad_logits, gs[0], gs[1], gs[2], gs[3], partial);
  else
    hipLaunchKernelGGL(keypoint_loss_kernel, dim3(rows), dim3(kBlock), 0, st, logits, ls[0], ls[1], ls[2], ls[3], heatmaps,
                       valid, K, H, W, inv_count, grad_logits, gs[0], gs[1], gs[2], gs[3], partial);
  hipLaunchKernelGGL(keypoint_loss_finish_kernel, dim3(1), dim3(kBlock), 0, st, partial, rows, inv_count, loss1);
  return launch_status();
}

DETOPS_API int detops_heatmaps_to_keypoints_f32(const float* heatmaps, const int64_t* strides, const float* boxes, int N, int K,
                                                int H, int W, float* keypoints, float* scores, detops_stream_t stream) {
  if (N < 0 || K <= 0 || H <= 0 || W <= 0 || H * W > kMaxMap || static_cast<int64_t>(N) * K > INT32_MAX) return DETOPS_EINVAL;
  if (N == 0) return 0;
  if (!heatmaps || !strides || !boxes || !keypoints || !scores) return DETOPS_EINVAL;
  hipLaunchKernelGGL(heatmaps_to_keypoints_kernel, dim3(N * K), dim3(kBlock), 0, as_stream(stream), heatmaps, strides[0],
                     strides[1], strides[2], strides[3], boxes, K, H, W, keypoints, scores);
  return launch_status();
}
