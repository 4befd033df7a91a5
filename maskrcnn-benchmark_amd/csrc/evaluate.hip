// evaluate.hip — detection evaluation on the device, for gfx950 (MI355X).  The arithmetic is stated in include/detops.h
// ("Detection evaluation"); maskrcnn_benchmark/_eval_cpu.py is the same four steps in numpy.
//
//   detops_mask_pack          uint8 planes -> bit rows (a wave's __ballot over 64 consecutive pixels of a row is one word),
//                             the planes' set-pixel counts and tight extents
//   detops_mask_pack_rle      the same results straight from uncompressed RLE runs, no plane stored
//   detops_mask_pair_counts   popcount(AND) over the intersection of two planes' extents, one wave per pair
//   detops_eval_iou           counts or boxes -> the fp64 IoU matrix of every problem (COCO segm / COCO bbox / VOC)
//   detops_eval_match         greedy matching, one wave per problem (COCO: a lane per (area range, threshold); VOC)
//
// A problem is the detections and the ground truths of one (image, category) pair.  dt_offset / gt_offset [P + 1] delimit
// its rows and columns, iou_offset [P + 1] (int64) its D_p x G_p row-major matrix; a flat pair index finds its problem by
// bisection of iou_offset (eval_problem.h, shared with eval_oks.hip).  The caller sizes every array from the same offsets;
// a pair index outside its problem's matrix (inconsistent offsets) writes 0 and reads nothing.
#include "eval_problem.h"

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr int kPackUnroll = 4;        // words of a plane a wave has in flight
constexpr int kPackItems = 32;        // words per wave the grid of detops_mask_pack is sized for
constexpr int kMaxGt = DETOPS_EVAL_MAX_GT;

// ---------------------------------------------------------------------------------------------------- pack
__global__ void mask_pack_init_kernel(const int32_t* __restrict__ plane_hw, int N, int32_t* __restrict__ area,
                                      int32_t* __restrict__ extent) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const int H = max(plane_hw[2 * n], 0), W = max(plane_hw[2 * n + 1], 0);
  area[n] = 0;
  extent[4 * n + 0] = H;              // first row, last row, first word column, last word column: empty until a pixel is found
  extent[4 * n + 1] = -1;
  extent[4 * n + 2] = (W + 63) / 64;
  extent[4 * n + 3] = -1;
}

// Workgroup (x, plane): its waves share the plane's words, word i = (row i / WW, word column i % WW), neighbouring waves
// on neighbouring words.  A lane holds one pixel; lanes at or beyond W vote 0.
__global__ void __launch_bounds__(kBlock)
mask_pack_kernel(const unsigned char* __restrict__ planes, const int64_t* __restrict__ plane_offset,
                 const int32_t* __restrict__ plane_hw, int plane_base, const int64_t* __restrict__ word_offset,
                 detops_u64* __restrict__ words, int32_t* __restrict__ area, int32_t* __restrict__ extent) {
  const int n = plane_base + blockIdx.y;
  const int H = plane_hw[2 * n], W = plane_hw[2 * n + 1];
  if (H <= 0 || W <= 0) return;
  const int WW = (W + 63) / 64;
  const int64_t items = static_cast<int64_t>(H) * WW;
  const unsigned char* src = planes + plane_offset[n];
  detops_u64* dst = words + word_offset[n];
  const int lane = threadIdx.x % kWave;
  const int64_t nwaves = static_cast<int64_t>(gridDim.x) * kWaves;
  int count = 0, rmin = H, rmax = -1, cmin = WW, cmax = -1;
  for (int64_t i0 = static_cast<int64_t>(blockIdx.x) * kWaves + threadIdx.x / kWave; i0 < items; i0 += nwaves * kPackUnroll) {
    unsigned char v[kPackUnroll];
#pragma unroll
    for (int k = 0; k < kPackUnroll; ++k) {
      const int64_t i = i0 + k * nwaves;
      v[k] = 0;
      if (i < items) {
        const int r = static_cast<int>(i / WW), col = static_cast<int>(i % WW) * 64 + lane;
        if (col < W) v[k] = src[static_cast<int64_t>(r) * W + col];
      }
    }
#pragma unroll
    for (int k = 0; k < kPackUnroll; ++k) {
      const int64_t i = i0 + k * nwaves;
      const detops_u64 word = __ballot(v[k] != 0);
      if (i < items) {                           // wave-uniform
        if (word) {
          const int r = static_cast<int>(i / WW), c = static_cast<int>(i % WW);
          count += __popcll(word);
          rmin = min(rmin, r); rmax = max(rmax, r);
          cmin = min(cmin, c); cmax = max(cmax, c);
        }
        if (lane == 0) dst[i] = word;
      }
    }
  }
  if (lane == 0 && count > 0) {                  // integer atomics: the result does not depend on their order
    atomicAdd(&area[n], count);
    atomicMin(&extent[4 * n + 0], rmin);
    atomicMax(&extent[4 * n + 1], rmax);
    atomicMin(&extent[4 * n + 2], cmin);
    atomicMax(&extent[4 * n + 3], cmax);
  }
}

// ---------------------------------------------------------------------------------------------------- pack from runs
// detops_mask_pack_rle: uncompressed RLE (column-major runs starting with a 0-run) straight to the results of the pack
// above; no plane is ever stored.
//   1. start[i] = sum of the runs in front of run i of the FLAT run array (block_scan inside a chunk, scan_tiles over the
//      chunks); a run's first position inside its mask is start[i] - start[run_offset[n]].
//   2. A workgroup owns one mask and one strip of 64 columns at a time.  The strip lives in LDS as a COLUMN-major bit
//      array, ceil(H / 64) words per column (padded to an odd number of words: the 32 lanes of a half wave then read 32
//      different bank pairs).  A thread owns whole words of it: it finds the run that holds its word's first position by
//      bisection of `start` and walks the runs that overlap the word — every LDS word is written once, by one thread.
//   3. A wave turns 64 rows x 64 columns around with 64 ballots (lane = column, the trick of mask_pack_kernel), counts
//      the pixels and narrows the extents on the way; lane b stores row 64 r + b's word.
// Integer atomics only where mask_pack_kernel has them: one add and four min / max per wave that saw a pixel.
constexpr int kRunPer = 8;                                    // consecutive runs of a thread of the scan
constexpr int kRunChunk = kBlock * kRunPer;
constexpr int kPackRleMaxH = DETOPS_MASK_PACK_RLE_MAX_H;
constexpr int kColWords = (kPackRleMaxH / 64) | 1;                // words of a column in LDS at most (odd)
static_assert(kPackRleMaxH % 64 == 0 && 64 * kColWords * 8 <= 64 * 1024, "the strip fits the static LDS of a workgroup");

__device__ __forceinline__ int64_t run_at(const int32_t* __restrict__ counts, int64_t i, int64_t total) {
  const int c = i < total ? counts[i] : 0;
  return c < 0 ? 0 : c;                                    // a negative run (malformed input) counts as empty
}

__global__ void __launch_bounds__(kBlock)
run_chunk_sums_kernel(const int32_t* __restrict__ counts, int64_t total, int64_t* __restrict__ chunk_sum) {
  __shared__ int64_t wave_tot[kWaves];
  const int64_t i0 = static_cast<int64_t>(blockIdx.x) * kRunChunk + static_cast<int64_t>(threadIdx.x) * kRunPer;
  int64_t s = 0;
#pragma unroll
  for (int j = 0; j < kRunPer; ++j) s += run_at(counts, i0 + j, total);
  int64_t all;
  block_scan<kBlock>(s, wave_tot, all);
  if (threadIdx.x == 0) chunk_sum[blockIdx.x] = all;
}

__global__ void __launch_bounds__(kBlock) run_chunk_offsets_kernel(int64_t nchunks, int64_t* __restrict__ chunk_sum) {
  __shared__ int64_t wave_tot[kWaves];
  scan_tiles<kBlock>(
      nchunks, [&](int64_t b) { return chunk_sum[b]; }, [&](int64_t b, int64_t before) { chunk_sum[b] = before; }, wave_tot);
}

__global__ void __launch_bounds__(kBlock)
run_starts_kernel(const int32_t* __restrict__ counts, int64_t total, const int64_t* __restrict__ chunk_base,
                  int64_t* __restrict__ start) {
  __shared__ int64_t wave_tot[kWaves];
  const int64_t i0 = static_cast<int64_t>(blockIdx.x) * kRunChunk + static_cast<int64_t>(threadIdx.x) * kRunPer;
  int64_t c[kRunPer], s = 0;
#pragma unroll
  for (int j = 0; j < kRunPer; ++j) s += c[j] = run_at(counts, i0 + j, total);
  int64_t all;
  int64_t at = chunk_base[blockIdx.x] + block_scan<kBlock>(s, wave_tot, all) - s;
#pragma unroll
  for (int j = 0; j < kRunPer; ++j) {
    if (i0 + j < total) start[i0 + j] = at;
    at += c[j];
  }
}

// bits [a, b) of a word, 0 <= a < b <= 64
__device__ __forceinline__ detops_u64 bit_range(int a, int b) {
  return (b >= 64 ? ~0ull : (1ull << b) - 1) & ~((1ull << a) - 1);
}

__global__ void __launch_bounds__(kBlock)
mask_pack_rle_kernel(const int32_t* __restrict__ counts, const int64_t* __restrict__ run_offset,
                     const int64_t* __restrict__ start, int64_t total, const int32_t* __restrict__ plane_hw, int plane_base,
                     const int64_t* __restrict__ word_offset, detops_u64* __restrict__ words, int32_t* __restrict__ area,
                     int32_t* __restrict__ extent) {
  __shared__ detops_u64 col[64 * kColWords];
  const int n = plane_base + blockIdx.y;
  const int H = plane_hw[2 * n], W = plane_hw[2 * n + 1];
  if (H <= 0 || W <= 0 || H > kPackRleMaxH) return;     // (the entry point refuses a call with a taller plane)
  const int WW = (W + 63) / 64, HW = (H + 63) / 64, HWp = HW | 1;
  int64_t r0 = run_offset[n], r1 = run_offset[n + 1];
  r0 = r0 < 0 ? 0 : (r0 > total ? total : r0);
  r1 = r1 < r0 ? r0 : (r1 > total ? total : r1);
  const int nr = static_cast<int>(r1 - r0 > INT32_MAX ? INT32_MAX : r1 - r0);
  const int64_t* st = start + r0;
  const int32_t* rc = counts + r0;
  const int64_t base = nr ? st[0] : 0;
  detops_u64* dst = words + word_offset[n];
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  int count = 0, rmin = H, rmax = -1, cmin = WW, cmax = -1;
  for (int s = blockIdx.x; s < WW; s += gridDim.x) {
    const int x0 = s * 64, ncol = min(64, W - x0);
    for (int idx = threadIdx.x; idx < ncol * HW; idx += kBlock) {
      const int c = idx / HW, r = idx % HW;
      const int64_t lo = static_cast<int64_t>(x0 + c) * H + r * 64;        // positions of the mask this word holds
      const int64_t hi = lo + min(64, H - r * 64);
      detops_u64 word = 0;
      if (nr) {
        for (int j = last_at_or_below(st, nr, base + lo); j < nr; ++j) {
          const int64_t a = st[j] - base;
          if (a >= hi) break;
          const int64_t b = a + (rc[j] < 0 ? 0 : rc[j]);
          if ((j & 1) && b > lo && b > a)
            word |= bit_range(static_cast<int>((a < lo ? lo : a) - lo), static_cast<int>((b > hi ? hi : b) - lo));
        }
      }
      col[c * HWp + r] = word;
    }
    __syncthreads();
    for (int r = wave; r < HW; r += kWaves) {
      const detops_u64 v = lane < ncol ? col[lane * HWp + r] : 0;
      detops_u64 mine = 0;
#pragma unroll 8
      for (int b = 0; b < 64; ++b) {
        const detops_u64 word = __ballot((v >> b) & 1);                     // row 64 r + b of the strip
        if (word) {                                                        // wave-uniform
          count += __popcll(word);
          rmin = min(rmin, r * 64 + b);
          rmax = max(rmax, r * 64 + b);
          cmin = min(cmin, s);
          cmax = max(cmax, s);
        }
        if (lane == b) mine = word;
      }
      const int y = r * 64 + lane;
      if (y < H) dst[static_cast<int64_t>(y) * WW + s] = mine;
    }
    __syncthreads();
  }
  if (lane == 0 && count > 0) {                    // integer atomics: the result does not depend on their order
    atomicAdd(&area[n], count);
    atomicMin(&extent[4 * n + 0], rmin);
    atomicMax(&extent[4 * n + 1], rmax);
    atomicMin(&extent[4 * n + 2], cmin);
    atomicMax(&extent[4 * n + 3], cmax);
  }
}

int64_t run_chunks_of(int64_t total) { return (total + kRunChunk - 1) / kRunChunk; }

// ---------------------------------------------------------------------------------------------------- pair counts
// One wave per pair.  The words of the two planes inside the intersection of their extents, 64 per step.
__global__ void __launch_bounds__(kBlock)
mask_pair_counts_kernel(const detops_u64* __restrict__ dt_words, const int64_t* __restrict__ dt_word_offset,
                        const int32_t* __restrict__ dt_hw, const int32_t* __restrict__ dt_extent,
                        const detops_u64* __restrict__ gt_words, const int64_t* __restrict__ gt_word_offset,
                        const int32_t* __restrict__ gt_hw, const int32_t* __restrict__ gt_extent,
                        const int32_t* __restrict__ dt_offset, const int32_t* __restrict__ gt_offset,
                        const int64_t* __restrict__ iou_offset, int P, int64_t total_pairs, int32_t* __restrict__ counts) {
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kWaves + threadIdx.x / kWave;
  if (idx >= total_pairs) return;
  const int lane = threadIdx.x % kWave;
  const Pair pr = pair_of(dt_offset, gt_offset, iou_offset, P, idx);
  int result = 0;
  if (pr.p >= 0) {
    const int H = dt_hw[2 * pr.d], W = dt_hw[2 * pr.d + 1];
    if (H != gt_hw[2 * pr.g] || W != gt_hw[2 * pr.g + 1]) {
      result = -1;                               // planes of different images: no answer, nothing read
    } else {
      const int r0 = max(max(dt_extent[4 * pr.d + 0], gt_extent[4 * pr.g + 0]), 0);
      const int r1 = min(min(dt_extent[4 * pr.d + 1], gt_extent[4 * pr.g + 1]), H - 1);
      const int c0 = max(max(dt_extent[4 * pr.d + 2], gt_extent[4 * pr.g + 2]), 0);
      const int c1 = min(min(dt_extent[4 * pr.d + 3], gt_extent[4 * pr.g + 3]), (W + 63) / 64 - 1);
      if (r0 <= r1 && c0 <= c1) {                // disjoint extents: no memory traffic
        const int WW = (W + 63) / 64, nw = c1 - c0 + 1;
        const int64_t items = static_cast<int64_t>(r1 - r0 + 1) * nw;
        const detops_u64* a = dt_words + dt_word_offset[pr.d];
        const detops_u64* b = gt_words + gt_word_offset[pr.g];
        int acc = 0;
        for (int64_t i = lane; i < items; i += kWave) {
          const int64_t w = static_cast<int64_t>(r0 + i / nw) * WW + c0 + i % nw;
          acc += __popcll(a[w] & b[w]);
        }
        result = wave_sum(acc);               // (valid in lane 0, the lane that writes)
      }
    }
  }
  if (lane == 0) counts[idx] = result;
}

// ---------------------------------------------------------------------------------------------------- IoU
__device__ __forceinline__ double iou_coco_bbox(const float* __restrict__ d, const float* __restrict__ g, bool crowd) {
#pragma clang fp contract(off)
  // BoxList.convert("xywh") in fp32
  float dw = d[2] - d[0]; dw = dw + 1.0f;
  float dh = d[3] - d[1]; dh = dh + 1.0f;
  float gw = g[2] - g[0]; gw = gw + 1.0f;
  float gh = g[3] - g[1]; gh = gh + 1.0f;
  const double dx = d[0], dy = d[1], gx = g[0], gy = g[1];
  const double DW = dw, DH = dh, GW = gw, GH = gh;
  const double da = DW * DH, ga = GW * GH;
  const double iw = fmin(dx + DW, gx + GW) - fmax(dx, gx);
  const double ih = fmin(dy + DH, gy + GH) - fmax(dy, gy);
  if (!(iw > 0.0) || !(ih > 0.0)) return 0.0;
  const double i = iw * ih;
  double u = da + ga;
  u = u - i;
  if (crowd) u = da;
  return u > 0.0 ? i / u : 0.0;
}

__device__ __forceinline__ double iou_voc(const float* __restrict__ d, const float* __restrict__ g) {
#pragma clang fp contract(off)
  const float dx2 = d[2] + 1.0f, dy2 = d[3] + 1.0f, gx2 = g[2] + 1.0f, gy2 = g[3] + 1.0f;   // the evaluation's own + 1
  float aw = dx2 - d[0]; aw = aw + 1.0f;
  float ah = dy2 - d[1]; ah = ah + 1.0f;
  float bw = gx2 - g[0]; bw = bw + 1.0f;
  float bh = gy2 - g[1]; bh = bh + 1.0f;
  const float area_d = aw * ah, area_g = bw * bh;
  float w = fminf(dx2, gx2) - fmaxf(d[0], g[0]); w = w + 1.0f; w = fmaxf(w, 0.0f);
  float h = fminf(dy2, gy2) - fmaxf(d[1], g[1]); h = h + 1.0f; h = fmaxf(h, 0.0f);
  const float inter = w * h;
  float u = area_d + area_g;
  u = u - inter;
  if (!(u != 0.0f)) return 0.0;
  // the fp32 quotient: the fp64 quotient of two fp32 values rounds to it (53 >= 2 * 24 + 2 bits)
  const float q = static_cast<float>(static_cast<double>(inter) / static_cast<double>(u));
  return static_cast<double>(q);
}

__global__ void __launch_bounds__(kBlock)
eval_iou_kernel(int mode, const int32_t* __restrict__ counts, const int32_t* __restrict__ dt_area,
                const int32_t* __restrict__ gt_area, const float* __restrict__ dt_boxes, const float* __restrict__ gt_boxes,
                const unsigned char* __restrict__ gt_crowd, const int32_t* __restrict__ dt_offset,
                const int32_t* __restrict__ gt_offset, const int64_t* __restrict__ iou_offset, int P, int64_t total_pairs,
                double* __restrict__ iou) {
#pragma clang fp contract(off)
  const int64_t idx = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (idx >= total_pairs) return;
  const Pair pr = pair_of(dt_offset, gt_offset, iou_offset, P, idx);
  double v = 0.0;
  if (pr.p >= 0) {
    const bool crowd = gt_crowd != nullptr && gt_crowd[pr.g] != 0;
    if (mode == DETOPS_EVAL_COCO_SEGM) {
      const double i = static_cast<double>(counts[idx]);
      const double da = static_cast<double>(dt_area[pr.d]), ga = static_cast<double>(gt_area[pr.g]);
      double u = da + ga;
      u = u - i;
      if (crowd) u = da;
      v = (i > 0.0 && u > 0.0) ? i / u : 0.0;
    } else if (mode == DETOPS_EVAL_COCO_BBOX) {
      v = iou_coco_bbox(dt_boxes + 4 * static_cast<int64_t>(pr.d), gt_boxes + 4 * static_cast<int64_t>(pr.g), crowd);
    } else {
      v = iou_voc(dt_boxes + 4 * static_cast<int64_t>(pr.d), gt_boxes + 4 * static_cast<int64_t>(pr.g));
    }
  }
  iou[idx] = v;
}

// ---------------------------------------------------------------------------------------------------- match
// COCO.  A lane is an (area range a, threshold t) pair; every lane walks the ground truths in INPUT order, so IoU[d, g],
// the ground truth's area and its crowd flag are one address for the whole wave.  The definition's order (the
// non-ignored ones first, then the ignored ones, and a stop at the first ignored one once a non-ignored match is held)
// is kept by carrying two candidates, the best non-ignored and the best ignored one, each starting at the threshold:
// the second is what the definition's walk finds exactly when the first stays empty.
template <bool kLds>
__device__ __forceinline__ void coco_match_lane(const double* __restrict__ iou, int d0, int D, int g0, int G, int64_t D_total,
                                                const double* __restrict__ dt_area, const double* __restrict__ gt_area,
                                                const unsigned char* __restrict__ gt_crowd, double thr, double lo, double hi,
                                                bool active, int64_t out_row, detops_u64* taken_lds,
                                                int32_t* __restrict__ dt_match, unsigned char* __restrict__ dt_ignore) {
  const int lane = threadIdx.x;
  const int nwords = (G + 63) / 64;
  detops_u64 taken_reg = 0;
  if (kLds)
    for (int w = 0; w < nwords; ++w) taken_lds[w * kWave + lane] = 0;
  if (!active) return;
  for (int d = 0; d < D; ++d) {
    const double* row = iou + static_cast<int64_t>(d) * G;
    double best_n = thr, best_i = thr;
    int m_n = -1, m_i = -1;
    for (int g = 0; g < G; ++g) {
      const bool crowd = gt_crowd[g0 + g] != 0;
      const double ga = gt_area[g0 + g];
      const double v = row[g];
      const bool ign = crowd || ga < lo || ga > hi;
      const detops_u64 word = kLds ? taken_lds[(g >> 6) * kWave + lane] : taken_reg;
      if (((word >> (g & 63)) & 1) && !crowd) continue;
      if (ign) {
        if (!(v < best_i)) { best_i = v; m_i = g; }
      } else {
        if (!(v < best_n)) { best_n = v; m_n = g; }
      }
    }
    const int m = m_n >= 0 ? m_n : m_i;
    unsigned char ig;
    if (m >= 0) {
      ig = m_n >= 0 ? 0 : 1;
      if (kLds) taken_lds[(m >> 6) * kWave + lane] |= 1ull << (m & 63);
      else taken_reg |= 1ull << (m & 63);
    } else {
      const double a = dt_area[d0 + d];
      ig = (a < lo || a > hi) ? 1 : 0;
    }
    dt_match[out_row * D_total + d0 + d] = m;
    dt_ignore[out_row * D_total + d0 + d] = ig;
  }
}

// One wave per problem (workgroup = one wave).  Dynamic LDS: the lanes' taken sets when some G_p > 64.
__global__ void __launch_bounds__(kWave)
eval_match_coco_kernel(const double* __restrict__ iou, const int32_t* __restrict__ dt_offset,
                       const int32_t* __restrict__ gt_offset, const int64_t* __restrict__ iou_offset, int P,
                       int64_t D_total, int64_t G_total,
                       const double* __restrict__ dt_area, const double* __restrict__ gt_area,
                       const unsigned char* __restrict__ gt_crowd, const double* __restrict__ iou_thrs, int T,
                       const double* __restrict__ area_rngs, int A, int lds_words, int32_t* __restrict__ dt_match,
                       unsigned char* __restrict__ dt_ignore, unsigned char* __restrict__ gt_ignore) {
  DETOPS_DYNAMIC_LDS(detops_u64, taken);
  const int p = blockIdx.x, lane = threadIdx.x;
  const int d0 = dt_offset[p], g0 = gt_offset[p];
  const int D = dt_offset[p + 1] - d0, G = gt_offset[p + 1] - g0;
  if (d0 < 0 || g0 < 0 || D < 0 || G < 0 || d0 + D > D_total || g0 + G > G_total) return;
  if (G > kMaxGt || (G > 64 && (G + 63) / 64 > lds_words)) return;       // the entry point reports DETOPS_EGTCAP
  const double* mat = iou + iou_offset[p];
  for (int base = 0; base < A * T; base += kWave) {
    const int id = base + lane;
    const bool active = id < A * T;
    const int a = active ? id / T : 0, t = active ? id % T : 0;
    const double lo = area_rngs[2 * a], hi = area_rngs[2 * a + 1];
    const double thr = fmin(iou_thrs[t], 1.0 - 1e-10);
    if (active && t == 0)
      for (int g = 0; g < G; ++g) {
        const double ga = gt_area[g0 + g];
        gt_ignore[a * G_total + g0 + g] = (gt_crowd[g0 + g] != 0 || ga < lo || ga > hi) ? 1 : 0;
      }
    if (G <= 64)
      coco_match_lane<false>(mat, d0, D, g0, G, D_total, dt_area, gt_area, gt_crowd, thr, lo, hi, active, id, taken, dt_match,
                             dt_ignore);
    else
      coco_match_lane<true>(mat, d0, D, g0, G, D_total, dt_area, gt_area, gt_crowd, thr, lo, hi, active, id, taken, dt_match,
                            dt_ignore);
  }
}

// VOC.  The lanes share the row's argmax (the first maximum); lane 0 keeps the selected flags (a byte per ground truth in LDS).
__global__ void __launch_bounds__(kWave)
eval_match_voc_kernel(const double* __restrict__ iou, const int32_t* __restrict__ dt_offset,
                      const int32_t* __restrict__ gt_offset, const int64_t* __restrict__ iou_offset, int P,
                      int64_t D_total, int64_t G_total,
                      const unsigned char* __restrict__ gt_difficult, const double* __restrict__ iou_thrs, int lds_bytes,
                      signed char* __restrict__ match) {
  DETOPS_DYNAMIC_LDS(unsigned char, selected);
  const int p = blockIdx.x, lane = threadIdx.x;
  const int d0 = dt_offset[p], g0 = gt_offset[p];
  const int D = dt_offset[p + 1] - d0, G = gt_offset[p + 1] - g0;
  if (d0 < 0 || g0 < 0 || D < 0 || G < 0 || d0 + D > D_total || g0 + G > G_total) return;
  if (G > kMaxGt || G > lds_bytes) return;
  const double thresh = iou_thrs[0];
  const double* mat = iou + iou_offset[p];
  for (int g = lane; g < G; g += kWave) selected[g] = 0;
  DETOPS_WAVE_SYNC();
  for (int d = 0; d < D; ++d) {
    const double* row = mat + static_cast<int64_t>(d) * G;
    double best = -1.0;
    int arg = 0x7fffffff;
    for (int g = lane; g < G; g += kWave) {
      const double v = row[g];
      if (v > best) { best = v; arg = g; }
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
      const double ob = __shfl_down(best, off);
      const int oa = __shfl_down(arg, off);
      if (ob > best || (ob == best && oa < arg)) { best = ob; arg = oa; }
    }
    if (lane == 0) {
      signed char m = 0;
      if (arg < G && !(best < thresh)) {
        if (gt_difficult[g0 + arg] != 0) m = -1;
        else m = selected[arg] ? 0 : 1;
        selected[arg] = 1;
      }
      match[d0 + d] = m;
    }
  }
}

}  // namespace

DETOPS_API int detops_mask_pack(const unsigned char* planes, const int64_t* plane_offset, const int32_t* plane_hw, int N,
                                int64_t max_words, const int64_t* word_offset, uint64_t* words, int32_t* area,
                                int32_t* extent, detops_stream_t stream) {
  if (N < 0 || max_words < 0) return DETOPS_EINVAL;
  if (N == 0) return 0;
  if (!plane_offset || !plane_hw || !word_offset || !area || !extent || (max_words > 0 && (!planes || !words)))
    return DETOPS_EINVAL;
  hipLaunchKernelGGL(mask_pack_init_kernel, dim3(static_cast<unsigned>((N + kBlock - 1) / kBlock)), dim3(kBlock), 0,
                     as_stream(stream), plane_hw, N, area, extent);
  if (max_words == 0) return launch_status();
  int64_t gx = ceil_div64(max_words, static_cast<int64_t>(kWaves) * kPackItems);
  gx = gx < 1 ? 1 : (gx > 4096 ? 4096 : gx);
  for (int base = 0; base < N; base += 65535) {
    const int ny = N - base < 65535 ? N - base : 65535;
    hipLaunchKernelGGL(mask_pack_kernel, dim3(static_cast<unsigned>(gx), static_cast<unsigned>(ny)), dim3(kBlock), 0,
                       as_stream(stream), planes, plane_offset, plane_hw, base, word_offset,
                       reinterpret_cast<detops_u64*>(words), area, extent);
  }
  return launch_status();
}

DETOPS_API size_t detops_mask_pack_rle_workspace_bytes(int64_t total) {
  if (total <= 0) return 0;
  return static_cast<size_t>(total + run_chunks_of(total)) * sizeof(int64_t);
}

DETOPS_API int detops_mask_pack_rle(const int32_t* counts, const int64_t* run_offset, int64_t total, const int32_t* plane_hw,
                                    int N, int max_h, int max_w, const int64_t* word_offset, uint64_t* words, int32_t* area,
                                    int32_t* extent, void* workspace, size_t workspace_bytes, detops_stream_t stream) {
  if (N < 0 || total < 0 || max_h < 0 || max_w < 0 || run_chunks_of(total) > INT32_MAX) return DETOPS_EINVAL;
  if (N == 0) return 0;
  if (max_h > kPackRleMaxH) return DETOPS_EUNSUPPORTED;
  const bool pixels = max_h > 0 && max_w > 0;
  if (!run_offset || !plane_hw || !word_offset || !area || !extent || (pixels && !words) ||
      (total > 0 && (!counts || !workspace)))
    return DETOPS_EINVAL;
  if (workspace_bytes < detops_mask_pack_rle_workspace_bytes(total)) return DETOPS_EWORKSPACE;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(mask_pack_init_kernel, dim3(static_cast<unsigned>((N + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                     plane_hw, N, area, extent);
  if (!pixels) return launch_status();
  int64_t* start = static_cast<int64_t*>(workspace);
  if (total > 0) {
    const int64_t nchunks = run_chunks_of(total);
    int64_t* chunk_sum = start + total;
    const dim3 grid(static_cast<unsigned>(nchunks));
    hipLaunchKernelGGL(run_chunk_sums_kernel, grid, dim3(kBlock), 0, st, counts, total, chunk_sum);
    hipLaunchKernelGGL(run_chunk_offsets_kernel, dim3(1), dim3(kBlock), 0, st, nchunks, chunk_sum);
    hipLaunchKernelGGL(run_starts_kernel, grid, dim3(kBlock), 0, st, counts, total, chunk_sum, start);
  }
  const int strips = (max_w + 63) / 64;
  const unsigned gx = static_cast<unsigned>(strips < 1 ? 1 : (strips > 4096 ? 4096 : strips));
  for (int base = 0; base < N; base += 65535) {
    const int ny = N - base < 65535 ? N - base : 65535;
    hipLaunchKernelGGL(mask_pack_rle_kernel, dim3(gx, static_cast<unsigned>(ny)), dim3(kBlock), 0, st, counts, run_offset,
                       start, total, plane_hw, base, word_offset, reinterpret_cast<detops_u64*>(words), area, extent);
  }
  return launch_status();
}

DETOPS_API int detops_mask_pair_counts(const uint64_t* dt_words, const int64_t* dt_word_offset, const int32_t* dt_hw,
                                       const int32_t* dt_extent, const uint64_t* gt_words, const int64_t* gt_word_offset,
                                       const int32_t* gt_hw, const int32_t* gt_extent, const int32_t* dt_offset,
                                       const int32_t* gt_offset, const int64_t* iou_offset, int P, int64_t total_pairs,
                                       int32_t* counts, detops_stream_t stream) {
  if (total_pairs < 0 || bad_problem_args(dt_offset, gt_offset, iou_offset, P)) return DETOPS_EINVAL;
  if (total_pairs == 0) return 0;
  if (P == 0 || !dt_word_offset || !dt_hw || !dt_extent || !gt_word_offset || !gt_hw || !gt_extent || !counts ||
      total_pairs > static_cast<int64_t>(kWaves) * 0x7fffffff)
    return DETOPS_EINVAL;
  hipLaunchKernelGGL(mask_pair_counts_kernel, dim3(static_cast<unsigned>(ceil_div64(total_pairs, kWaves))), dim3(kBlock), 0,
                     as_stream(stream), reinterpret_cast<const detops_u64*>(dt_words), dt_word_offset, dt_hw, dt_extent,
                     reinterpret_cast<const detops_u64*>(gt_words), gt_word_offset, gt_hw, gt_extent, dt_offset, gt_offset,
                     iou_offset, P, total_pairs, counts);
  return launch_status();
}

DETOPS_API int detops_eval_iou(int mode, const int32_t* counts, const int32_t* dt_area, const int32_t* gt_area,
                               const float* dt_boxes, const float* gt_boxes, const unsigned char* gt_crowd,
                               const int32_t* dt_offset, const int32_t* gt_offset, const int64_t* iou_offset, int P,
                               int64_t total_pairs, double* iou, detops_stream_t stream) {
  if (total_pairs < 0 || bad_problem_args(dt_offset, gt_offset, iou_offset, P) ||
      (mode != DETOPS_EVAL_COCO_SEGM && mode != DETOPS_EVAL_COCO_BBOX && mode != DETOPS_EVAL_VOC))
    return DETOPS_EINVAL;
  if (total_pairs == 0) return 0;
  if (P == 0 || !iou) return DETOPS_EINVAL;
  if (mode == DETOPS_EVAL_COCO_SEGM ? (!counts || !dt_area || !gt_area) : (!dt_boxes || !gt_boxes)) return DETOPS_EINVAL;
  hipLaunchKernelGGL(eval_iou_kernel, dim3(static_cast<unsigned>(ceil_div64(total_pairs, kBlock))), dim3(kBlock), 0,
                     as_stream(stream), mode, counts, dt_area, gt_area, dt_boxes, gt_boxes, gt_crowd, dt_offset, gt_offset,
                     iou_offset, P, total_pairs, iou);
  return launch_status();
}

DETOPS_API int detops_eval_match(int mode, const double* iou, const int32_t* dt_offset, const int32_t* gt_offset,
                                 const int64_t* iou_offset, int P, int64_t D_total, int64_t G_total, int max_gt,
                                 const double* dt_area, const double* gt_area,
                                 const unsigned char* gt_flag, const double* iou_thrs, int T, const double* area_rngs, int A,
                                 int32_t* dt_match, unsigned char* dt_ignore, unsigned char* gt_ignore, signed char* voc_match,
                                 detops_stream_t stream) {
  if (max_gt < 0 || D_total < 0 || G_total < 0 || bad_problem_args(dt_offset, gt_offset, iou_offset, P) ||
      (mode != DETOPS_EVAL_COCO_SEGM && mode != DETOPS_EVAL_COCO_BBOX && mode != DETOPS_EVAL_VOC))
    return DETOPS_EINVAL;
  if (P == 0) return 0;
  if (!iou_thrs || (G_total > 0 && !gt_flag)) return DETOPS_EINVAL;   // iou is null when no problem has a pair
  const int served = max_gt > kMaxGt ? kMaxGt : max_gt;
  if (mode == DETOPS_EVAL_VOC) {
    if (D_total > 0 && !voc_match) return DETOPS_EINVAL;
    hipLaunchKernelGGL(eval_match_voc_kernel, dim3(static_cast<unsigned>(P)), dim3(kWave), static_cast<size_t>(served),
                       as_stream(stream), iou, dt_offset, gt_offset, iou_offset, P, D_total, G_total, gt_flag, iou_thrs, served,
                       voc_match);
  } else {
    if (T < 1 || A < 1 || static_cast<int64_t>(A) * T > 4096 || !area_rngs ||
        (D_total > 0 && (!dt_area || !dt_match || !dt_ignore)) || (G_total > 0 && (!gt_area || !gt_ignore)))
      return DETOPS_EINVAL;
    const int lds_words = served > 64 ? (served + 63) / 64 : 0;
    hipLaunchKernelGGL(eval_match_coco_kernel, dim3(static_cast<unsigned>(P)), dim3(kWave),
                       static_cast<size_t>(lds_words) * kWave * sizeof(detops_u64), as_stream(stream), iou, dt_offset,
                       gt_offset, iou_offset, P, D_total, G_total, dt_area, gt_area, gt_flag, iou_thrs, T, area_rngs, A, lds_words,
                       dt_match,
                       dt_ignore, gt_ignore);
  }
  const int rc = launch_status();
  if (rc != 0) return rc;
  return max_gt > kMaxGt ? DETOPS_EGTCAP : 0;
}
