// cityscapes_eval.hip — the pixel counts behind the Cityscapes instance-level AP, for gfx950 (MI355X).
//
//   detops_window_counts   for one image: the windowed pixel count of every predicted and every ground-truth plane, and
//                          for every (prediction, ground truth) pair whose boxes overlap the box intersection and the
//                          count of the pixels set in both planes inside the union box (reference
//                          data/datasets/evaluation/cityscapes/eval_instances.py: matchGtWithPred, which crops, multiplies,
//                          sums and calls .item() once per pair and per instance)
//
// The definitions are in include/detops.h ("Cityscapes evaluation").  Two launches.  The first writes every output
// element: zeros into the three pixel counts, the box intersection into pair_box.  The second counts: its work items are
// the D + G self windows and the D x G pairs (blockIdx.x), each cut into strips of rows (blockIdx.y); a workgroup whose
// pair does not overlap, or whose strip lies below the window, leaves after reading two boxes and no plane.
//
// Inside a strip a thread takes units of (row, 16-byte chunk of the FIRST plane's row segment): a chunk that lies inside
// the segment moves as one 16-byte access, aligned for the first plane (planes of a batch do not start aligned when H * W
// is odd, rows do not when W is no multiple of 16, and a window starts at any column, so the alignment is taken per row
// from the address); the second plane of a pair sits at another residue and is read through memcpy, which the compiler
// lowers to an access it may issue unaligned.  The chunks at a segment's head and tail are read byte by byte.  A set pixel
// is a non-zero byte.  Integers only: the strips of a window are combined with 32-bit integer atomics on the zeros of the
// first launch, and any order gives the same bits.
#include "detops_dtype.h"

#include <string.h>

namespace {

constexpr int kBlock = 256;
constexpr int kStripRows = 64, kMaxStrips = 64;

struct Box {
  int64_t x0, y0, x1, y1;
};

__host__ __device__ inline Box load_box(const int32_t* b) { return Box{b[0], b[1], b[2], b[3]}; }
__host__ __device__ inline int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }
__host__ __device__ inline int64_t max64(int64_t a, int64_t b) { return a > b ? a : b; }

// isOverlapping: strict on all four sides
__host__ __device__ inline bool overlapping(const Box& a, const Box& b) {
  return a.x0 < b.x1 && b.x0 < a.x1 && a.y0 < b.y1 && b.y0 < a.y1;
}

// the box clamped to the image: rows [y0, y1), columns [x0, x1); empty when a maximum does not exceed its minimum
__host__ __device__ inline Box clamp_window(const Box& b, int H, int W) {
  return Box{min64(max64(b.x0, 0), W), min64(max64(b.y0, 0), H), min64(max64(b.x1, 0), W), min64(max64(b.y1, 0), H)};
}

// per byte of x: 0x80 where the byte is not zero
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t x) {
  return (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
}

__device__ __forceinline__ uint4 load16_any(const uint8_t* p) {
  uint4 v;
  memcpy(&v, p, sizeof(v));
  return v;
}

// rows and strips of a window of `rows` rows: at most kMaxStrips strips of at least kStripRows rows
__host__ __device__ inline int strip_rows(int H) {
  const int strips = min64(ceil_div64(H, kStripRows), kMaxStrips);
  return strips > 0 ? static_cast<int>(ceil_div64(H, strips)) : kStripRows;
}

// every output element: zeros for the counts the second launch adds into, the box intersection for pair_box
__global__ void __launch_bounds__(kBlock)
window_init_kernel(const int32_t* __restrict__ dt_box, const int32_t* __restrict__ gt_box, int D, int G,
                   int32_t* __restrict__ dt_count, int32_t* __restrict__ gt_count, int32_t* __restrict__ pair_box,
                   int32_t* __restrict__ pair_mask) {
  const int64_t pairs = static_cast<int64_t>(D) * G;
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i < D) dt_count[i] = 0;
  if (i < G) gt_count[i] = 0;
  if (i < pairs) {
    const Box d = load_box(dt_box + 4 * (i / G)), g = load_box(gt_box + 4 * (i % G));
    int64_t inter = 0;
    if (overlapping(d, g)) {
      // each side lies in (-2^32, 2^32); positive for boxes whose minima lie below their maxima
      inter = (min64(d.x1, g.x1) - max64(d.x0, g.x0)) * (min64(d.y1, g.y1) - max64(d.y0, g.y0));
      inter = min64(max64(inter, -0x7fffffffll - 1), 0x7fffffff);                                     // saturated
    }
    pair_box[i] = static_cast<int32_t>(inter);
    pair_mask[i] = 0;
  }
}

// grid (D + G + D * G, strips).  Everything before the unit loop is uniform over the workgroup, the two early returns too.
__global__ void __launch_bounds__(kBlock)
window_count_kernel(const uint8_t* __restrict__ dt_planes, const int32_t* __restrict__ dt_box, int D,
                    const uint8_t* __restrict__ gt_planes, const int32_t* __restrict__ gt_box, int G, int H, int W,
                    int rows_per_strip, int32_t* __restrict__ dt_count, int32_t* __restrict__ gt_count,
                    int32_t* __restrict__ pair_mask) {
  __shared__ int red[kBlock / kWave];
  const int64_t item = blockIdx.x, plane = static_cast<int64_t>(H) * W;
  const uint8_t *pa, *pb = nullptr;
  int32_t* out;
  Box win;
  if (item < D) {
    win = load_box(dt_box + 4 * item);
    pa = dt_planes + item * plane;
    out = dt_count + item;
  } else if (item < static_cast<int64_t>(D) + G) {
    const int64_t g = item - D;
    win = load_box(gt_box + 4 * g);
    pa = gt_planes + g * plane;
    out = gt_count + g;
  } else {
    const int64_t p = item - D - G, d = p / G, g = p % G;
    const Box bd = load_box(dt_box + 4 * d), bg = load_box(gt_box + 4 * g);
    if (!overlapping(bd, bg)) return;
    win = Box{min64(bd.x0, bg.x0), min64(bd.y0, bg.y0), max64(bd.x1, bg.x1), max64(bd.y1, bg.y1)};
    pa = dt_planes + d * plane;
    pb = gt_planes + g * plane;
    out = pair_mask + p;
  }
  win = clamp_window(win, H, W);
  const int64_t w = win.x1 - win.x0;
  const int64_t r0 = win.y0 + static_cast<int64_t>(blockIdx.y) * rows_per_strip, r1 = min64(r0 + rows_per_strip, win.y1);
  if (w <= 0 || r0 >= r1) return;
  // every access below lies in rows [r0, r1) <= [0, H) and columns [win.x0, win.x1) <= [0, W) of the item's planes
  // (32-bit: rows of a strip x chunks of a row stays below H * W / 16 + 2 H)
  const int per_row = static_cast<int>((w + 15) / 16 + 1);       // aligned chunks that a segment of w bytes can touch
  const int units = static_cast<int>(r1 - r0) * per_row;
  int count = 0;
  for (int u = threadIdx.x; u < units; u += kBlock) {
    const int row = u / per_row, c = u % per_row;
    const int64_t off = (r0 + row) * W + win.x0;                                  // the segment's first byte in its plane
    const int64_t lead = static_cast<int64_t>(reinterpret_cast<uintptr_t>(pa + off) & 15);
    const int64_t lo = max64(c * 16ll - lead, 0), hi = min64(c * 16ll - lead + 16, w);   // bytes [lo, hi) of the segment
    if (lo >= hi) continue;
    if (hi - lo == 16) {
      const uint4 a = *reinterpret_cast<const uint4*>(pa + off + lo);
      uint32_t m0 = nonzero_bytes(a.x), m1 = nonzero_bytes(a.y), m2 = nonzero_bytes(a.z), m3 = nonzero_bytes(a.w);
      if (pb) {
        const uint4 b = load16_any(pb + off + lo);
        m0 &= nonzero_bytes(b.x);
        m1 &= nonzero_bytes(b.y);
        m2 &= nonzero_bytes(b.z);
        m3 &= nonzero_bytes(b.w);
      }
      count += __popc(m0) + __popc(m1) + __popc(m2) + __popc(m3);
    } else {
      for (int64_t k = lo; k < hi; ++k) count += (pa[off + k] != 0 && (!pb || pb[off + k] != 0)) ? 1 : 0;
    }
  }
  count = block_sum<kBlock>(count, red);
  if (threadIdx.x == 0 && count) atomicAdd(out, count);
}

}  // namespace

DETOPS_API int detops_window_counts(const unsigned char* dt_planes, const int32_t* dt_box, int D,
                                    const unsigned char* gt_planes, const int32_t* gt_box, int G, int H, int W,
                                    int32_t* dt_count, int32_t* gt_count, int32_t* pair_box, int32_t* pair_mask,
                                    detops_stream_t stream) {
  if (D < 0 || G < 0 || H < 0 || W < 0 || static_cast<int64_t>(H) * W > 0x7fffffff) return DETOPS_EINVAL;
  if (D > 0 && (!dt_box || !dt_count)) return DETOPS_EINVAL;
  if (G > 0 && (!gt_box || !gt_count)) return DETOPS_EINVAL;
  const int64_t pairs = static_cast<int64_t>(D) * G, area = static_cast<int64_t>(H) * W;
  if (pairs > 0 && (!pair_box || !pair_mask)) return DETOPS_EINVAL;
  if (area > 0 && ((D > 0 && !dt_planes) || (G > 0 && !gt_planes))) return DETOPS_EINVAL;
  const int64_t items = static_cast<int64_t>(D) + G + pairs;
  if (items >= DETOPS_WINDOW_COUNTS_MAX_ITEMS) return DETOPS_EINVAL;
  if (items == 0) return 0;
  hipStream_t st = as_stream(stream);
  const int64_t most = max64(pairs, max64(D, G));
  hipLaunchKernelGGL(window_init_kernel, dim3(static_cast<unsigned>(ceil_div64(most, kBlock))), dim3(kBlock), 0, st, dt_box,
                     gt_box, D, G, dt_count, gt_count, pair_box, pair_mask);
  const int rc = launch_status();
  if (rc || area == 0) return rc;
  const int rows = strip_rows(H);
  hipLaunchKernelGGL(window_count_kernel, dim3(static_cast<unsigned>(items), static_cast<unsigned>(ceil_div64(H, rows))),
                     dim3(kBlock), 0, st, dt_planes, dt_box, D, gt_planes, gt_box, G, H, W, rows, dt_count, gt_count, pair_mask);
  return launch_status();
}
