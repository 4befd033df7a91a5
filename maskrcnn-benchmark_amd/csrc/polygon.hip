// polygon.hip — polygon instance masks rasterised on the device, for gfx950 (MI355X).
//
//   detops_polygon_mask_targets   mask-head targets straight from polygons (reference roi_heads/mask_head/loss.py:11-42 over
//                                 structures/segmentation_mask.py:273-335: PolygonInstance.crop, .resize, convert_to_binarymask)
//                                 for every slot of every image of the batch in one launch
//   detops_polygons_to_masks      the dense H x W planes of the instances of one image (convert("mask"))
//
// The rasteriser is the polygon-to-RLE routine restated in include/detops.h.  Its boundary walk visits up to 5 * |edge|
// points per edge; only the steps of the walk across u = 5c + 2 | 5c + 3 (c a column of the grid) produce a crossing, an
// edge makes that step at most once per column, and where it does follows in closed form.  The work item here is
// therefore one (edge, column) pair: the work of a slot is edges x M whatever the ratio of instance size to box size.
//
// Crossings toggle a bit per pixel in LDS (column-major: one run of words per column).  A closed polygon steps across a
// column's boundary an even number of times, so the running parity of the definition (which runs through all columns)
// is zero at every column's start once the crossings clamped to row h are counted; those land on row 0 of the NEXT column
// and cancel exactly the parity their own column hands over.  Dropping them and taking the prefix parity per column is
// the same fill, and lets a workgroup own a strip of columns.
#include "detops_dtype.h"

namespace {

constexpr int kBlock = 256;
constexpr int kEdgeChunk = 256;          // edges staged in LDS at a time (one per thread)
constexpr int kCoordLimit = 500000000;   // |5 * coordinate| at most: differences of two stay an int32
constexpr int kMaxM = 256;
constexpr int kStrip = 64;               // columns of a plane per workgroup
constexpr int kMaxPlaneH = 3584;         // 2 * kStrip * (H / 32) words + the edge stage within 64 KiB of LDS
constexpr int kSeg = 16;                 // bytes per wide store
constexpr int kRowItems = kStrip / kSeg + 2;   // head, 16-byte segments, tail of a strip's row

// ---------------------------------------------------------------------------------------------------- the definition
// int(5.0 * v + .5): fp64, two roundings, truncation toward zero (so (-0.1, 0) gives 0).  NaN and values beyond
// +-kCoordLimit saturate (the C cast is undefined there)
__device__ __forceinline__ int scaled_vertex(float v) {
#pragma clang fp contract(off)
  double z = 5.0 * static_cast<double>(v);
  z = z + 0.5;
  if (!(z > -static_cast<double>(kCoordLimit))) return -kCoordLimit;
  if (z > static_cast<double>(kCoordLimit)) return kCoordLimit;
  return static_cast<int>(z);
}

// int(a + s * t + .5) of the walk
__device__ __forceinline__ int walk_point(int a, double s, int t) {
#pragma clang fp contract(off)
  double z = s * static_cast<double>(t);
  z = static_cast<double>(a) + z;
  z = z + 0.5;
  return static_cast<int>(z);
}

// Edge e = (xs, ys, xe, ye) in upsampled integers against column c of a grid of h rows: the row at which the crossing
// toggles, or -1 (the walk does not step across 5c + 2 | 5c + 3, or the crossing is clamped to row h: see the top).
__device__ __forceinline__ int crossing_row(int4 e, int c, int h) {
#pragma clang fp contract(off)
  const int A = 5 * c + 2;
  if (min(e.x, e.z) > A || max(e.x, e.z) <= A) return -1;
  int xs = e.x, ys = e.y, xe = e.z, ye = e.w;
  const int dx = abs(xe - xs), dy = abs(ys - ye);
  const bool x_major = dx >= dy;
  if (x_major ? xs > xe : ys > ye) {          // the walk's own orientation: the major coordinate grows with t
    int k = xs; xs = xe; xe = k;
    k = ys; ys = ye; ye = k;
  }
  int vm;                                     // min of v over the two points of the step
  if (x_major) {                              // u = t + xs exactly; dx > 0 because the edge spans a boundary
    const double s = static_cast<double>(ye - ys) / static_cast<double>(dx);
    const int t = A - xs;
    vm = min(walk_point(ys, s, t), walk_point(ys, s, t + 1));
  } else {
    // u(t) = int(xs + s * t + .5) is monotone in t and moves by at most 1 per step: the step is (t - 1, t) for the first t
    // at which u has reached the far side, P(t).  P(0) is false and P(dy) is true.  The estimate from the real line is off
    // by a step at most; the literal u decides.
    const double s = static_cast<double>(xe - xs) / static_cast<double>(dy);
    const bool up = xe > xs;
    const double tau = (static_cast<double>(A) + 0.5 - static_cast<double>(xs)) / s;
    double guess = up ? ceil(tau) : floor(tau) + 1.0;
    guess = fmin(fmax(guess, 1.0), static_cast<double>(dy));
    int t = static_cast<int>(guess);
    auto reached = [&](int tt) { const int u = walk_point(xs, s, tt); return up ? u > A : u <= A; };
    while (t > 1 && reached(t - 1)) --t;
    while (t < dy && !reached(t)) ++t;
    vm = t - 1 + ys;                          // v = t + ys
  }
  // ceil(clamp((vm + .5) / 5 - .5, 0, h)) = ceil((vm - 2) / 5) clamped: the fp64 form is exact at vm = 5r + 2 and at
  // least 0.2 from an integer elsewhere
  const int n = vm - 2;
  const int r = n <= 0 ? 0 : (n + 4) / 5;
  return r >= h ? -1 : r;
}

// inclusive prefix parity of the bits of a word (bit i = xor of bits 0 .. i)
__device__ __forceinline__ uint32_t prefix_parity(uint32_t x) {
  x ^= x << 1;
  x ^= x << 2;
  x ^= x << 4;
  x ^= x << 8;
  x ^= x << 16;
  return x;
}

struct Identity {
  __device__ __forceinline__ float2 operator()(float2 v) const { return v; }
};

// PolygonInstance.crop(box).resize((M, M)) of one slot: fp32(fp32(x - xmin) * fp32(M / (xmax - xmin))), the window and
// the quotient in fp64, no rounding of the window, vertices not clamped
struct CropResize {
  float x0, y0, fx, fy;
  __device__ __forceinline__ float2 operator()(float2 v) const {
#pragma clang fp contract(off)
    float x = v.x - x0, y = v.y - y0;
    x = x * fx;
    y = y * fy;
    return make_float2(x, y);
  }
};

__device__ __forceinline__ CropResize slot_transform(const float* __restrict__ b, int W, int H, int M) {
#pragma clang fp contract(off)
  const double xmin = fmin(fmax(static_cast<double>(b[0]), 0.0), static_cast<double>(W - 1));
  const double ymin = fmin(fmax(static_cast<double>(b[1]), 0.0), static_cast<double>(H - 1));
  const double xmax = fmax(fmin(fmax(static_cast<double>(b[2]), 0.0), static_cast<double>(W)), xmin + 1.0);
  const double ymax = fmax(fmin(fmax(static_cast<double>(b[3]), 0.0), static_cast<double>(H)), ymin + 1.0);
  CropResize t;
  t.x0 = static_cast<float>(xmin);
  t.y0 = static_cast<float>(ymin);
  t.fx = static_cast<float>(static_cast<double>(M) / (xmax - xmin));
  t.fy = static_cast<float>(static_cast<double>(M) / (ymax - ymin));
  return t;
}

// LDS of the edge stage: the chunk's edges, where each edge's crossings start in the chunk's work list, the waves' sums
static_assert(kEdgeChunk == kBlock, "a thread per staged edge");
struct EdgeStage {
  int4 edge[kEdgeChunk];
  int start[kEdgeChunk];
  int wave_sum[kBlock / kWave];
};

// columns of [c0, c0 + ncols) whose boundary the edge spans: [first, first + count)
__device__ __forceinline__ int2 edge_columns(int4 e, int c0, int ncols) {
  const int lo = min(e.x, e.z) - 2, hi = max(e.x, e.z) - 3;   // lo <= 5c and 5c <= hi
  if (hi < 0) return make_int2(0, 0);
  const int first = max(lo > 0 ? (lo + 4) / 5 : 0, c0), last = min(hi / 5, c0 + ncols - 1);
  return make_int2(first, max(last - first + 1, 0));
}

// The union of the fills of polygons [p0, p1) over columns [c0, c0 + ncols) of a grid of h rows, as bits in
// res[(column - c0) * hw + row / 32].  tog and res ([ncols * hw] words each) must be zero and the workgroup in step on
// entry; tog is zero again and the workgroup in step on return.  A polygon of fewer than 3 vertices fills nothing.
// Per chunk of edges: a thread per edge turns its vertices into integers and counts the columns it spans; a scan of the
// counts lays the (edge, column) pairs out as one dense list, which the threads then share: few pairs of the
// edges x columns rectangle are crossings, and a wave that held one of them would run the fp64 walk for all its lanes.
template <typename Transform>
__device__ __forceinline__ void fill_polygons(const float2* __restrict__ verts, const int* __restrict__ poly_offset, int p0, int p1,
                                              int V, Transform xf, int c0, int ncols, int h, int hw, uint32_t* tog,
                                              uint32_t* res, EdgeStage* st) {
  const int tid = threadIdx.x;
  for (int p = p0; p < p1; ++p) {
    const int v0 = min(max(poly_offset[p], 0), V);
    const int k = min(max(poly_offset[p + 1], v0), V) - v0;
    if (k < 3) continue;
    for (int eb = 0; eb < k; eb += kEdgeChunk) {
      const int n = min(kEdgeChunk, k - eb);
      int count = 0;
      if (tid < n) {
        const int j = eb + tid;
        const float2 a = xf(verts[v0 + j]), b = xf(verts[v0 + (j + 1 == k ? 0 : j + 1)]);
        const int4 e = make_int4(scaled_vertex(a.x), scaled_vertex(a.y), scaled_vertex(b.x), scaled_vertex(b.y));
        st->edge[tid] = e;
        count = edge_columns(e, c0, ncols).y;
      }
      int total;
      st->start[tid] = block_scan<kBlock>(count, st->wave_sum, total) - count;     // threads beyond the chunk: the total
      __syncthreads();
      for (int i = tid; i < total; i += kBlock) {
        // the last edge with start[e] <= i: edges without crossings share their start with the next edge that has some
        const int e = last_at_or_below(st->start, n, i);
        const int4 edge = st->edge[e];
        const int c = edge_columns(edge, c0, ncols).x + (i - st->start[e]);
        const int r = crossing_row(edge, c, h);
        if (r >= 0) atomicXor(&tog[(c - c0) * hw + (r >> 5)], 1u << (r & 31));
      }
      __syncthreads();
    }
    for (int cl = tid; cl < ncols; cl += kBlock) {
      uint32_t carry = 0;
      for (int i = 0; i < hw; ++i) {
        const uint32_t f = prefix_parity(tog[cl * hw + i]) ^ carry;
        carry = 0u - (f >> 31);
        res[cl * hw + i] |= f;
        tog[cl * hw + i] = 0;
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------- mask-head targets
// One workgroup per slot.  LDS: tog [M * hw], res [M * hw], the edge stage.
__global__ void __launch_bounds__(kBlock)
polygon_mask_targets_kernel(const float2* __restrict__ verts, const int* __restrict__ poly_offset,
                            const int* __restrict__ inst_offset, int V, int P, int G, const int64_t* __restrict__ slot_inst,
                            const float* __restrict__ boxes, const int* __restrict__ slot_wh, int M, bool vec4,
                            float* __restrict__ out) {
  DETOPS_DYNAMIC_LDS(uint32_t, lds);
  const int64_t s = blockIdx.x;
  const int hw = (M + 31) / 32;
  uint32_t* tog = lds;
  uint32_t* res = lds + M * hw;
  EdgeStage* stage = reinterpret_cast<EdgeStage*>(lds + ((2 * M * hw + 3) & ~3));
  for (int i = threadIdx.x; i < 2 * M * hw; i += kBlock) lds[i] = 0;
  __syncthreads();
  const int64_t g = slot_inst[s];
  if (g >= 0 && g < G) {
    const int p0 = min(max(inst_offset[g], 0), P), p1 = min(max(inst_offset[g + 1], p0), P);
    const CropResize xf = slot_transform(boxes + s * 4, slot_wh[s * 2], slot_wh[s * 2 + 1], M);
    fill_polygons(verts, poly_offset, p0, p1, V, xf, 0, M, M, hw, tog, res, stage);
  }
  float* o = out + s * M * M;
  if (vec4) {                                 // M % 4 == 0 and `out` 16-byte aligned: four columns of one row
    for (int i = threadIdx.x; i < M * M / 4; i += kBlock) {
      const int r = (4 * i) / M, c = (4 * i) % M;
      float q[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) q[j] = static_cast<float>((res[(c + j) * hw + (r >> 5)] >> (r & 31)) & 1u);
      reinterpret_cast<float4*>(o)[i] = make_float4(q[0], q[1], q[2], q[3]);
    }
  } else {
    for (int i = threadIdx.x; i < M * M; i += kBlock) {
      const int r = i / M, c = i % M;
      o[i] = static_cast<float>((res[c * hw + (r >> 5)] >> (r & 31)) & 1u);
    }
  }
}

// ---------------------------------------------------------------------------------------------------- dense planes
// Workgroup (strip, instance): columns [strip * kStrip, + kStrip) of the instance's H x W plane.  A row of the strip is
// cut at the 16-byte boundaries of its address into a head, 16-byte segments and a tail; every byte of the plane is
// written once, zeros included.  LDS: tog [kStrip * hw], res [kStrip * hw], the edge stage.
__global__ void __launch_bounds__(kBlock)
polygons_to_masks_kernel(const float2* __restrict__ verts, const int* __restrict__ poly_offset,
                         const int* __restrict__ inst_offset, int V, int P, int H, int W, unsigned char* __restrict__ out) {
  DETOPS_DYNAMIC_LDS(uint32_t, lds);
  const int g = blockIdx.y;
  const int c0 = blockIdx.x * kStrip, ncols = min(kStrip, W - c0);
  const int hw = (H + 31) / 32;
  uint32_t* tog = lds;
  uint32_t* res = lds + kStrip * hw;
  EdgeStage* stage = reinterpret_cast<EdgeStage*>(lds + 2 * kStrip * hw);
  for (int i = threadIdx.x; i < 2 * kStrip * hw; i += kBlock) lds[i] = 0;
  __syncthreads();
  const int p0 = min(max(inst_offset[g], 0), P), p1 = min(max(inst_offset[g + 1], p0), P);
  fill_polygons(verts, poly_offset, p0, p1, V, Identity(), c0, ncols, H, hw, tog, res, stage);
  unsigned char* plane = out + static_cast<int64_t>(g) * H * W;
  for (int i = threadIdx.x; i < H * kRowItems; i += kBlock) {
    const int r = i / kRowItems, item = i % kRowItems;
    unsigned char* row = plane + static_cast<int64_t>(r) * W + c0;
    const int head = min(static_cast<int>((0 - reinterpret_cast<uintptr_t>(row)) & (kSeg - 1)), ncols);
    const int nbody = (ncols - head) / kSeg;
    int cl, len;
    if (item == 0) { cl = 0; len = head; }
    else if (item <= nbody) { cl = head + (item - 1) * kSeg; len = kSeg; }
    else if (item == nbody + 1) { cl = head + nbody * kSeg; len = ncols - cl; }
    else continue;
    const uint32_t* w = res + (r >> 5);
    const int sh = r & 31;
    if (len == kSeg) {
      uint32_t q[4] = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int j = 0; j < kSeg; ++j) q[j / 4] |= ((w[(cl + j) * hw] >> sh) & 1u) << (8 * (j % 4));
      *reinterpret_cast<uint4*>(row + cl) = make_uint4(q[0], q[1], q[2], q[3]);
    } else {
      for (int j = 0; j < len; ++j) row[cl + j] = static_cast<unsigned char>((w[(cl + j) * hw] >> sh) & 1u);
    }
  }
}

}  // namespace

DETOPS_API int detops_polygon_mask_targets(const float* verts, const int32_t* poly_offset, const int32_t* inst_offset, int V,
                                           int P, int G, const int64_t* slot_inst, const float* boxes,
                                           const int32_t* slot_wh, int S, int M, float* out, detops_stream_t stream) {
  if (V < 0 || P < 0 || G < 0 || S < 0 || M < 1 || M > kMaxM) return DETOPS_EINVAL;
  if (S == 0) return 0;
  if (!poly_offset || !inst_offset || !slot_inst || !boxes || !slot_wh || !out || (V > 0 && !verts)) return DETOPS_EINVAL;
  const int hw = (M + 31) / 32;
  const size_t lds = static_cast<size_t>((2 * M * hw + 3) & ~3) * sizeof(uint32_t) + sizeof(EdgeStage);
  const bool vec4 = M % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
  hipLaunchKernelGGL(polygon_mask_targets_kernel, dim3(static_cast<unsigned>(S)), dim3(kBlock), lds, as_stream(stream),
                     reinterpret_cast<const float2*>(verts), poly_offset, inst_offset, V, P, G, slot_inst, boxes, slot_wh, M,
                     vec4, out);
  return launch_status();
}

DETOPS_API int detops_polygons_to_masks(const float* verts, const int32_t* poly_offset, const int32_t* inst_offset, int V,
                                        int P, int G, int H, int W, unsigned char* out, detops_stream_t stream) {
  if (V < 0 || P < 0 || G < 0 || H < 0 || W < 0 || H > kMaxPlaneH || G > 65535) return DETOPS_EINVAL;
  if (G == 0 || H == 0 || W == 0) return 0;
  if (!poly_offset || !inst_offset || !out || (V > 0 && !verts)) return DETOPS_EINVAL;
  const int hw = (H + 31) / 32;
  const size_t lds = static_cast<size_t>(2 * kStrip * hw) * sizeof(uint32_t) + sizeof(EdgeStage);
  const dim3 grid(static_cast<unsigned>((W + kStrip - 1) / kStrip), static_cast<unsigned>(G));
  hipLaunchKernelGGL(polygons_to_masks_kernel, grid, dim3(kBlock), lds, as_stream(stream),
                     reinterpret_cast<const float2*>(verts), poly_offset, inst_offset, V, P, H, W, out);
  return launch_status();
}
