// masker.hip — Mask R-CNN inference: paste every detection's M x M probability map into its image, for gfx950 (MI355X).
//
//   detops_paste_masks            Masker / paste_mask_in_image (reference roi_heads/mask_head/inference.py:91-199) for every
//                                 detection of every image of the batch in one launch: the uint8 H x W planes, every byte
//                                 written exactly once
//   detops_paste_masks_rle_count  the same masks as uncompressed COCO RLE (column-major run lengths) without the planes:
//   detops_paste_masks_rle_write  a count pass over the clipped windows, two small scans, [one host read of the total], a
//                                 write pass
//
// The reference runs `interpolate`, the threshold and a slice assignment in a Python loop over the detections on the
// CPU.  Both consumers here evaluate a pixel with the same three device functions: load_det (box -> integer window),
// axis_tap (ATen's bilinear source index and weight of one output coordinate) and mask_bit (four taps, threshold).
#include "detops_dtype.h"

namespace {

constexpr int kBlock = 256;
constexpr int kMaxPadded = 64;       // M + 2 * padding at most (a 56 x 56 map with padding 1 is 58)
constexpr int kSeg = 16;             // pixels (= bytes) per lane and row: one 16-byte store
constexpr int kRowClasses = 16;      // rows r, r + 16, ... of a plane start at the same address modulo 16
constexpr int kBoxLimit = 500000000; // |integer box coordinate| at most: w = x2 - x1 + 1 stays an int32

// ---------------------------------------------------------------------------------------------------- the definition
struct Det {
  int H, W;             // the image
  int x1, y1;           // expanded box, truncated: where pixel (0, 0) of the resized map lands
  int w, h;             // the resized map
  int cx0, cx1;         // clipped window, columns [cx0, cx1) and rows [ry0, ry1); empty = all four 0
  int ry0, ry1;
  float rx, ry;         // ATen's resize ratios float(P) / w, float(P) / h
};

struct Tap {
  int i0;               // lower source index; the upper one is i0 + 1 (the staged map repeats its last row and column)
  float l1;             // weight of the upper tap
};

// torch's float -> int32 conversion: truncation toward zero (-0.4 -> 0, where floor gives -1).  NaN and values beyond
// +-kBoxLimit saturate (the C cast is undefined there); such a box cannot meet an image
__device__ __forceinline__ int trunc_i32(float v) {
  if (!(v > -static_cast<float>(kBoxLimit))) return -kBoxLimit;
  if (v > static_cast<float>(kBoxLimit)) return kBoxLimit;
  return static_cast<int>(v);
}

// expand_boxes in fp32 (every step one rounding, `scale` = the Python float rounded to fp32 by the tensor multiply),
// the int32 conversion, w / h and the clipped window of paste_mask_in_image (:124-157)
__device__ __forceinline__ Det load_det(const float* __restrict__ boxes, const int* __restrict__ det_hw, int64_t n, int P,
                                        float scale) {
#pragma clang fp contract(off)
  const float* b = boxes + n * 4;
  const float bx1 = b[0], by1 = b[1], bx2 = b[2], by2 = b[3];
  float w_half = (bx2 - bx1) * 0.5f, h_half = (by2 - by1) * 0.5f;
  const float x_c = (bx2 + bx1) * 0.5f, y_c = (by2 + by1) * 0.5f;
  w_half *= scale;
  h_half *= scale;
  Det d;
  d.H = det_hw[n * 2];
  d.W = det_hw[n * 2 + 1];
  d.x1 = trunc_i32(x_c - w_half);
  d.y1 = trunc_i32(y_c - h_half);
  const int x2 = trunc_i32(x_c + w_half), y2 = trunc_i32(y_c + h_half);
  d.w = max(x2 - d.x1 + 1, 1);
  d.h = max(y2 - d.y1 + 1, 1);
  d.cx0 = max(d.x1, 0);
  d.cx1 = min(x2 + 1, d.W);
  d.ry0 = max(d.y1, 0);
  d.ry1 = min(y2 + 1, d.H);
  if (d.cx1 <= d.cx0 || d.ry1 <= d.ry0) d.cx0 = d.cx1 = d.ry0 = d.ry1 = 0;   // the box misses the image: all zeros
  d.rx = static_cast<float>(P) / static_cast<float>(d.w);
  d.ry = static_cast<float>(P) / static_cast<float>(d.h);
  return d;
}

// ATen's CPU bilinear resize, align_corners = False (UpSampleKernel.cpp compute_source_index_and_lambda): output
// coordinate d of `out` over `in` inputs
__device__ __forceinline__ Tap axis_tap(int d, int in, int out, float ratio) {
#pragma clang fp contract(off)
  Tap t;
  if (out == in) {
    t.i0 = d;
    t.l1 = 0.f;
    return t;
  }
  float src = ratio * (static_cast<float>(d) + 0.5f) - 0.5f;
  src = src < 0.f ? 0.f : src;
  t.i0 = min(static_cast<int>(src), in - 1);
  t.l1 = fminf(fmaxf(src - static_cast<float>(t.i0), 0.f), 1.f);
  return t;
}

// one pixel: the four taps in ATen's order, then the threshold (`threshold < 0`: the reference's debugging mode)
__device__ __forceinline__ bool mask_bit(const float* smap, int stride, Tap ty, Tap tx, float threshold) {
#pragma clang fp contract(off)
  const float* p = smap + ty.i0 * stride + tx.i0;
  const float a = p[0], b = p[1], c = p[stride], d = p[stride + 1];
  const float wx0 = 1.f - tx.l1, hy0 = 1.f - ty.l1;
  const float v = hy0 * (wx0 * a + tx.l1 * b) + ty.l1 * (wx0 * c + tx.l1 * d);
  return threshold >= 0.f ? v > threshold : v * 255.f != 0.f;
}

// The zero-padded map of one detection in LDS as fp32, [P + 1][P + 1]: row and column P repeat row and column P - 1, so
// that the upper tap is always at i0 + 1 (ATen's index min(i0 + 1, P - 1): the same element)
template <typename T>
__device__ __forceinline__ void stage_map(const T* __restrict__ m, int M, int pad, float* smap) {
  const int P = M + 2 * pad, S = P + 1;
  for (int i = threadIdx.x; i < S * S; i += kBlock) {
    const int y = min(i / S, P - 1) - pad, x = min(i % S, P - 1) - pad;
    smap[i] = (y >= 0 && y < M && x >= 0 && x < M) ? Io<T>::ld(m[y * M + x]) : 0.f;
  }
}

// ---------------------------------------------------------------------------------------------------- dense planes
// `len` < 16 bytes of q (little-endian, byte 0 first) to an address of any alignment: the widest aligned store that fits,
// at most four per call
__device__ __forceinline__ void store_narrow(unsigned char* p, uint64_t lo, uint64_t hi, int len) {
  while (len > 0) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    int k;
    if ((a & 7) == 0 && len >= 8) {
      *reinterpret_cast<uint64_t*>(p) = lo;
      k = 8;
    } else if ((a & 3) == 0 && len >= 4) {
      *reinterpret_cast<uint32_t*>(p) = static_cast<uint32_t>(lo);
      k = 4;
    } else if ((a & 1) == 0 && len >= 2) {
      *reinterpret_cast<uint16_t*>(p) = static_cast<uint16_t>(lo);
      k = 2;
    } else {
      *p = static_cast<unsigned char>(lo);
      k = 1;
    }
    if (k == 8) {
      lo = hi;
      hi = 0;
    } else {
      lo = (lo >> (8 * k)) | (hi << (64 - 8 * k));
      hi >>= 8 * k;
    }
    p += k;
    len -= k;
  }
}

// Workgroup (n, row class k, split z).  The rows r = k (mod 16) of a plane start at one address modulo 16, so they share
// one cut into a head (up to the first 16-byte boundary), 16-byte segments and a tail.  A thread owns one segment (16
// consecutive pixels of a row) for all its rows: the column taps are computed once and stay in registers; as many row
// groups as fit into the workgroup run side by side.  Every byte of the plane is written once, zeros included.
template <typename T>
__global__ void __launch_bounds__(kBlock)
paste_masks_kernel(const T* __restrict__ masks, const float* __restrict__ boxes, const int* __restrict__ det_hw,
                   const int64_t* __restrict__ out_offset, int M, int pad, float scale, float threshold,
                   unsigned char* __restrict__ out) {
  DETOPS_DYNAMIC_LDS(float, smap);
  const int64_t n = blockIdx.x;
  const int P = M + 2 * pad, S = P + 1;
  const Det d = load_det(boxes, det_hw, n, P, scale);
  const int cls = blockIdx.y % kRowClasses, split = blockIdx.y / kRowClasses, nsplit = gridDim.y / kRowClasses;
  if (d.W <= 0 || cls >= d.H) return;
  const bool any = d.cx1 > d.cx0;
  if (any) {
    stage_map(masks + n * M * M, M, pad, smap);
    __syncthreads();
  }
  unsigned char* plane = out + out_offset[n];
  const int W = d.W;
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(plane + static_cast<int64_t>(cls) * W);
  const int head = min(static_cast<int>((0 - a0) & (kSeg - 1)), W);
  const int nbody = (W - head) / kSeg;
  const int items = nbody + 2;                        // head, body segments, tail (head and tail may be empty)
  const int per = min(items, kBlock);                 // threads of a row group
  const int G = kBlock / per;
  const int g = threadIdx.x / per, t = threadIdx.x % per;
  if (g >= G) return;
  for (int s = t; s < items; s += per) {
    int c0, len;
    if (s == 0) { c0 = 0; len = head; }
    else if (s <= nbody) { c0 = head + (s - 1) * kSeg; len = kSeg; }
    else { c0 = head + nbody * kSeg; len = W - c0; }
    if (len == 0) continue;
    const bool col_hit = any && c0 < d.cx1 && c0 + len > d.cx0;
    Tap tx[kSeg];
    unsigned inside = 0;                              // bit j: column c0 + j is in the window (and in the segment)
    if (col_hit) {
#pragma unroll
      for (int j = 0; j < kSeg; ++j) {
        const int c = c0 + j;
        tx[j] = axis_tap(min(max(c - d.x1, 0), d.w - 1), P, d.w, d.rx);
        inside |= (j < len && c >= d.cx0 && c < d.cx1) ? (1u << j) : 0u;
      }
    }
    for (int64_t r = cls + kRowClasses * (g + static_cast<int64_t>(G) * split); r < d.H;
         r += static_cast<int64_t>(kRowClasses) * G * nsplit) {
      uint32_t q[4] = {0u, 0u, 0u, 0u};
      if (col_hit && r >= d.ry0 && r < d.ry1) {
        const Tap ty = axis_tap(static_cast<int>(r) - d.y1, P, d.h, d.ry);
#pragma unroll
        for (int j = 0; j < kSeg; ++j) {
          const uint32_t bit = (mask_bit(smap, S, ty, tx[j], threshold) ? 1u : 0u) & (inside >> j);
          q[j / 4] |= bit << (8 * (j % 4));
        }
      }
      unsigned char* p = plane + r * W + c0;
      if (len == kSeg)
        *reinterpret_cast<uint4*>(p) = make_uint4(q[0], q[1], q[2], q[3]);
      else
        store_narrow(p, q[0] | (static_cast<uint64_t>(q[1]) << 32), q[2] | (static_cast<uint64_t>(q[3]) << 32), len);
    }
  }
}

// ---------------------------------------------------------------------------------------------------- run lengths
// Column-major position of pixel (r, c) is c * H + r.  A TRANSITION is a position whose bit differs from its
// predecessor's (the predecessor of position 0 is a zero).  With the transitions p_0 < p_1 < ... the counts are
// p_0, p_1 - p_0, ..., H * W - p_last: canonical by construction (only the first can be 0).  Ones exist only in the
// window, so transitions exist only at window pixels and at the position right behind a window column's last pixel.
constexpr int kRleCols = 32;                    // window columns per workgroup: a wave per column, lanes over the rows
constexpr int kRleWaves = kBlock / kWave;

struct RleWorkspace {
  int* col_count;   // [N, max_w]  transitions of a column; after the scan: transitions before it
  int* col_last;    // [N, max_w]  position of a column's last transition (-1: none); after the scan: the last one before it (0: none)
  int* det_last;    // [N]         position of the detection's last transition (0: none)
  int* det_runs;    // [N]         counts of the detection = transitions + 1
};

__host__ __device__ inline RleWorkspace rle_workspace(void* ws, int64_t N, int64_t max_w) {
  RleWorkspace r;
  r.col_count = static_cast<int*>(ws);
  r.col_last = r.col_count + N * max_w;
  r.det_last = r.col_last + N * max_w;
  r.det_runs = r.det_last + N;
  return r;
}

// kWrite = false: col_count / col_last of every column < max_w.  kWrite = true: the counts, from the scanned tables.
template <typename T, bool kWrite>
__global__ void __launch_bounds__(kBlock)
paste_masks_rle_kernel(const T* __restrict__ masks, const float* __restrict__ boxes, const int* __restrict__ det_hw, int M,
                       int pad, float scale, float threshold, int max_w, RleWorkspace ws,
                       const int64_t* __restrict__ run_offset, int* __restrict__ counts) {
  DETOPS_DYNAMIC_LDS(float, smap);
  const int64_t n = blockIdx.x;
  const int P = M + 2 * pad, S = P + 1;
  Det d = load_det(boxes, det_hw, n, P, scale);
  const int H = max(d.H, 0), W = max(d.W, 0);
  const int cx1 = min(d.cx1, max_w), cx0 = min(d.cx0, cx1);   // max_w >= W by contract; a smaller one must not overrun
  const int c_begin = blockIdx.y * kRleCols, c_end = min(c_begin + kRleCols, max_w);
  int* col_count = ws.col_count + n * max_w;
  int* col_last = ws.col_last + n * max_w;
  if (!kWrite) {
    const int c = c_begin + threadIdx.x;
    if (c < c_end && (c < cx0 || c >= cx1)) {
      col_count[c] = 0;
      col_last[c] = -1;
    }
  } else if (blockIdx.y == 0 && threadIdx.x == 0) {
    counts[run_offset[n + 1] - 1] = static_cast<int>(static_cast<int64_t>(H) * W - ws.det_last[n]);
  }
  if (c_begin >= cx1 || c_end <= cx0) return;
  stage_map(masks + n * M * M, M, pad, smap);
  __syncthreads();
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const bool full = d.ry0 == 0 && d.ry1 == H;     // the window spans the full height: columns chain into each other
  const int64_t total = static_cast<int64_t>(H) * W;
  for (int c = c_begin + wave; c < min(c_end, cx1); c += kRleWaves) {
    if (c < cx0) continue;
    const Tap tx = axis_tap(c - d.x1, P, d.w, d.rx);
    // the bit in front of the column's first window pixel: a zero above the window, or the previous column's last pixel
    int prev = 0;
    if (full && c > cx0)
      prev = mask_bit(smap, S, axis_tap(H - 1 - d.y1, P, d.h, d.ry), axis_tap(c - 1 - d.x1, P, d.w, d.rx), threshold);
    const int64_t p_col = static_cast<int64_t>(c) * H;
    int cnt = 0;
    int64_t last = kWrite ? col_last[c] : -1;
    const int64_t base = kWrite ? run_offset[n] + col_count[c] : 0;
    for (int r0 = d.ry0; r0 <= d.ry1; r0 += kWave) {     // row ry1 is the position behind the column
      const int r = r0 + lane;
      bool valid = r <= d.ry1, bit = false;
      if (r < d.ry1)
        bit = mask_bit(smap, S, axis_tap(r - d.y1, P, d.h, d.ry), tx, threshold);
      else if (r == d.ry1 && ((full && c + 1 < cx1) || p_col + r >= total))
        valid = false;      // the next column's first pixel (that column compares it), or the end of the plane
      int up = __shfl_up(static_cast<int>(bit), 1);
      if (lane == 0) up = prev;
      const bool tr = valid && (static_cast<int>(bit) != up);
      const uint64_t m = __ballot(tr);
      if (kWrite && tr) {
        const uint64_t below = m & ((1ull << lane) - 1ull);
        const int64_t before = below ? p_col + r0 + (63 - __clzll(below)) : last;
        counts[base + cnt + __popcll(below)] = static_cast<int>(p_col + r - before);
      }
      if (m) {
        cnt += __popcll(m);
        last = p_col + r0 + (63 - __clzll(m));
      }
      prev = __shfl(static_cast<int>(bit), kWave - 1);
    }
    if (!kWrite && lane == 0) {
      col_count[c] = cnt;
      col_last[c] = static_cast<int>(last);
    }
  }
}

// One wave per detection: exclusive sum of col_count and exclusive running maximum of col_last (positions grow with the
// column; 0 = no transition yet, which makes the first count p_0 - 0), both in place; the detection's totals.
__global__ void __launch_bounds__(kWave)
paste_masks_rle_scan_kernel(RleWorkspace ws, int max_w) {
  const int64_t n = blockIdx.x;
  const int lane = threadIdx.x;
  int* col_count = ws.col_count + n * max_w;
  int* col_last = ws.col_last + n * max_w;
  int sum = 0, last = 0;
  for (int c0 = 0; c0 < max_w; c0 += kWave) {
    const int c = c0 + lane;
    const int v = c < max_w ? col_count[c] : 0;
    const int l = c < max_w ? col_last[c] : -1;
    const int s = wave_scan(v), m = wave_scan(l, [](int a, int b) { return max(a, b); });
    int m_before = __shfl_up(m, 1);
    if (lane == 0) m_before = -1;
    if (c < max_w) {
      col_count[c] = sum + s - v;
      col_last[c] = max(last, m_before);
    }
    sum += __shfl(s, kWave - 1);
    last = max(last, __shfl(m, kWave - 1));
  }
  if (lane == 0) {
    ws.det_last[n] = last;
    ws.det_runs[n] = sum + 1;
  }
}

// run_offset [N + 1] = exclusive sum of det_runs (one wave)
__global__ void __launch_bounds__(kWave)
paste_masks_rle_offsets_kernel(RleWorkspace ws, int N, int64_t* __restrict__ run_offset) {
  const int lane = threadIdx.x;
  const int64_t total = scan_tiles<kWave>(
      N, [&](int i) { return static_cast<int64_t>(ws.det_runs[i]); }, [&](int i, int64_t before) { run_offset[i] = before; });
  if (lane == 0) run_offset[N] = total;
}

int check_args(int N, int M, int padding) {
  if (padding < 1 || M <= 0 || N < 0) return DETOPS_EINVAL;
  if (M > kMaxPadded || padding > kMaxPadded || M + 2 * padding > kMaxPadded) return DETOPS_EINVAL;
  return 0;
}

// `scale` of expand_masks as the tensor multiply sees it: the Python float (double) rounded to fp32
float expand_scale(int M, int padding) { return static_cast<float>(static_cast<double>(M + 2 * padding) / M); }

size_t map_lds_bytes(int M, int padding) {
  const size_t S = static_cast<size_t>(M + 2 * padding + 1);
  return S * S * sizeof(float);
}

}  // namespace

DETOPS_API int detops_paste_masks(const void* masks, int dtype, const float* boxes, const int32_t* det_hw,
                                  const int64_t* out_offset, int N, int M, int padding, float threshold, unsigned char* out,
                                  detops_stream_t stream) {
  if (const int rc = check_args(N, M, padding)) return rc;
  if (N == 0) return 0;
  if (!masks || !boxes || !det_hw || !out_offset || !out) return DETOPS_EINVAL;
  // 16 row classes per detection; a batch of few detections splits each class further, up to 8 workgroups per CU (the
  // cap for a memory-bound grid) and at most 16 ways (an 800-row plane then still has 3 rows per class and split)
  const int64_t classes = static_cast<int64_t>(kRowClasses) * N;
  const int nsplit = classes >= kNumCU * 8 ? 1 : static_cast<int>(kNumCU * 8 / classes) < 16 ? static_cast<int>(kNumCU * 8 / classes) : 16;
  const dim3 grid(static_cast<unsigned>(N), static_cast<unsigned>(kRowClasses * nsplit));
  return dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(paste_masks_kernel<T>, grid, dim3(kBlock), map_lds_bytes(M, padding), as_stream(stream),
                       static_cast<const T*>(masks), boxes, det_hw, out_offset, M, padding, expand_scale(M, padding),
                       threshold, out);
    return launch_status();
  });
}

DETOPS_API size_t detops_paste_masks_rle_workspace_bytes(int N, int max_w) {
  if (N <= 0 || max_w <= 0) return 0;
  return (2 * static_cast<size_t>(N) * max_w + 2 * static_cast<size_t>(N)) * sizeof(int);
}

DETOPS_API int detops_paste_masks_rle_count(const void* masks, int dtype, const float* boxes, const int32_t* det_hw, int N,
                                            int M, int padding, float threshold, int max_w, int64_t* run_offset,
                                            void* workspace, size_t workspace_bytes, detops_stream_t stream) {
  if (const int rc = check_args(N, M, padding)) return rc;
  if (max_w <= 0 || (max_w + kRleCols - 1) / kRleCols > 65535) return DETOPS_EINVAL;
  if (!run_offset) return DETOPS_EINVAL;
  hipStream_t st = as_stream(stream);
  if (N == 0) {
    DETOPS_HIP_TRY(hipMemsetAsync(run_offset, 0, sizeof(int64_t), st));
    return 0;
  }
  if (!masks || !boxes || !det_hw || !workspace) return DETOPS_EINVAL;
  if (workspace_bytes < detops_paste_masks_rle_workspace_bytes(N, max_w)) return DETOPS_EWORKSPACE;
  const RleWorkspace ws = rle_workspace(workspace, N, max_w);
  const dim3 grid(static_cast<unsigned>(N), static_cast<unsigned>((max_w + kRleCols - 1) / kRleCols));
  const int rc = dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((paste_masks_rle_kernel<T, false>), grid, dim3(kBlock), map_lds_bytes(M, padding), st,
                       static_cast<const T*>(masks), boxes, det_hw, M, padding, expand_scale(M, padding), threshold, max_w, ws,
                       static_cast<const int64_t*>(nullptr), static_cast<int*>(nullptr));
    return launch_status();
  });
  if (rc) return rc;
  hipLaunchKernelGGL(paste_masks_rle_scan_kernel, dim3(static_cast<unsigned>(N)), dim3(kWave), 0, st, ws, max_w);
  hipLaunchKernelGGL(paste_masks_rle_offsets_kernel, dim3(1), dim3(kWave), 0, st, ws, N, run_offset);
  return launch_status();
}

DETOPS_API int detops_paste_masks_rle_write(const void* masks, int dtype, const float* boxes, const int32_t* det_hw, int N,
                                            int M, int padding, float threshold, int max_w, const int64_t* run_offset,
                                            int32_t* counts, void* workspace, size_t workspace_bytes,
                                            detops_stream_t stream) {
  if (const int rc = check_args(N, M, padding)) return rc;
  if (max_w <= 0 || (max_w + kRleCols - 1) / kRleCols > 65535) return DETOPS_EINVAL;
  if (N == 0) return 0;
  if (!masks || !boxes || !det_hw || !run_offset || !counts || !workspace) return DETOPS_EINVAL;
  if (workspace_bytes < detops_paste_masks_rle_workspace_bytes(N, max_w)) return DETOPS_EWORKSPACE;
  const RleWorkspace ws = rle_workspace(workspace, N, max_w);
  const dim3 grid(static_cast<unsigned>(N), static_cast<unsigned>((max_w + kRleCols - 1) / kRleCols));
  return dispatch_dtype(dtype, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((paste_masks_rle_kernel<T, true>), grid, dim3(kBlock), map_lds_bytes(M, padding), as_stream(stream),
                       static_cast<const T*>(masks), boxes, det_hw, M, padding, expand_scale(M, padding), threshold, max_w, ws,
                       run_offset, counts);
    return launch_status();
  });
}
