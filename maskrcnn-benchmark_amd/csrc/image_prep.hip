// image_prep.hip — the input path of a batch on the device, for gfx950 (MI355X).
//
//   detops_image_batch_u8   raw RGB uint8 HWC images of a batch -> the zero-padded fp32 batch tensor the backbone reads
//                           (reference data/transforms/transforms.py Resize, RandomHorizontalFlip, RandomVerticalFlip,
//                           ToTensor, Normalize and structures/image_list.py to_image_list), one launch for the batch
//
// The resize is Pillow's bilinear resize restated in include/detops.h: per axis and output index a first tap, a tap
// count and 22-bit integer coefficients made in fp64; the horizontal pass first, rounded and clipped to uint8, then the
// vertical pass over those bytes.  A workgroup owns a tile of kTileH x kTileW elements of one image's padded output plane.
// It makes the taps of its columns and rows once (fp64, a thread per column / row), stages the horizontally resampled
// source rows its output rows reach as packed uint8 pixels in LDS, and resamples vertically from LDS: a thread makes four
// neighbouring pixels of one row, so the staged row is read 16 bytes at a time and the fp32 result leaves as 16-byte
// stores (three per thread in either layout).  Flips are an index reversal where the taps are made.  Every element of the
// output is written exactly once, the padding zeros included.
#include "detops_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kTileW = 64;                 // output columns of a tile: 16 threads x 4 pixels
constexpr int kTileH = 16;                 // output rows of a tile
constexpr int kPix = 4;                    // pixels per thread
constexpr int kMaxK = DETOPS_IMAGE_PREP_MAX_KSIZE;
constexpr int kBits = 22;                  // Pillow's PRECISION_BITS = 32 - 8 - 2
constexpr int kGeom = 5;                   // int32 per image: h, w, oh, ow, flip bits
static_assert(kBlock == kTileH * (kTileW / kPix), "a thread per four pixels of the tile");
static_assert(kTileW + kTileH <= kBlock, "a thread per column and per row makes the taps");

// the filter's tap budget of one axis: ceil(max(in / out, 1)) * 2 + 1 within kMaxK
__host__ __device__ inline bool axis_served(int in, int out) {
  return static_cast<int64_t>(in) <= static_cast<int64_t>((kMaxK - 1) / 2) * static_cast<int64_t>(out);
}

// Taps of output index xx of an axis resampled from `in` to `out` elements: *lo, *n, k[0 .. n).  An axis that keeps its
// size is not resampled: its single tap 2^22 hands the byte through ((2^21 + v * 2^22) >> 22 == v).
__device__ __forceinline__ void axis_taps(int in, int out, int xx, int* lo, int* n, int* k) {
#pragma clang fp contract(off)
  if (in == out) {
    *lo = xx;
    *n = 1;
    k[0] = 1 << kBits;
    return;
  }
  const double scale = static_cast<double>(in) / static_cast<double>(out);
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = fs;
  const double center = (static_cast<double>(xx) + 0.5) * scale;
  const double ss = 1.0 / fs;
  double e = center - support;
  e = e + 0.5;
  int xmin = static_cast<int>(e);
  xmin = xmin < 0 ? 0 : xmin;
  e = center + support;
  e = e + 0.5;
  int xmax = static_cast<int>(e);
  xmax = xmax > in ? in : xmax;
  const int cnt = min(max(xmax - xmin, 0), kMaxK);
  auto weight = [&](int x) {
    double a = static_cast<double>(x + xmin) - center;
    a = a + 0.5;
    a = fabs(a * ss);
    return a < 1.0 ? 1.0 - a : 0.0;
  };
  double ww = 0.0;
  for (int x = 0; x < cnt; ++x) ww = ww + weight(x);
  for (int x = 0; x < cnt; ++x) {
    double w = weight(x);
    if (ww != 0.0) w = w / ww;
    w = w * 4194304.0;
    w = w + 0.5;
    k[x] = static_cast<int>(w);
  }
  *lo = xmin;
  *n = cnt;
}

__device__ __forceinline__ uint32_t clip8(int v) {
  v >>= kBits;
  return static_cast<uint32_t>(v < 0 ? 0 : (v > 255 ? 255 : v));
}

__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// LDS of a workgroup ahead of the staged rows
struct Tile {
  float table[3 * 256];
  int hlo[kTileW], hn[kTileW], hk[kTileW * kMaxK];
  int vlo[kTileH], vn[kTileH], vk[kTileH * kMaxK];
};
static_assert(sizeof(Tile) % 16 == 0, "the staged rows are read 16 bytes at a time");

// grid (ceil(Wp / kTileW), ceil(Hp / kTileH), N).  An image whose record the kernel cannot serve (sizes outside the batch,
// bytes outside `raw`, a tap budget beyond kMaxK) is written as zeros: the entry point rejects such a batch from the
// host copy of the records, the kernel only has to stay inside its buffers if the two copies differ.
__global__ void __launch_bounds__(kBlock)
image_batch_kernel(const uint8_t* __restrict__ raw, int64_t raw_bytes, const int64_t* __restrict__ offsets,
                   const int32_t* __restrict__ geom, const float* __restrict__ table, int bgr, int Hp, int Wp,
                   int channels_last, int max_rows, float* __restrict__ out) {
  DETOPS_DYNAMIC_LDS(uint32_t, lds);
  Tile* tile = reinterpret_cast<Tile*>(lds);
  uint32_t* stage = lds + sizeof(Tile) / sizeof(uint32_t);       // [max_rows][kTileW] pixels: R | G << 8 | B << 16
  const int img = blockIdx.z, y0 = blockIdx.y * kTileH, x0 = blockIdx.x * kTileW;
  const int tid = threadIdx.x, tx = tid % (kTileW / kPix), ty = tid / (kTileW / kPix);
  const int32_t* g = geom + static_cast<int64_t>(img) * kGeom;
  const int h = g[0], w = g[1], flip = g[4];
  int oh = g[2], ow = g[3];
  const int64_t off = offsets[img];
  const bool served = h >= 1 && w >= 1 && oh >= 1 && ow >= 1 && oh <= Hp && ow <= Wp && off >= 0 &&
                      off + static_cast<int64_t>(h) * w * 3 <= raw_bytes && axis_served(h, oh) && axis_served(w, ow);
  if (!served) oh = ow = 0;
  const int rows = min(max(oh - y0, 0), kTileH), cols = min(max(ow - x0, 0), kTileW);   // of the image inside this tile
  int smin = 0, nrows = 0;
  if (rows > 0 && cols > 0) {                                      // the same for every thread of the workgroup
    for (int i = tid; i < 3 * 256; i += kBlock) tile->table[i] = table[i];
    if (tid < cols) {
      const int x = x0 + tid;
      axis_taps(w, ow, (flip & 1) ? ow - 1 - x : x, &tile->hlo[tid], &tile->hn[tid], &tile->hk[tid * kMaxK]);
    } else if (tid >= kTileW && tid - kTileW < rows) {
      const int r = tid - kTileW, y = y0 + r;
      axis_taps(h, oh, (flip & 2) ? oh - 1 - y : y, &tile->vlo[r], &tile->vn[r], &tile->vk[r * kMaxK]);
    }
    __syncthreads();
    // the taps' bounds are monotone in the output index: the tile's first and last row span its source rows
    const int a = tile->vlo[0], b = tile->vlo[rows - 1];
    smin = min(a, b);
    nrows = min(max(a + tile->vn[0], b + tile->vn[rows - 1]) - smin, max_rows);
    const uint8_t* src = raw + off;
    for (int i = tid; i < nrows * kTileW; i += kBlock) {
      const int r = i / kTileW, c = i % kTileW;
      if (c >= cols) continue;
      const uint8_t* p = src + (static_cast<int64_t>(smin + r) * w + tile->hlo[c]) * 3;
      const int n = tile->hn[c];
      const int* k = &tile->hk[c * kMaxK];
      int s0 = 1 << (kBits - 1), s1 = s0, s2 = s0;
      for (int t = 0; t < n; ++t) {
        const int kt = k[t];
        s0 += static_cast<int>(p[3 * t]) * kt;
        s1 += static_cast<int>(p[3 * t + 1]) * kt;
        s2 += static_cast<int>(p[3 * t + 2]) * kt;
      }
      stage[i] = clip8(s0) | (clip8(s1) << 8) | (clip8(s2) << 16);
    }
    __syncthreads();
  }
  const int y = y0 + ty, x = x0 + tx * kPix;
  if (y >= Hp || x >= Wp) return;
  float v[3][kPix];                                                // [output channel][pixel]
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int j = 0; j < kPix; ++j) v[c][j] = 0.0f;
  if (ty < rows && tx * kPix < cols) {
    int s[kPix][3];
#pragma unroll
    for (int j = 0; j < kPix; ++j) s[j][0] = s[j][1] = s[j][2] = 1 << (kBits - 1);
    const int first = tile->vlo[ty] - smin, n = tile->vn[ty];
    const int* k = &tile->vk[ty * kMaxK];
    for (int t = 0; t < n; ++t) {
      if (first + t >= nrows) break;                               // never with the host's max_rows
      const uint4 q = *reinterpret_cast<const uint4*>(&stage[(first + t) * kTileW + tx * kPix]);
      const uint32_t px[kPix] = {q.x, q.y, q.z, q.w};
      const int kt = k[t];
#pragma unroll
      for (int j = 0; j < kPix; ++j) {
        s[j][0] += static_cast<int>(px[j] & 255u) * kt;
        s[j][1] += static_cast<int>((px[j] >> 8) & 255u) * kt;
        s[j][2] += static_cast<int>((px[j] >> 16) & 255u) * kt;
      }
    }
#pragma unroll
    for (int j = 0; j < kPix; ++j)
      if (tx * kPix + j < cols) {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c][j] = tile->table[c * 256 + clip8(s[j][bgr ? 2 - c : c])];
      }
  }
  const bool full = x + kPix <= Wp;
  if (channels_last) {                                             // [N, Hp, Wp, 3]: twelve consecutive floats
    float* p = out + ((static_cast<int64_t>(img) * Hp + y) * Wp + x) * 3;
    if (full && aligned16(p)) {
      float4* p4 = reinterpret_cast<float4*>(p);
      p4[0] = make_float4(v[0][0], v[1][0], v[2][0], v[0][1]);
      p4[1] = make_float4(v[1][1], v[2][1], v[0][2], v[1][2]);
      p4[2] = make_float4(v[2][2], v[0][3], v[1][3], v[2][3]);
    } else {
#pragma unroll
      for (int j = 0; j < kPix; ++j)
        if (x + j < Wp) {
#pragma unroll
          for (int c = 0; c < 3; ++c) p[3 * j + c] = v[c][j];
        }
    }
  } else {                                                         // [N, 3, Hp, Wp]: four floats in each plane
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float* p = out + ((static_cast<int64_t>(img) * 3 + c) * Hp + y) * Wp + x;
      if (full && aligned16(p)) {
        *reinterpret_cast<float4*>(p) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
      } else {
#pragma unroll
        for (int j = 0; j < kPix; ++j)
          if (x + j < Wp) p[j] = v[c][j];
      }
    }
  }
}

// source rows the kTileH output rows of a tile can reach: (kTileH - 1) * scale + 2 * support + 1 of the real line
int tile_rows(int h, int oh) {
  if (h == oh) return kTileH;
  const double scale = static_cast<double>(h) / static_cast<double>(oh), support = scale < 1.0 ? 1.0 : scale;
  return static_cast<int>((kTileH - 1) * scale + 2.0 * support) + 3;
}

}  // namespace

DETOPS_API int detops_image_batch_u8(const uint8_t* raw, int64_t raw_bytes, const int64_t* offsets, const int32_t* geom,
                                     const int32_t* geom_host, int N, const float* table, int bgr, int Hp, int Wp,
                                     int channels_last, float* out, detops_stream_t stream) {
  if (N < 0 || N > 65535 || Hp < 0 || Wp < 0 || raw_bytes < 0 || (Hp + kTileH - 1) / kTileH > 65535) return DETOPS_EINVAL;
  if (N == 0 || Hp == 0 || Wp == 0) return 0;
  if (!raw || !offsets || !geom || !geom_host || !table || !out) return DETOPS_EINVAL;
  int max_rows = 1;
  for (int i = 0; i < N; ++i) {
    const int32_t* g = geom_host + static_cast<int64_t>(i) * kGeom;
    if (g[0] < 1 || g[1] < 1 || g[2] < 1 || g[3] < 1 || g[2] > Hp || g[3] > Wp) return DETOPS_EINVAL;
    if (!axis_served(g[0], g[2]) || !axis_served(g[1], g[3])) return DETOPS_EINVAL;   // beyond DETOPS_IMAGE_PREP_MAX_KSIZE
    const int r = tile_rows(g[0], g[2]);
    max_rows = r > max_rows ? r : max_rows;
  }
  const size_t lds = sizeof(Tile) + static_cast<size_t>(max_rows) * kTileW * sizeof(uint32_t);
  const dim3 grid(static_cast<unsigned>((Wp + kTileW - 1) / kTileW), static_cast<unsigned>((Hp + kTileH - 1) / kTileH),
                  static_cast<unsigned>(N));
  hipLaunchKernelGGL(image_batch_kernel, grid, dim3(kBlock), lds, as_stream(stream), raw, raw_bytes, offsets, geom, table,
                     bgr ? 1 : 0, Hp, Wp, channels_last ? 1 : 0, max_rows, out);
  return launch_status();
}
