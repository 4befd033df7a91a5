// color_jitter.hip — colour jitter of the raw images of a batch, in place on the device, for gfx950 (MI355X).
//
//   detops_color_jitter_u8   brightness, contrast, saturation and hue of every image of a RawImageBatch's buffer, in the
//                            image's own order (reference data/transforms/transforms.py ColorJitter = torchvision's over
//                            Pillow), before detops_image_batch_u8 reads the bytes
//
// The arithmetic is Pillow's, restated in include/detops.h and checked against it byte for byte: three blends in fp32
// against a degenerate byte, convert("L") in integers, the HSV round trip in fp32 / fp64.  Nothing here may be contracted
// into an FMA, hence the pragma for the whole file.
//
// Work split: the buffer's flat byte range is cut into chunks of kChunk bytes, a workgroup per chunk; the shared offsets
// lookup finds the images a chunk meets.  Inside an image, pixels are owned in units: the head (up to 15 pixels, until a
// pixel starts on a 16-byte boundary: 3 p = -address mod 16), then groups of 16 pixels = 48 aligned bytes that move as
// three 16-byte accesses, then the tail (under 16 pixels).  A unit belongs to the chunk that holds its first byte, so
// every byte of a jittered image is written exactly once, and nothing else is written.
//
// Two launches at most: contrast blends against the image's mean grey level AS IT IS when the step is reached, so a sum
// pass first applies the steps in front of contrast on the fly (writing nothing) and adds L of every pixel: 32-bit inside
// a workgroup (a chunk holds 4096 pixels), then one 64-bit integer atomic per (workgroup, image) into the workspace.
// Integer sums: any order gives the same bits.  The apply pass forms the mean in fp64 and runs every step.
#include "detops_dtype.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBlock = 256;
constexpr int kGroupPix = 16, kGroupBytes = 3 * kGroupPix;     // 48 bytes: three uint4
constexpr int64_t kChunk = static_cast<int64_t>(kBlock) * kGroupBytes;
constexpr int kGeom = 5;                   // int32 per image: h, w, oh, ow, flip bits (image_prep.hip's record)
constexpr int kRec = DETOPS_COLOR_JITTER_FIELDS, kSteps = DETOPS_COLOR_JITTER_MAX_STEPS;
enum { kNone = 0, kBrightness = 1, kContrast = 2, kSaturation = 3, kHue = 4 };
static_assert(kRec == 2 * kSteps, "a parameter per step");

__host__ __device__ inline float bits_float(int32_t b) {
  union { int32_t i; float f; } u;
  u.i = b;
  return u.f;
}

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// Image.blend(degenerate, image, a) of one byte.  For 0 <= a <= 1 the value lies between d and x (both roundings are
// monotone), so the clip Pillow leaves out there changes nothing and one form serves every factor.
__device__ __forceinline__ int blend(int d, int x, float a) {
  const float t = static_cast<float>(d) + a * static_cast<float>(x - d);
  return t <= 0.f ? 0 : (t >= 255.f ? 255 : static_cast<int>(t));
}

__device__ __forceinline__ int luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// round half away from zero of x >= 0, clipped to a byte
__device__ __forceinline__ int round8(double x) {
  double r = floor(x);
  if (x - r >= 0.5) r = r + 1.0;
  return clip8(static_cast<int>(r));
}

__device__ __forceinline__ void hue_step(int& r, int& g, int& b, int k) {
  const int maxc = max(r, max(g, b)), minc = min(r, min(g, b)), V = maxc;
  int H = 0, S = 0;
  if (minc != maxc) {
    const float cr = static_cast<float>(maxc - minc);
    const float s = cr / static_cast<float>(maxc);
    const float rc = static_cast<float>(maxc - r) / cr;
    const float gc = static_cast<float>(maxc - g) / cr;
    const float bc = static_cast<float>(maxc - b) / cr;
    float h;
    if (r == maxc) {
      h = bc - gc;
    } else if (g == maxc) {
      double t = 2.0 + static_cast<double>(rc);
      t = t - static_cast<double>(bc);
      h = static_cast<float>(t);
    } else {
      double t = 4.0 + static_cast<double>(gc);
      t = t - static_cast<double>(rc);
      h = static_cast<float>(t);
    }
    double hd = static_cast<double>(h) / 6.0;
    hd = hd + 1.0;                                       // in [5/6, 11/6]
    hd = hd - floor(hd);                                 // fmod(hd, 1.0): the difference is exact
    h = static_cast<float>(hd);
    H = clip8(static_cast<int>(static_cast<double>(h) * 255.0));
    S = clip8(static_cast<int>(static_cast<double>(s) * 255.0));
  }
  H = (H + k) & 255;
  if (S == 0) {
    r = g = b = V;
    return;
  }
  double h6 = static_cast<double>(H) * 6.0;
  h6 = h6 / 255.0;
  const int i = static_cast<int>(floor(h6));
  const double f = static_cast<double>(static_cast<float>(h6 - static_cast<double>(i)));
  const double fs = static_cast<double>(static_cast<float>(static_cast<double>(S) / 255.0));
  const double v = static_cast<double>(V);
  double e = 1.0 - fs;
  const int p = round8(v * e);
  e = fs * f;
  e = 1.0 - e;
  const int q = round8(v * e);
  e = 1.0 - f;
  e = fs * e;
  e = 1.0 - e;
  const int t = round8(v * e);
  switch (i % 6) {
    case 0: r = V; g = t; b = p; break;
    case 1: r = q; g = V; b = p; break;
    case 2: r = p; g = V; b = t; break;
    case 3: r = p; g = q; b = V; break;
    case 4: r = t; g = p; b = V; break;
    default: r = V; g = p; b = q; break;
  }
}

// the steps of one image, as the kernel holds them: the codes a byte each, in order
struct Steps {
  int codes, n, contrast_at;                 // contrast_at: the index of the contrast step, n when there is none
  int par[kSteps];
};

// The list ends at the first code that is no operation (the host refuses such records; the device copy only has to be safe).
__device__ __forceinline__ Steps load_steps(const int32_t* rec) {
  Steps s;
  s.codes = 0;
  s.n = 0;
  bool open = true;
#pragma unroll
  for (int i = 0; i < kSteps; ++i) {
    const int c = rec[i];
    s.par[i] = rec[kSteps + i];
    open = open && c >= kBrightness && c <= kHue;
    if (open) {
      s.codes |= c << (8 * i);
      s.n = i + 1;
    }
  }
  s.contrast_at = s.n;
#pragma unroll
  for (int i = kSteps - 1; i >= 0; --i)
    if (i < s.n && ((s.codes >> (8 * i)) & 255) == kContrast) s.contrast_at = i;
  return s;
}

// The first `nrun` steps on one pixel (R | G << 8 | B << 16); m: the grey level contrast blends against.  One copy of the
// code for the sixteen pixels of a group and the narrow paths: the fp64 hue path is long.
__device__ __noinline__ uint32_t jitter_pixel(uint32_t px, int codes, int nrun, int par0, int par1, int par2, int par3,
                                              int m) {
  int r = px & 255u, g = (px >> 8) & 255u, b = (px >> 16) & 255u;
  for (int i = 0; i < nrun; ++i) {
    const int code = (codes >> (8 * i)) & 255;
    const int par = i == 0 ? par0 : (i == 1 ? par1 : (i == 2 ? par2 : par3));
    if (code == kHue) {
      hue_step(r, g, b, par & 255);
    } else {
      const float a = bits_float(par);
      const int l = luma(r, g, b);
      const int dr = code == kBrightness ? 0 : (code == kContrast ? m : l);
      r = blend(dr, r, a);
      g = blend(dr, g, a);
      b = blend(dr, b, a);
    }
  }
  return static_cast<uint32_t>(r) | (static_cast<uint32_t>(g) << 8) | (static_cast<uint32_t>(b) << 16);
}

__device__ __forceinline__ uint32_t byte_of(const uint32_t (&w)[12], int idx) { return (w[idx >> 2] >> (8 * (idx & 3))) & 255u; }

// The pixels [pa, pb) of an image of npix pixels at `img` that this workgroup owns, by units (see the head of the file):
// f(px) -> px for each; with kWrite the result goes back.  Every access lies inside [img, img + 3 npix).
template <bool kWrite, typename F>
__device__ __forceinline__ void visit(uint8_t* img, int64_t npix, int64_t pa, int64_t pb, F&& f) {
  const int tid = threadIdx.x;
  int64_t p0 = ((16 - static_cast<int>(reinterpret_cast<uintptr_t>(img) & 15)) * 11) & 15;   // 3 * 11 = 1 mod 16
  p0 = p0 < npix ? p0 : npix;
  const int64_t ng = (npix - p0) / kGroupPix, tail = p0 + ng * kGroupPix;
  const int64_t g_lo = pa <= p0 ? 0 : (pa - p0 + kGroupPix - 1) / kGroupPix;
  int64_t g_hi = pb <= p0 ? 0 : (pb - p0 + kGroupPix - 1) / kGroupPix;
  g_hi = g_hi < ng ? g_hi : ng;
  for (int64_t g = g_lo + tid; g < g_hi; g += kBlock) {
    uint4* q = reinterpret_cast<uint4*>(img + 3 * (p0 + g * kGroupPix));
    const uint4 a = q[0], b = q[1], c = q[2];
    const uint32_t w[12] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w};
    uint32_t o[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < kGroupPix; ++j) {
      const uint32_t px = f(byte_of(w, 3 * j) | (byte_of(w, 3 * j + 1) << 8) | (byte_of(w, 3 * j + 2) << 16));
      if (kWrite) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) o[(3 * j + ch) >> 2] |= ((px >> (8 * ch)) & 255u) << (8 * ((3 * j + ch) & 3));
      }
    }
    if (kWrite) {
      q[0] = make_uint4(o[0], o[1], o[2], o[3]);
      q[1] = make_uint4(o[4], o[5], o[6], o[7]);
      q[2] = make_uint4(o[8], o[9], o[10], o[11]);
    }
  }
  // head [0, p0) and tail [tail, npix): a pixel per thread, byte accesses
  const int64_t h_hi = pb < p0 ? pb : p0, n_head = h_hi > pa ? h_hi - pa : 0;
  const int64_t t_lo = pa > tail ? pa : tail, n_tail = pb > t_lo ? pb - t_lo : 0;
  for (int64_t i = tid; i < n_head + n_tail; i += kBlock) {
    uint8_t* q = img + 3 * (i < n_head ? pa + i : t_lo + (i - n_head));
    const uint32_t px = f(static_cast<uint32_t>(q[0]) | (static_cast<uint32_t>(q[1]) << 8) | (static_cast<uint32_t>(q[2]) << 16));
    if (kWrite) {
      q[0] = static_cast<uint8_t>(px & 255u);
      q[1] = static_cast<uint8_t>((px >> 8) & 255u);
      q[2] = static_cast<uint8_t>((px >> 16) & 255u);
    }
  }
}

// grid ceil(raw_bytes / kChunk).  kSum: the sum pass (images with a contrast step; nothing written to raw); else the
// apply pass.  An image whose device record the kernel cannot serve (sizes below 1, bytes outside `raw`) is skipped: the
// entry point validates the host copy, the kernel only has to stay inside the buffer if the two copies differ.
template <bool kSum>
__global__ void __launch_bounds__(kBlock)
color_jitter_kernel(uint8_t* __restrict__ raw, int64_t raw_bytes, const int64_t* __restrict__ offsets,
                    const int32_t* __restrict__ geom, const int32_t* __restrict__ jitter, int N,
                    unsigned long long* __restrict__ sums) {
  __shared__ int red[kBlock / kWave];
  const int64_t lo = static_cast<int64_t>(blockIdx.x) * kChunk;
  const int64_t hi = lo + kChunk < raw_bytes ? lo + kChunk : raw_bytes;
  for (int img = last_at_or_below(offsets, N, lo); img < N; ++img) {       // (everything here is uniform over the workgroup)
    const int64_t base = offsets[img];
    if (base >= hi) break;
    const int64_t h = geom[static_cast<int64_t>(img) * kGeom], w = geom[static_cast<int64_t>(img) * kGeom + 1];
    if (base < 0 || h < 1 || w < 1 || h * w > (raw_bytes - base) / 3) continue;
    const int64_t npix = h * w;
    const Steps s = load_steps(jitter + static_cast<int64_t>(img) * kRec);
    if (s.n == 0 || (kSum && s.contrast_at == s.n)) continue;
    int64_t pa = lo <= base ? 0 : (lo - base + 2) / 3, pb = (hi - base + 2) / 3;   // pixels whose first byte is in [lo, hi)
    pa = pa < npix ? pa : npix;
    pb = pb < npix ? pb : npix;
    if (pa >= pb) continue;
    if (kSum) {
      int part = 0;
      visit<false>(raw + base, npix, pa, pb, [&](uint32_t px) {
        if (s.contrast_at > 0) px = jitter_pixel(px, s.codes, s.contrast_at, s.par[0], s.par[1], s.par[2], s.par[3], 0);
        part += luma(px & 255u, (px >> 8) & 255u, (px >> 16) & 255u);
        return px;
      });
      part = block_sum<kBlock>(part, red);
      if (threadIdx.x == 0 && part) atomicAdd(&sums[img], static_cast<unsigned long long>(part));
      __syncthreads();                                   // `red` is free for the next image
    } else {
      int m = 0;
      if (s.contrast_at < s.n && sums) {
        const double mean = static_cast<double>(static_cast<int64_t>(sums[img])) / static_cast<double>(npix);
        m = clip8(static_cast<int>(mean + 0.5));
      }
      visit<true>(raw + base, npix, pa, pb, [&](uint32_t px) {
        return jitter_pixel(px, s.codes, s.n, s.par[0], s.par[1], s.par[2], s.par[3], m);
      });
    }
  }
}

}  // namespace

DETOPS_API int detops_color_jitter_u8(uint8_t* raw, int64_t raw_bytes, const int64_t* offsets, const int32_t* geom,
                                      const int32_t* geom_host, const int32_t* jitter, const int32_t* jitter_host, int N,
                                      void* workspace, size_t workspace_bytes, detops_stream_t stream) {
  if (N < 0 || raw_bytes < 0) return DETOPS_EINVAL;
  if (N == 0) return 0;
  if (!raw || !offsets || !geom || !geom_host || !jitter || !jitter_host) return DETOPS_EINVAL;
  bool any = false, contrast = false;
  for (int i = 0; i < N; ++i) {
    const int32_t* g = geom_host + static_cast<int64_t>(i) * kGeom;
    const int32_t* r = jitter_host + static_cast<int64_t>(i) * kRec;
    if (g[0] < 1 || g[1] < 1) return DETOPS_EINVAL;
    unsigned seen = 0;
    bool open = true;
    for (int k = 0; k < kSteps; ++k) {
      const int c = r[k];
      if (c == kNone) {
        open = false;
        continue;
      }
      if (!open || c < kBrightness || c > kHue || (seen & (1u << c))) return DETOPS_EINVAL;   // also a code after the list's end
      seen |= 1u << c;
      const int32_t par = r[kSteps + k];
      if (c == kHue ? (par < 0 || par > 255) : ((par & 0x7f800000) == 0x7f800000)) return DETOPS_EINVAL;
      any = true;
      contrast = contrast || c == kContrast;
    }
  }
  if (!any || raw_bytes == 0) return 0;
  const int64_t chunks = ceil_div64(raw_bytes, kChunk);
  if (chunks > 0x7fffffff) return DETOPS_EINVAL;
  hipStream_t st = as_stream(stream);
  unsigned long long* sums = static_cast<unsigned long long*>(workspace);
  if (contrast) {
    if (!workspace) return DETOPS_EINVAL;
    if (workspace_bytes < static_cast<size_t>(N) * sizeof(unsigned long long)) return DETOPS_EWORKSPACE;
    DETOPS_HIP_TRY(hipMemsetAsync(sums, 0, static_cast<size_t>(N) * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(color_jitter_kernel<true>, dim3(static_cast<unsigned>(chunks)), dim3(kBlock), 0, st, raw, raw_bytes,
                       offsets, geom, jitter, N, sums);
    const int rc = launch_status();
    if (rc) return rc;
  }
  hipLaunchKernelGGL(color_jitter_kernel<false>, dim3(static_cast<unsigned>(chunks)), dim3(kBlock), 0, st, raw, raw_bytes,
                     offsets, geom, jitter, N, sums);
  return launch_status();
}
