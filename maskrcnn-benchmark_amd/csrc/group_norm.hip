// group_norm.hip — GroupNorm (+ residual add) (+ ReLU) on channels-last activations, forward and backward, for gfx950
// (MI355X).  fp32 / fp16 / bf16 storage; statistics, gamma, beta and every sum in fp32.
//
// The activation is x[n][p][c]: N samples, HW rows (pixels), C channels, the channel the fastest index.  A group is
// D = C / G ADJACENT channels of every row of one sample, so its HW * D elements are strided through the whole sample.
//
// One thread layout serves every kernel here.  A workgroup of 256 threads covers a COLUMN TILE of `cols_tile` vector
// columns (a vector = V consecutive channels moved as one access) and `rpp = 256 / cols_tile` rows per pass: thread
// (tx, ty) owns vector column tx of the tile and rows ty, ty + rpp, ... of the workgroup's row range.  A thread's channel
// window therefore never changes: its gamma / beta / mean / rstd are loop-invariant registers, and its partial statistics
// belong to fixed groups.  V and D are powers of two, so either the vector holds V / D whole groups (D <= V: 1, 2 or 4
// channels per group sit inside one lane's vector) or D / V adjacent lanes share a group (8 .. 256 channels per group);
// both cases go through the same LDS combine below, which never assumes that a group stays inside one wave.
//
// Variance never comes from E[x^2] - E[x]^2.  A thread takes the exact mean and squared deviations of the E = min(V, D)
// elements of a group it holds in one vector and merges that (count, mean, M2) triple into its running triple with
// Chan's update; the triples of the threads (and, in the split regime, of the workgroups) that share a group are merged
// by the same formula in a FIXED tree order.  No atomics anywhere: two runs give identical bits.
//
// Two regimes, chosen by gn_geometry() (the threshold is kGnKeep * kGnThreads, see there):
//   sample kernel  few rows per sample (ROI heads: 1024 x 49 x 256, 256 x 196 x 256).  A workgroup owns a column tile of
//                  ONE sample over all its rows, keeps its <= kGnKeep vectors per thread in registers, reduces, and
//                  writes y from the registers: x is read from HBM once, one launch.
//   split          few samples with huge planes (backbone: 2 x (400 x 672) x 64).  The rows of a sample are cut into S
//                  chunks over many workgroups: a partial pass writes one triple per (n, g, chunk) to the workspace, a
//                  small finalize merges them in chunk order into mean / rstd, an elementwise pass writes y.  x is read
//                  twice.
// The backward is always the split form (S = 1 for small samples): one reduction pass makes per-(n, chunk, channel)
// sums of dy and dy * xhat, a finalize turns them into the two per-(n, g) means the input gradient needs and — in chunk
// order, then sample order — grad_gamma / grad_beta, and one elementwise pass writes grad_x (and grad_residual).
#include "detops_dtype.h"

namespace {

constexpr int kGnThreads = 256;
constexpr int kGnKeep = 16;                 // vectors a thread of the sample kernel keeps in registers
constexpr int kGnMinTileCols = 4;           // narrowest column tile of the sample kernel the routing plans for (64-byte row segments)
constexpr int64_t kGnChunkElems = 32768;    // split regime: elements of one sample per workgroup (all channels x a row range)
constexpr int kGnMaxChunks = 1024;
constexpr int kGnMaxD = 256;                // channels per group at most (D / V lanes of ONE workgroup row share a group)

static inline bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

// S, the chunks a sample's rows are cut into in the split regime and in the backward: a function of the shape only, so the
// workspace query needs no pointer alignment
static inline int gn_chunks(int64_t HW, int C) {
  const int64_t s = ceil_div64(HW * C, kGnChunkElems);
  return static_cast<int>(s < 1 ? 1 : (s > kGnMaxChunks ? kGnMaxChunks : s));
}

struct GnGeom {
  int V, D, lpg, cols, cols_tile, ctiles, rpp, S;
  int64_t R;          // rows per chunk
  bool sample;        // forward regime: the sample kernel serves it
};

// THE routing function.  lpg = lanes that share a group in a row.  The sample kernel needs every row of a sample in the
// registers of one workgroup: rpp * kGnKeep >= HW with rpp = 256 / cols_tile and cols_tile >= max(lpg, kGnMinTileCols), i.e.
//   HW * max(lpg, kGnMinTileCols) <= kGnThreads * kGnKeep   (= 4096: up to 1024 rows for groups of <= 16 channels)
// Everything above that threshold takes the split regime.
static inline GnGeom gn_geometry(int64_t HW, int C, int G, int V, bool backward) {
  GnGeom g;
  g.V = V;
  g.D = C / G;
  g.lpg = g.D > V ? g.D / V : 1;
  g.cols = C / V;
  const int floor_cols = g.lpg > kGnMinTileCols ? g.lpg : kGnMinTileCols;
  g.sample = !backward && HW * floor_cols <= static_cast<int64_t>(kGnThreads) * kGnKeep;
  if (g.sample) {
    const int64_t cap = static_cast<int64_t>(kGnThreads) * kGnKeep / HW;      // >= floor_cols
    int t = 1;
    while (t * 2 <= cap && t * 2 <= kGnThreads) t *= 2;                       // a power of two >= lpg: whole groups per tile
    g.cols_tile = t >= g.cols ? g.cols : t;
    g.S = 1;
  } else {
    g.cols_tile = g.cols < kGnThreads ? g.cols : kGnThreads;
    g.S = gn_chunks(HW, C);
  }
  g.R = ceil_div64(HW, g.S);
  g.S = static_cast<int>(ceil_div64(HW, g.R));
  g.ctiles = (g.cols + g.cols_tile - 1) / g.cols_tile;
  g.rpp = kGnThreads / g.cols_tile;
  return g;
}

// ---- (count, mean, M2) arithmetic
struct Tri { float n, m, s; };

// a <- a (+) b, Chan et al.; an empty b leaves a alone, an empty a takes b
__device__ __forceinline__ void tri_merge(Tri& a, const Tri& b) {
  if (b.n > 0.f) {
    const float n = a.n + b.n;
    const float d = b.m - a.m;
    const float w = b.n / n;
    a.m = a.m + d * w;
    a.s = a.s + b.s + d * d * (a.n * w);
    a.n = n;
  }
}

// running statistics of the E-element runs a thread meets: k runs so far
template <int E>
__device__ __forceinline__ void run_merge(const float* v, int k, float& mean, float& m2) {
  float lm = v[0];
#pragma unroll
  for (int e = 1; e < E; ++e) lm += v[e];
  lm *= (1.f / E);
  float ls = 0.f;
#pragma unroll
  for (int e = 0; e < E; ++e) { const float d = v[e] - lm; ls += d * d; }
  const float inv = 1.f / static_cast<float>(k + 1);
  const float d = lm - mean;
  mean = mean + d * inv;
  m2 = m2 + ls + d * d * (static_cast<float>(E) * static_cast<float>(k) * inv);
}

// Merge of the workgroup's per-thread triples per group, through LDS, in a fixed binary-tree order.  Thread (tx, ty) holds
// GPV = V / E triples (its vector's groups).  Group gl of the tile has Q = rpp * lpg contributors, contributor q = ty * lpg
// + lane-in-group.  On return sm[.][gl * Q] is the tile's triple of group gl.  `active` false: the thread contributes
// empty triples (columns past the last tile's end).
template <int GPV>
__device__ __forceinline__ void tile_merge(float (*sm)[kGnThreads * GPV], const float* cnt, const float* mean, const float* m2,
                                           bool active, int tx, int ty, int cols_tile, int rpp, int lpg) {
  const int Q = rpp * lpg;
  if (ty < rpp) {
#pragma unroll
    for (int j = 0; j < GPV; ++j) {
      const int slot = tx * GPV + j;
      const int at = (slot / lpg) * Q + ty * lpg + slot % lpg;
      sm[0][at] = active ? cnt[j] : 0.f;
      sm[1][at] = active ? mean[j] : 0.f;
      sm[2][at] = active ? m2[j] : 0.f;
    }
  }
  __syncthreads();
  const int groups = cols_tile * GPV / lpg;
  int h = 1;
  while (h < Q) h <<= 1;
  int live = Q;
  for (h >>= 1; h >= 1; h >>= 1) {
    for (int i = threadIdx.x; i < groups * h; i += kGnThreads) {
      const int gl = i / h, q = i % h;
      if (q + h < live) {
        const int a = gl * Q + q, b = a + h;
        Tri ta = {sm[0][a], sm[1][a], sm[2][a]};
        const Tri tb = {sm[0][b], sm[1][b], sm[2][b]};
        tri_merge(ta, tb);
        sm[0][a] = ta.n; sm[1][a] = ta.m; sm[2][a] = ta.s;
      }
    }
    __syncthreads();
    if (live > h) live = h;
  }
}

__device__ __forceinline__ float gn_rstd(float m2, float count, float eps) { return 1.f / sqrtf(m2 / count + eps); }

// y of one vector: fma(x - mean, rstd * gamma, beta) [+ residual] [relu]
template <typename T, int V>
__device__ __forceinline__ Vec<T, V> gn_apply(const Vec<T, V>& a, const Vec<T, V>& r, const float* mu, const float* sc, const float* be,
                                              bool res, bool relu) {
  Vec<T, V> o;
#pragma unroll
  for (int j = 0; j < V; ++j) {
    float t = fmaf(Io<T>::ld(a.v[j]) - mu[j], sc[j], be[j]);
    if (res) t = t + Io<T>::ld(r.v[j]);
    if (relu) t = relu_fwd(t);
    o.v[j] = Io<T>::st(t);
  }
  return o;
}

// the thread's loop-invariant per-channel registers: gamma (null: 1) and beta (null: 0)
template <int V>
__device__ __forceinline__ void gn_affine(const float* gamma, const float* beta, int c0, float* ga, float* be) {
#pragma unroll
  for (int j = 0; j < V; ++j) {
    ga[j] = gamma ? gamma[c0 + j] : 1.f;
    be[j] = beta ? beta[c0 + j] : 0.f;
  }
}

// ---- forward, sample kernel: workgroup = (sample n = blockIdx.x, column tile = blockIdx.y), all HW rows, x kept in registers
template <typename T, int V, int E>
__global__ void __launch_bounds__(kGnThreads)
gn_fwd_sample_kernel(const T* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                     const T* __restrict__ res, T* __restrict__ y, float* __restrict__ mean_out, float* __restrict__ rstd_out,
                     int HW, int C, int G, float eps, int relu, int cols_tile, int rpp, int lpg) {
  constexpr int GPV = V / E;
  using VT = Vec<T, V>;
  __shared__ float sm[3][kGnThreads * GPV];
  const int tx = threadIdx.x % cols_tile, ty = threadIdx.x / cols_tile;
  const int col = blockIdx.y * cols_tile + tx;
  const int cols = C / V, D = C / G;
  const bool active = col < cols && ty < rpp;
  const size_t n = blockIdx.x;
  const size_t base = n * static_cast<size_t>(HW) * cols + col;          // in vectors
  const VT* xv = reinterpret_cast<const VT*>(x);
  VT keep[kGnKeep];
  float cnt[GPV], mean[GPV], m2[GPV];
#pragma unroll
  for (int j = 0; j < GPV; ++j) { cnt[j] = 0.f; mean[j] = 0.f; m2[j] = 0.f; }
  if (active) {
#pragma unroll
    for (int k = 0; k < kGnKeep; ++k) {
      const int r = ty + k * rpp;
      if (r < HW) {
        keep[k] = xv[base + static_cast<size_t>(r) * cols];
        float f[V];
#pragma unroll
        for (int j = 0; j < V; ++j) f[j] = Io<T>::ld(keep[k].v[j]);
#pragma unroll
        for (int j = 0; j < GPV; ++j) { run_merge<E>(f + j * E, k, mean[j], m2[j]); cnt[j] = static_cast<float>((k + 1) * E); }
      }
    }
  }
  tile_merge<GPV>(sm, cnt, mean, m2, active, tx, ty, cols_tile, rpp, lpg);
  if (!active) return;
  const int Q = rpp * lpg;
  const int c0 = col * V;
  float mu[V], sc[V], be[V];
  gn_affine<V>(gamma, beta, c0, sc, be);
#pragma unroll
  for (int j = 0; j < GPV; ++j) {
    const int slot = tx * GPV + j;
    const int at = (slot / lpg) * Q;
    const float m = sm[1][at];
    const float rs = gn_rstd(sm[2][at], sm[0][at], eps);
    if (ty == 0 && slot % lpg == 0) {
      const size_t o = n * G + (c0 + j * E) / D;
      mean_out[o] = m;
      rstd_out[o] = rs;
    }
#pragma unroll
    for (int e = 0; e < E; ++e) { mu[j * E + e] = m; sc[j * E + e] = rs * sc[j * E + e]; }
  }
  const VT* rv = reinterpret_cast<const VT*>(res);
  VT* yv = reinterpret_cast<VT*>(y);
#pragma unroll
  for (int k = 0; k < kGnKeep; ++k) {
    const int r = ty + k * rpp;
    if (r < HW) {
      const size_t at = base + static_cast<size_t>(r) * cols;
      VT rr;
      if (res) rr = rv[at];
      yv[at] = gn_apply<T, V>(keep[k], rr, mu, sc, be, res != nullptr, relu != 0);
    }
  }
}

// ---- forward, split regime 1/3: workgroup = (n * S + s = blockIdx.x, column tile = blockIdx.y) -> one triple per group of
// the tile into part[((n * G + g) * S + s) * 3]
template <typename T, int V, int E>
__global__ void __launch_bounds__(kGnThreads)
gn_fwd_partial_kernel(const T* __restrict__ x, float* __restrict__ part, int HW, int C, int G, int S, int R, int cols_tile,
                      int rpp, int lpg) {
  constexpr int GPV = V / E;
  using VT = Vec<T, V>;
  __shared__ float sm[3][kGnThreads * GPV];
  const int tx = threadIdx.x % cols_tile, ty = threadIdx.x / cols_tile;
  const int col = blockIdx.y * cols_tile + tx;
  const int cols = C / V, D = C / G;
  const bool active = col < cols && ty < rpp;
  const size_t n = blockIdx.x / S;
  const int s = blockIdx.x % S;
  const int r0 = s * R, r1 = r0 + R < HW ? r0 + R : HW;
  const VT* xv = reinterpret_cast<const VT*>(x) + n * static_cast<size_t>(HW) * cols + col;
  float cnt[GPV], mean[GPV], m2[GPV];
#pragma unroll
  for (int j = 0; j < GPV; ++j) { cnt[j] = 0.f; mean[j] = 0.f; m2[j] = 0.f; }
  if (active) {
    int k = 0;
    for (int r = r0 + ty; r < r1; r += rpp, ++k) {
      const VT a = xv[static_cast<size_t>(r) * cols];
      float f[V];
#pragma unroll
      for (int j = 0; j < V; ++j) f[j] = Io<T>::ld(a.v[j]);
#pragma unroll
      for (int j = 0; j < GPV; ++j) run_merge<E>(f + j * E, k, mean[j], m2[j]);
    }
#pragma unroll
    for (int j = 0; j < GPV; ++j) cnt[j] = static_cast<float>(k * E);
  }
  tile_merge<GPV>(sm, cnt, mean, m2, active, tx, ty, cols_tile, rpp, lpg);
  const int Q = rpp * lpg;
  if (active && ty == 0) {
#pragma unroll
    for (int j = 0; j < GPV; ++j) {
      const int slot = tx * GPV + j;
      if (slot % lpg == 0) {
        const int at = (slot / lpg) * Q;
        float* o = part + ((n * G + (col * V + j * E) / D) * S + s) * 3;
        o[0] = sm[0][at]; o[1] = sm[1][at]; o[2] = sm[2][at];
      }
    }
  }
}

// ---- forward, split regime 2/3: a wave per (n, g): lane l merges chunks l, l + 64, ... in order, then the lanes in a fixed tree
__global__ void __launch_bounds__(kGnThreads)
gn_fwd_finalize_kernel(const float* __restrict__ part, float* __restrict__ mean_out, float* __restrict__ rstd_out, int64_t NG,
                       int S, float eps) {
  const int lane = threadIdx.x % kWave;
  const int64_t ng = static_cast<int64_t>(blockIdx.x) * (kGnThreads / kWave) + threadIdx.x / kWave;
  if (ng >= NG) return;
  Tri t = {0.f, 0.f, 0.f};
  for (int s = lane; s < S; s += kWave) {
    const float* p = part + (ng * S + s) * 3;
    const Tri b = {p[0], p[1], p[2]};
    tri_merge(t, b);
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const Tri b = {__shfl_down(t.n, off), __shfl_down(t.m, off), __shfl_down(t.s, off)};
    if (lane < off) tri_merge(t, b);
  }
  if (lane == 0) {
    mean_out[ng] = t.m;
    rstd_out[ng] = gn_rstd(t.s, t.n, eps);
  }
}

// the thread's per-channel mean / rstd of sample n
template <int V, int E>
__device__ __forceinline__ void gn_stats(const float* mean, const float* rstd, size_t n, int G, int D, int c0, float* mu, float* rs) {
#pragma unroll
  for (int j = 0; j < V / E; ++j) {
    const size_t o = n * G + (c0 + j * E) / D;
    const float m = mean[o], r = rstd[o];
#pragma unroll
    for (int e = 0; e < E; ++e) { mu[j * E + e] = m; rs[j * E + e] = r; }
  }
}

// ---- forward, split regime 3/3: elementwise, same workgroup -> data mapping as the partial pass
template <typename T, int V, int E>
__global__ void __launch_bounds__(kGnThreads)
gn_fwd_apply_kernel(const T* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                    const T* __restrict__ res, T* __restrict__ y, const float* __restrict__ mean, const float* __restrict__ rstd,
                    int HW, int C, int G, int S, int R, int relu, int cols_tile, int rpp) {
  using VT = Vec<T, V>;
  const int tx = threadIdx.x % cols_tile, ty = threadIdx.x / cols_tile;
  const int col = blockIdx.y * cols_tile + tx;
  const int cols = C / V;
  if (col >= cols || ty >= rpp) return;
  const size_t n = blockIdx.x / S;
  const int s = blockIdx.x % S;
  const int r0 = s * R, r1 = r0 + R < HW ? r0 + R : HW;
  float mu[V], sc[V], be[V], rs[V];
  gn_affine<V>(gamma, beta, col * V, sc, be);
  gn_stats<V, E>(mean, rstd, n, G, C / G, col * V, mu, rs);
#pragma unroll
  for (int j = 0; j < V; ++j) sc[j] = rs[j] * sc[j];
  const size_t base = n * static_cast<size_t>(HW) * cols + col;
  const VT* xv = reinterpret_cast<const VT*>(x);
  const VT* rv = reinterpret_cast<const VT*>(res);
  VT* yv = reinterpret_cast<VT*>(y);
  for (int r = r0 + ty; r < r1; r += rpp) {
    const size_t at = base + static_cast<size_t>(r) * cols;
    const VT a = xv[at];
    VT rr;
    if (res) rr = rv[at];
    yv[at] = gn_apply<T, V>(a, rr, mu, sc, be, res != nullptr, relu != 0);
  }
}

// ---- backward 1/3: per (n, chunk, channel) sums of g = masked grad_y and of g * xhat into
// sums[((n * S + s) * 2 + {0: g, 1: g * xhat}) * C + c]; a thread adds its rows in order, the rows' threads add in ty order
template <typename T, int V, int E>
__global__ void __launch_bounds__(kGnThreads)
gn_bwd_reduce_kernel(const T* __restrict__ gy, const T* __restrict__ x, const T* __restrict__ y, const float* __restrict__ mean,
                     const float* __restrict__ rstd, float* __restrict__ sums, int HW, int C, int G, int S, int R, int relu,
                     int cols_tile, int rpp) {
  using VT = Vec<T, V>;
  __shared__ float sm[2 * kGnThreads * V];
  const int tx = threadIdx.x % cols_tile, ty = threadIdx.x / cols_tile;
  const int col = blockIdx.y * cols_tile + tx;
  const int cols = C / V;
  const bool active = col < cols && ty < rpp;
  const size_t n = blockIdx.x / S;
  const int s = blockIdx.x % S;
  const int r0 = s * R, r1 = r0 + R < HW ? r0 + R : HW;
  float s1[V], s2[V];
#pragma unroll
  for (int j = 0; j < V; ++j) { s1[j] = 0.f; s2[j] = 0.f; }
  if (active) {
    float mu[V], rs[V];
    gn_stats<V, E>(mean, rstd, n, G, C / G, col * V, mu, rs);
    const size_t base = n * static_cast<size_t>(HW) * cols + col;
    const VT* gv = reinterpret_cast<const VT*>(gy);
    const VT* xv = reinterpret_cast<const VT*>(x);
    const VT* yv = reinterpret_cast<const VT*>(y);
    for (int r = r0 + ty; r < r1; r += rpp) {
      const size_t at = base + static_cast<size_t>(r) * cols;
      const VT g = gv[at];
      const VT a = xv[at];
      VT m;
      if (relu) m = yv[at];
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float t = Io<T>::ld(g.v[j]);
        if (relu) t = relu_bwd(t, Io<T>::ld(m.v[j]));
        s1[j] += t;
        s2[j] += t * ((Io<T>::ld(a.v[j]) - mu[j]) * rs[j]);
      }
    }
  }
  const int width = cols_tile * V;            // channels of the tile
  if (ty < rpp) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
      sm[(ty * 2 + 0) * width + tx * V + j] = s1[j];
      sm[(ty * 2 + 1) * width + tx * V + j] = s2[j];
    }
  }
  __syncthreads();
  const int c_lo = blockIdx.y * width;
  for (int i = threadIdx.x; i < 2 * width; i += kGnThreads) {
    const int which = i / width, cl = i % width;
    if (c_lo + cl < C) {
      float t = sm[which * width + cl];
      for (int q = 1; q < rpp; ++q) t += sm[(q * 2 + which) * width + cl];
      sums[((n * S + s) * 2 + which) * C + c_lo + cl] = t;
    }
  }
}

// ---- backward 2/3 a: a wave per (n, g) -> ab[(n * G + g) * 2] = { sum(g * gamma) / m, sum(g * gamma * xhat) / m }, m = HW * D
__global__ void __launch_bounds__(kGnThreads)
gn_bwd_group_kernel(const float* __restrict__ sums, const float* __restrict__ gamma, float* __restrict__ ab, int64_t NG, int G,
                    int C, int S, float inv_m) {
  const int lane = threadIdx.x % kWave;
  const int64_t ng = static_cast<int64_t>(blockIdx.x) * (kGnThreads / kWave) + threadIdx.x / kWave;
  if (ng >= NG) return;
  const int64_t n = ng / G;
  const int g = static_cast<int>(ng % G), D = C / G;
  float a = 0.f, b = 0.f;
  for (int t = lane; t < S * D; t += kWave) {
    const int s = t / D, c = g * D + t % D;
    const float w = gamma ? gamma[c] : 1.f;
    const float* p = sums + (n * S + s) * 2 * C + c;
    a += w * p[0];
    b += w * p[C];
  }
  a = wave_sum(a);
  b = wave_sum(b);
  if (lane == 0) { ab[ng * 2] = a * inv_m; ab[ng * 2 + 1] = b * inv_m; }
}

// ---- backward 3/3: grad_x = rstd * (gamma * g - A - xhat * B), grad_residual = g
template <typename T, int V, int E>
__global__ void __launch_bounds__(kGnThreads)
gn_bwd_apply_kernel(const T* __restrict__ gy, const T* __restrict__ x, const T* __restrict__ y, const float* __restrict__ gamma,
                    const float* __restrict__ mean, const float* __restrict__ rstd, const float* __restrict__ ab,
                    T* __restrict__ gx, T* __restrict__ gres, int HW, int C, int G, int S, int R, int relu, int cols_tile, int rpp) {
  using VT = Vec<T, V>;
  const int tx = threadIdx.x % cols_tile, ty = threadIdx.x / cols_tile;
  const int col = blockIdx.y * cols_tile + tx;
  const int cols = C / V, D = C / G;
  if (col >= cols || ty >= rpp) return;
  const size_t n = blockIdx.x / S;
  const int s = blockIdx.x % S;
  const int r0 = s * R, r1 = r0 + R < HW ? r0 + R : HW;
  float mu[V], rs[V], c1[V], k0[V], k1[V];
  gn_stats<V, E>(mean, rstd, n, G, D, col * V, mu, rs);
#pragma unroll
  for (int j = 0; j < V; ++j) {
    const int c = col * V + j;
    const float* p = ab + (n * G + c / D) * 2;
    c1[j] = (gamma ? gamma[c] : 1.f) * rs[j];
    k0[j] = rs[j] * p[0];
    k1[j] = rs[j] * rs[j] * p[1];
  }
  const size_t base = n * static_cast<size_t>(HW) * cols + col;
  const VT* gv = reinterpret_cast<const VT*>(gy);
  const VT* xv = reinterpret_cast<const VT*>(x);
  const VT* yv = reinterpret_cast<const VT*>(y);
  VT* xo = reinterpret_cast<VT*>(gx);
  VT* ro = reinterpret_cast<VT*>(gres);
  for (int r = r0 + ty; r < r1; r += rpp) {
    const size_t at = base + static_cast<size_t>(r) * cols;
    const VT g = gv[at];
    const VT a = xv[at];
    VT m;
    if (relu) m = yv[at];
    VT ox, orr;
#pragma unroll
    for (int j = 0; j < V; ++j) {
      float t = Io<T>::ld(g.v[j]);
      if (relu) t = relu_bwd(t, Io<T>::ld(m.v[j]));
      const float d = c1[j] * t - k0[j] - (Io<T>::ld(a.v[j]) - mu[j]) * k1[j];
      ox.v[j] = Io<T>::st(d);
      orr.v[j] = Io<T>::st(t);
    }
    xo[at] = ox;
    if (gres) ro[at] = orr;
  }
}

// E = min(V, D) as a template argument (E <= V, both powers of two)
template <int V, typename F> static inline int dispatch_run(int E, F&& f) {
  if constexpr (V >= 8) if (E == 8) return f(std::integral_constant<int, 8>{});
  if constexpr (V >= 4) if (E == 4) return f(std::integral_constant<int, 4>{});
  if constexpr (V >= 2) if (E == 2) return f(std::integral_constant<int, 2>{});
  return f(std::integral_constant<int, 1>{});
}

static inline size_t fwd_ws_floats(int N, int64_t HW, int C, int G) {
  return static_cast<size_t>(N) * G * gn_chunks(HW, C) * 3;
}
static inline size_t bwd_ws_floats(int N, int64_t HW, int C, int G) {
  return static_cast<size_t>(N) * gn_chunks(HW, C) * 2 * C + static_cast<size_t>(N) * G * 2;
}

template <typename T>
int gn_forward(const void* x, const float* gamma, const float* beta, const void* res, void* y, float* mean, float* rstd, int N,
               int HW, int C, int G, float eps, int relu, float* ws, hipStream_t st) {
  const T* xp = static_cast<const T*>(x);
  const T* rp = static_cast<const T*>(res);
  T* yp = static_cast<T*>(y);
  return dispatch_vec<T>(pick_vec<T>(C, {x, res, y}), [&](auto vc) {
    constexpr int V = decltype(vc)::value;
    const GnGeom g = gn_geometry(HW, C, G, V, false);
    return dispatch_run<V>(g.D < V ? g.D : V, [&](auto ec) {
      constexpr int E = decltype(ec)::value;
      const dim3 grid(static_cast<unsigned>(N) * g.S, g.ctiles), block(kGnThreads);
      if (g.sample) {
        hipLaunchKernelGGL((gn_fwd_sample_kernel<T, V, E>), grid, block, 0, st, xp, gamma, beta, rp, yp, mean, rstd, HW, C, G, eps,
                           relu, g.cols_tile, g.rpp, g.lpg);
        return launch_status();
      }
      hipLaunchKernelGGL((gn_fwd_partial_kernel<T, V, E>), grid, block, 0, st, xp, ws, HW, C, G, g.S, static_cast<int>(g.R),
                         g.cols_tile, g.rpp, g.lpg);
      int e = launch_status();
      if (e) return e;
      const int64_t NG = static_cast<int64_t>(N) * G;
      hipLaunchKernelGGL(gn_fwd_finalize_kernel, dim3(static_cast<unsigned>(ceil_div64(NG, kGnThreads / kWave))), block, 0, st, ws, mean,
                         rstd, NG, g.S, eps);
      e = launch_status();
      if (e) return e;
      hipLaunchKernelGGL((gn_fwd_apply_kernel<T, V, E>), grid, block, 0, st, xp, gamma, beta, rp, yp, mean, rstd, HW, C, G, g.S,
                         static_cast<int>(g.R), relu, g.cols_tile, g.rpp);
      return launch_status();
    });
  });
}

template <typename T>
int gn_backward(const void* gy, const void* x, const void* y, const float* gamma, const float* mean, const float* rstd, void* gx,
                void* gres, float* ggamma, float* gbeta, int N, int HW, int C, int G, int relu, float* ws, hipStream_t st) {
  const T* gp = static_cast<const T*>(gy);
  const T* xp = static_cast<const T*>(x);
  const T* yp = static_cast<const T*>(y);
  T* xo = static_cast<T*>(gx);
  T* ro = static_cast<T*>(gres);
  return dispatch_vec<T>(pick_vec<T>(C, {gy, x, relu ? y : nullptr, gx, gres}), [&](auto vc) {
    constexpr int V = decltype(vc)::value;
    const GnGeom g = gn_geometry(HW, C, G, V, true);
    return dispatch_run<V>(g.D < V ? g.D : V, [&](auto ec) {
      constexpr int E = decltype(ec)::value;
      const dim3 grid(static_cast<unsigned>(N) * g.S, g.ctiles), block(kGnThreads);
      float* sums = ws;
      float* ab = ws + static_cast<size_t>(N) * g.S * 2 * C;
      const int R = static_cast<int>(g.R);
      hipLaunchKernelGGL((gn_bwd_reduce_kernel<T, V, E>), grid, block, 0, st, gp, xp, yp, mean, rstd, sums, HW, C, G, g.S, R, relu,
                         g.cols_tile, g.rpp);
      int e = launch_status();
      if (e) return e;
      const int64_t NG = static_cast<int64_t>(N) * G;
      hipLaunchKernelGGL(gn_bwd_group_kernel, dim3(static_cast<unsigned>(ceil_div64(NG, kGnThreads / kWave))), block, 0, st, sums, gamma,
                         ab, NG, G, C, g.S, 1.f / (static_cast<float>(HW) * static_cast<float>(g.D)));
      e = launch_status();
      if (e) return e;
      if (ggamma || gbeta) {
        // backward 2/3 b: grad_beta[c] = sum over (n, s) of sums[.][0][c], grad_gamma[c] likewise of sums[.][1][c]
        e = column_partials_finish(sums, gbeta, ggamma, C, static_cast<int64_t>(N) * g.S, 2 * C, C, st);
        if (e) return e;
      }
      hipLaunchKernelGGL((gn_bwd_apply_kernel<T, V, E>), grid, block, 0, st, gp, xp, yp, gamma, mean, rstd, ab, xo, ro, HW, C, G, g.S, R,
                         relu, g.cols_tile, g.rpp);
      return launch_status();
    });
  });
}

// shape checks shared by the two entry points: 0 = go on, 1 = nothing to do, negative = the error to return
static inline int gn_shape(int N, int64_t HW, int C, int G) {
  if (N < 0 || HW < 0 || C <= 0 || G <= 0) return DETOPS_EINVAL;
  if (!detops_group_norm_supported(C, G)) return DETOPS_EUNSUPPORTED;
  if (N == 0 || HW == 0) return 1;
  // 32-bit row indices and grid.x = N * S
  if (HW > 0x7fffffff / 2 || static_cast<int64_t>(N) * gn_chunks(HW, C) > 0x7fffffff) return DETOPS_EUNSUPPORTED;
  return 0;
}

}  // namespace

// C % G == 0, a power-of-two group width of at most 256 channels (every width of the detector: 64 .. 2048 channels in 32
// groups; 1 channel per group and G = 1 included)
DETOPS_API int detops_group_norm_supported(int C, int G) {
  if (C <= 0 || G <= 0 || C % G != 0) return 0;
  const int D = C / G;
  return (pow2(D) && D <= kGnMaxD) ? 1 : 0;
}

DETOPS_API size_t detops_group_norm_workspace_bytes(int N, int64_t HW, int C, int G) {
  if (N <= 0 || HW <= 0 || !detops_group_norm_supported(C, G)) return 0;
  const size_t f = fwd_ws_floats(N, HW, C, G), b = bwd_ws_floats(N, HW, C, G);
  return sizeof(float) * (f > b ? f : b);
}

DETOPS_API int detops_group_norm_forward_nhwc(const void* x, const float* gamma, const float* beta, const void* residual, void* y,
                                              float* mean, float* rstd, int dtype, int N, int64_t HW, int C, int G, float eps,
                                              int relu, void* workspace, size_t workspace_bytes, detops_stream_t stream) {
  const int sh = gn_shape(N, HW, C, G);
  if (sh) return sh < 0 ? sh : 0;
  if (!x || !y || !mean || !rstd) return DETOPS_EINVAL;
  if (dtype != DETOPS_F32 && dtype != DETOPS_F16 && dtype != DETOPS_BF16) return DETOPS_EUNSUPPORTED;
  if (!workspace || workspace_bytes < detops_group_norm_workspace_bytes(N, HW, C, G)) return DETOPS_EWORKSPACE;   // one size serves both directions
  hipStream_t st = as_stream(stream);
  return dispatch_dtype(dtype, [&](auto tag) {
    return gn_forward<typename decltype(tag)::type>(x, gamma, beta, residual, y, mean, rstd, N, static_cast<int>(HW), C, G, eps, relu,
                                                    static_cast<float*>(workspace), st);
  });
}

DETOPS_API int detops_group_norm_backward_nhwc(const void* grad_y, const void* x, const void* y, const float* gamma, const float* mean,
                                               const float* rstd, void* grad_x, void* grad_residual, float* grad_gamma,
                                               float* grad_beta, int dtype, int N, int64_t HW, int C, int G, int relu, void* workspace,
                                               size_t workspace_bytes, detops_stream_t stream) {
  const int sh = gn_shape(N, HW, C, G);
  if (sh) return sh < 0 ? sh : 0;      // no rows: nothing is written (the caller zeroes the parameter gradients it wants)
  hipStream_t st = as_stream(stream);
  if (!grad_y || !x || !mean || !rstd || !grad_x || (relu && !y)) return DETOPS_EINVAL;
  if (dtype != DETOPS_F32 && dtype != DETOPS_F16 && dtype != DETOPS_BF16) return DETOPS_EUNSUPPORTED;
  if (!workspace || workspace_bytes < detops_group_norm_workspace_bytes(N, HW, C, G)) return DETOPS_EWORKSPACE;   // one size serves both directions
  return dispatch_dtype(dtype, [&](auto tag) {
    return gn_backward<typename decltype(tag)::type>(grad_y, x, y, gamma, mean, rstd, grad_x, grad_residual, grad_gamma, grad_beta, N,
                                                     static_cast<int>(HW), C, G, relu, static_cast<float*>(workspace), st);
  });
}
