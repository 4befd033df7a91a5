// detops_dtype.h — what the elementwise and loss kernels share: storage-type I/O, 16-byte vectors, the host-side step from
// a run-time dtype code / vector width / flag to a template argument, the wave and workgroup sums in the library's one
// fixed order, the integer prefix scans (wave, workgroup, carried over tiles) with their one scratch and barrier contract,
// the lookup in an ascending offsets table, the finish kernel for column partials, and the fused ReLU rule.  Only helpers
// with at least two users live here.
#pragma once
#include <initializer_list>
#include <type_traits>
#include <utility>

#include "detops_common.h"

// ---- storage type <-> the fp32 value the arithmetic runs on
template <typename T> struct Io;
template <> struct Io<float> {
  static __device__ __forceinline__ float ld(float v) { return v; }
  static __device__ __forceinline__ float st(float v) { return v; }
};
template <> struct Io<__half> {
  static __device__ __forceinline__ float ld(__half v) { return __half2float(v); }
  static __device__ __forceinline__ __half st(float v) { return __float2half(v); }
};
template <> struct Io<__hip_bfloat16> {
  static __device__ __forceinline__ float ld(__hip_bfloat16 v) { return __bfloat162float(v); }
  static __device__ __forceinline__ __hip_bfloat16 st(float v) { return __float2bfloat16(v); }
};

// V elements moved as one access (at most 16 bytes)
template <typename T, int V> struct alignas(sizeof(T) * V) Vec { T v[V]; };

template <typename T> constexpr int max_vec() { return 16 / static_cast<int>(sizeof(T)); }

// widest power of two V <= max_vec<T>() such that V | extent (a vector never straddles a row / plane / pixel) and every
// non-null pointer is aligned to a whole vector
template <typename T> static inline int pick_vec(int64_t extent, std::initializer_list<const void*> ptrs) {
  uintptr_t bits = 0;
  for (const void* p : ptrs) bits |= reinterpret_cast<uintptr_t>(p);
  for (int v = max_vec<T>(); v > 1; v >>= 1)
    if (extent % v == 0 && bits % (v * sizeof(T)) == 0) return v;
  return 1;
}

// ---- run-time value -> compile-time argument of a C++17 generic lambda (host side).  The lambda returns the entry
// point's status code.
//   dispatch_dtype(dtype, [&](auto tag) { using T = typename decltype(tag)::type; ... });
//   dispatch_vec<T>(v, [&](auto vc) { constexpr int V = decltype(vc)::value; ... });      only V <= max_vec<T>() exist
//   dispatch_bools(a, b, [&](auto ca, auto cb) { ... decltype(ca)::value ... });
template <typename T> struct DType { using type = T; };

template <typename F> static inline int dispatch_dtype(int dtype, F&& f) {
  switch (dtype) {
    case DETOPS_F32: return f(DType<float>{});
    case DETOPS_F16: return f(DType<__half>{});
    case DETOPS_BF16: return f(DType<__hip_bfloat16>{});
    default: return DETOPS_EUNSUPPORTED;
  }
}

template <typename T, typename F> static inline int dispatch_vec(int v, F&& f) {
  if constexpr (max_vec<T>() >= 8)
    if (v == 8) return f(std::integral_constant<int, 8>{});
  if (v == 4) return f(std::integral_constant<int, 4>{});
  if (v == 2) return f(std::integral_constant<int, 2>{});
  return f(std::integral_constant<int, 1>{});
}

template <typename F> static inline int dispatch_bool(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }

template <typename F> static inline int dispatch_bools(bool a, bool b, F&& f) {
  return dispatch_bool(a, [&](auto ca) { return dispatch_bool(b, [&](auto cb) { return f(ca, cb); }); });
}

// ---- reductions of ONE value over the wave: the result is valid in lane 0; the _all forms hand it to every lane
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v = fmaxf(v, __shfl_down(v, off));
  return v;
}
__device__ __forceinline__ float wave_sum_all(float v) { return __shfl(wave_sum(v), 0); }
__device__ __forceinline__ float wave_max_all(float v) { return __shfl(wave_max(v), 0); }
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off);
  return v;
}

// ---- THE fixed-order sum of N values over a workgroup of kThreads threads (T = float | int), the library's one order
// for every loss and count: a thread first adds its own strided share (the caller's loop), then wave_sum's shuffle tree
// inside each wave, then the waves' values in wave order starting from zero.  Two runs give identical bits.
// Contract: every thread of the workgroup calls it, in uniform control flow (it holds a barrier).  On return EVERY
// thread holds the N sums in v.  `scratch` is LDS; other threads may still be reading it on return, so it (this
// function included) may be written again only after a later __syncthreads().
template <int kThreads, typename T, int N>
__device__ __forceinline__ void block_sum(T (&v)[N], T (&scratch)[N][kThreads / kWave]) {
  static_assert(kThreads % kWave == 0, "whole waves");
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const T w = wave_sum(v[k]);
    if ((threadIdx.x & (kWave - 1)) == 0) scratch[k][threadIdx.x / kWave] = w;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) {
    T t = 0;
#pragma unroll
    for (int j = 0; j < kThreads / kWave; ++j) t += scratch[k][j];
    v[k] = t;
  }
}
// one value: `scratch` holds kThreads / kWave elements
template <int kThreads, typename T>
__device__ __forceinline__ T block_sum(T v, T (&scratch)[kThreads / kWave]) {
  T a[1] = {v};
  block_sum<kThreads>(a, reinterpret_cast<T (&)[1][kThreads / kWave]>(scratch));
  return a[0];
}

// ---- THE inclusive scan of ONE value over the wave, in lane order: lane l gets op(... op(v_0, v_1) ..., v_l); op is +
// unless given (T = int | int64_t; integers, so the tree's order changes no bit).  The exclusive sum is `incl - v` at the
// call site, the wave's total is `__shfl(incl, kWave - 1)`.  Every lane of the wave calls it.
template <typename T, typename Op>
__device__ __forceinline__ T wave_scan(T v, Op op) {
  const int lane = threadIdx.x & (kWave - 1);
#pragma unroll
  for (int off = 1; off < kWave; off <<= 1) {
    const T o = __shfl_up(v, off);
    if (lane >= off) v = op(v, o);
  }
  return v;
}
template <typename T> __device__ __forceinline__ T wave_scan(T v) {
  return wave_scan(v, [](T a, T b) { return a + b; });
}

// ---- THE scan over a workgroup of kThreads threads, in thread order.  Same contract as block_sum: every thread of the
// workgroup calls it, in uniform control flow (it holds one barrier); `scratch` is LDS of kThreads / kWave elements, other
// threads may still be reading it on return, so it (these functions included) may be written again only after a later
// __syncthreads(), which the caller places (a loop around it: one at the end of the body).
// The cross-wave half: `wave_total` is the wave's sum in its LAST lane (wave_scan's inclusive value there; a ballot's
// popcount in every lane); returns the sum of the waves before the caller's own, `total` = the sum of all.
template <int kThreads, typename T>
__device__ __forceinline__ T block_scan_base(T wave_total, T* scratch, T& total) {
  static_assert(kThreads % kWave == 0, "whole waves");
  const int wave = threadIdx.x / kWave;
  if ((threadIdx.x & (kWave - 1)) == kWave - 1) scratch[wave] = wave_total;
  __syncthreads();
  T base = 0, all = 0;
#pragma unroll
  for (int j = 0; j < kThreads / kWave; ++j) {
    const T t = scratch[j];
    if (j < wave) base += t;
    all += t;
  }
  total = all;
  return base;
}
// the whole of it: the inclusive sum of v over the threads up to the caller's own (exclusive: `- v` at the call site)
template <int kThreads, typename T>
__device__ __forceinline__ T block_scan(T v, T* scratch, T& total) {
  const T incl = wave_scan(v);
  return block_scan_base<kThreads>(incl, scratch, total) + incl;
}

// ---- THE loop that scans an array longer than its tile: elements [0, n) in tiles of kTile, tiles in order with a running
// carry.  kTile = kWave: the calling wave alone (uniform over the wave; no barrier, no scratch).  kTile = the workgroup's
// size: block_scan and its contract, with the barrier that frees `scratch` for the next tile at the end of each round
// (two barriers a round).  load(i) reads element i, store(i, before) gets the sum of the elements in front of i (it may
// overwrite what load read); the sum of all n is returned to every thread.  T is what load returns.
template <int kTile, typename I, typename Load, typename Store, typename T = decltype(std::declval<Load>()(I{}))>
__device__ __forceinline__ T scan_tiles(I n, Load load, Store store, T* scratch = nullptr) {
  static_assert(kTile % kWave == 0 && (kTile & (kTile - 1)) == 0, "whole waves, a power of two");
  T carry = 0;
  for (I base = 0; base < n; base += kTile) {
    const I i = base + static_cast<I>(threadIdx.x & (kTile - 1));
    const T v = i < n ? load(i) : T(0);
    T incl, total;
    if constexpr (kTile == kWave) {
      incl = wave_scan(v);
      total = __shfl(incl, kWave - 1);
    } else {
      incl = block_scan<kTile>(v, scratch, total);
    }
    if (i < n) store(i, carry + incl - v);
    carry += total;
    if constexpr (kTile != kWave) __syncthreads();
  }
  return carry;
}

// ---- THE lookup in an ascending offsets table (global or LDS; int or int64_t): the last m < n with table[m] <= i, 0 when
// there is none.  Entries without elements share their successor's offset, so the LAST of equal entries owns i.  A
// bisection that reads table[1 .. n - 1] only and ends after ceil(log2 n) steps whatever the table holds.
template <typename T, typename I>
__device__ __forceinline__ int last_at_or_below(const T* table, int n, I i) {
  int lo = 0, hi = n;                   // table[lo] <= i < table[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (table[mid] <= i) lo = mid; else hi = mid;
  }
  return lo;
}

// ---- THE fused ReLU rule, torch's, for every kernel that folds a ReLU into its epilogue or its backward
// forward: torch.relu(t) — the comparison is false for NaN, so NaN stays NaN (and -0.0 becomes +0.0)
__host__ __device__ __forceinline__ float relu_fwd(float t) { return t <= 0.f ? 0.f : t; }
// backward: aten.threshold_backward(g, y, 0) = y <= 0 ? 0 : g — a NaN activation PASSES the gradient
__host__ __device__ __forceinline__ float relu_bwd(float g, float y) { return y <= 0.f ? 0.f : g; }
// (the same gate on stored values: the gradient does not leave its storage type)
template <typename T> __device__ __forceinline__ T relu_bwd(T g, T y) { return Io<T>::ld(y) <= 0.f ? Io<T>::st(0.f) : g; }

// ---- THE finish kernel behind every pass that leaves per-workgroup column partials (bias gradients, column sums,
// GroupNorm's gamma / beta gradients): out_y[c] = sum over p < rows of partials[p * row_stride + y * offset1 + c], c < C,
// for y = blockIdx.y in {0, 1} (the second sum reads the same rows `offset1` floats further on: an interleaved
// [rows][2][C] layout; a null out_y skips its sum).  A workgroup per kColCh channels, kColRows row lanes per channel:
// lane r adds rows r, r + kColRows, ... in order, then the lane sums are added in lane order through LDS — a fixed order,
// and 32x shorter dependent chains than one thread per channel (which took 156 us for 1024 partial rows).
constexpr int kColCh = 32, kColRows = 32;
static __global__ void __launch_bounds__(kColCh * kColRows)
column_partials_finish_kernel(const float* __restrict__ partials, float* __restrict__ out0, float* __restrict__ out1, int C,
                              int64_t rows, int64_t row_stride, int64_t offset1) {
  __shared__ float red[kColRows][kColCh + 1];
  float* out = blockIdx.y ? out1 : out0;
  if (!out) return;                                          // (uniform over the workgroup)
  const int cl = threadIdx.x % kColCh, r = threadIdx.x / kColCh;
  const int c = static_cast<int>(blockIdx.x) * kColCh + cl;
  const float* col = partials + blockIdx.y * offset1 + c;
  float s = 0.f;
  if (c < C)
    for (int64_t p = r; p < rows; p += kColRows) s += col[p * row_stride];
  red[r][cl] = s;
  __syncthreads();
  if (r == 0 && c < C) {
    float t = red[0][cl];
    for (int q = 1; q < kColRows; ++q) t += red[q][cl];
    out[c] = t;
  }
}
// one sum: out1 = nullptr (a single row of workgroups)
static inline int column_partials_finish(const float* partials, float* out0, float* out1, int C, int64_t rows, int64_t row_stride,
                                         int64_t offset1, hipStream_t st) {
  hipLaunchKernelGGL(column_partials_finish_kernel, dim3(static_cast<unsigned>(ceil_div64(C, kColCh)), out1 ? 2 : 1),
                     dim3(kColCh * kColRows), 0, st, partials, out0, out1, C, rows, row_stride, offset1);
  return launch_status();
}
