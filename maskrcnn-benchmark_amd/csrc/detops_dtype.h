// detops_dtype.h — what the elementwise and loss kernels share: storage-type I/O, 16-byte vectors, the host-side step from
// a run-time dtype code / vector width / flag to a template argument, and single-value wave reductions.  Only helpers with
// at least two users live here.
#pragma once
#include <initializer_list>
#include <type_traits>

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
