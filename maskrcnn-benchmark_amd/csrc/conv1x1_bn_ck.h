// conv1x1_bn_ck.h — the composable_kernel (CK) side of csrc/conv1x1_bn.hip: the grouped-convolution forward template MIOpen
// already runs the backbone's fp32 1x1 convolutions through (DeviceGroupedConvFwdMultipleABD_Xdl_CShuffle, true fp32 MFMA),
// instantiated with THIS library's epilogue: y = [relu](acc * scale[k] + bias[k] [+ residual]).  The tile configurations are
// taken from CK's own instance lists (the ones MIOpen's tuning database names for these shapes), not re-typed here.
// Each conv1x1_bn_t*.hip instantiates a part of the (tile, stride, residual) grid so that the build stays parallel.
#pragma once
#include "detops_dtype.h"

struct Conv1x1BnArgs {
  const float* x;       // [N, H, W, C]
  const float* w;       // [K, C]
  const float* scale;   // [K]
  const float* bias;    // [K]
  const float* res;     // [N, Ho, Wo, K] or null
  float* y;             // [N, Ho, Wo, K]
  int N, C, H, W, K, stride, relu;
  hipStream_t st;
};

// tile configurations (the `config` argument of the C entry points)
constexpr int kConv1x1BnTile32 = 1;   // 256 threads, 64 x 128 x 16 block tile, 32x32x2 fp32 MFMA
constexpr int kConv1x1BnTile16 = 2;   // 256 threads, 64 x 64 x 32 block tile, 16x16x4 fp32 MFMA

// One function per translation unit; `check_only`: answer 0 / DETOPS_EUNSUPPORTED without launching.
int conv1x1_bn_t32_s1(const Conv1x1BnArgs& a, bool check_only);   // stride 1, with or without residual
int conv1x1_bn_t16_s1(const Conv1x1BnArgs& a, bool check_only);
int conv1x1_bn_s2(const Conv1x1BnArgs& a, int config, bool check_only);   // stride > 1 (no residual), both tiles

#if __has_include(<ck/library/tensor_operation_instance/gpu/grouped_conv_fwd/device_grouped_conv_fwd_xdl_instance.hpp>)
#define DETOPS_HAVE_CK 1
#ifdef DETOPS_CONV1X1_BN_INSTANTIATE
#include <array>
#include <map>
#include <mutex>
#include <tuple>
#include <type_traits>

#include <ck/library/tensor_operation_instance/gpu/grouped_conv_fwd/device_grouped_conv_fwd_xdl_instance.hpp>

namespace conv1x1_bn {

// The epilogue, in the operation order of frozen_bn_fwd_nhwc_kernel (csrc/frozen_bn.hip): product and sum rounded
// separately (no FMA), then the residual, then the library's ReLU rule (relu_fwd).
struct FrozenBnAct {
  template <typename E, typename C, typename S, typename B>
  __host__ __device__ void operator()(E& e, const C& c, const S& s, const B& b) const {
#pragma clang fp contract(off)
    float t = c * s + b;
    if (relu) t = relu_fwd(t);
    e = t;
  }
  template <typename E, typename C, typename S, typename B, typename R>
  __host__ __device__ void operator()(E& e, const C& c, const S& s, const B& b, const R& r) const {
#pragma clang fp contract(off)
    float t = c * s + b;
    t = t + r;
    if (relu) t = relu_fwd(t);
    e = t;
  }
  int relu;
};

namespace ckl = ck::tensor_layout::convolution;
namespace cki = ck::tensor_operation::device::instance;
using ck::tensor_operation::device::ConvolutionForwardSpecialization;

template <bool kRes>
using DsLayout = std::conditional_t<kRes, ck::Tuple<ckl::G_K, ckl::G_K, ckl::NHWGK>, ck::Tuple<ckl::G_K, ckl::G_K>>;
template <bool kRes>
using DsTypes = std::conditional_t<kRes, ck::Tuple<float, float, float>, ck::Tuple<float, float>>;

// <256, 64, 128, 16, 32, 32, 1, 2, 4-wide vectors> is the 12th entry of CK's fp32 list, <256, 64, 64, 32, 16, 16, 2, 2, 4-wide
// vectors> the third of its 16x16 list
template <bool kRes, ConvolutionForwardSpecialization kSpec>
using Tile32 = std::tuple_element_t<11, cki::device_grouped_conv_fwd_xdl_f32_instances<
    2, ckl::NHWGC, ckl::GKYXC, DsLayout<kRes>, ckl::NHWGK, kSpec, DsTypes<kRes>, FrozenBnAct>>;
template <bool kRes, ConvolutionForwardSpecialization kSpec>
using Tile16 = std::tuple_element_t<2, cki::device_grouped_conv_fwd_xdl_f32_16x16_instances<
    2, ckl::NHWGC, ckl::GKYXC, DsLayout<kRes>, ckl::NHWGK, kSpec, DsTypes<kRes>, FrozenBnAct>>;

// Builds the argument, asks the instance whether it serves it (the answer is kept per shape: the query reads the device
// properties several times) and launches.  Nothing but the kernel launch reaches the stream.
template <typename Op, bool kRes>
int run(const Conv1x1BnArgs& a, bool check_only) {
  using ck::index_t;
  constexpr int kD = kRes ? 3 : 2;
  const index_t N = a.N, C = a.C, H = a.H, W = a.W, K = a.K, s = a.stride;
  const index_t Ho = (H - 1) / s + 1, Wo = (W - 1) / s + 1;
  const std::array<index_t, 5> x_len{1, N, C, H, W}, x_str{C, H * W * C, 1, W * C, C};
  const std::array<index_t, 5> w_len{1, K, C, 1, 1}, w_str{K * C, C, 1, C, C};
  const std::array<index_t, 5> y_len{1, N, K, Ho, Wo}, y_str{K, Ho * Wo * K, 1, Wo * K, K};
  const std::array<index_t, 5> v_str{K, 0, 1, 0, 0};   // per-channel vector: every pixel reads the same K values
  std::array<const void*, kD> ds;
  std::array<std::array<index_t, 5>, kD> ds_len, ds_str;
  ds[0] = a.scale, ds[1] = a.bias;
  ds_len[0] = ds_len[1] = y_len;
  ds_str[0] = ds_str[1] = v_str;
  if constexpr (kRes) { ds[2] = a.res; ds_len[2] = y_len; ds_str[2] = y_str; }
  try {
    auto arg = Op::MakeArgument(a.x, a.w, ds, a.y, x_len, x_str, w_len, w_str, ds_len, ds_str, y_len, y_str, {s, s}, {1, 1},
                                {0, 0}, {0, 0}, ck::tensor_operation::element_wise::PassThrough{},
                                ck::tensor_operation::element_wise::PassThrough{}, FrozenBnAct{a.relu});
    static std::mutex mu;
    static std::map<std::array<int, 6>, bool> served;
    const std::array<int, 6> key{a.N, a.C, a.H, a.W, a.K, a.stride};
    bool ok;
    {
      std::lock_guard<std::mutex> lock(mu);
      auto it = served.find(key);
      if (it == served.end()) it = served.emplace(key, Op::IsSupportedArgument(arg)).first;
      ok = it->second;
    }
    if (!ok) return DETOPS_EUNSUPPORTED;
    if (check_only) return 0;
    Op::MakeInvoker().Run(arg, StreamConfig{a.st, false});
  } catch (const std::exception&) {
    const int e = static_cast<int>(hipGetLastError());
    return e ? e : DETOPS_EUNSUPPORTED;
  }
  return launch_status();
}

}  // namespace conv1x1_bn
#endif   // DETOPS_CONV1X1_BN_INSTANTIATE
#endif   // CK headers present
