// conv1x1_bn.hip — the backbone's 1x1 convolution with FrozenBatchNorm (+ residual) (+ ReLU) folded into its epilogue, fp32,
// channels-last, for gfx950 (MI355X):  y[n, ho, wo, k] = [relu]( (sum_c x[n, ho*s, wo*s, c] * w[k, c]) * scale[k] + bias[k]
// [+ residual[n, ho, wo, k]] ).
//
// Why: after every convolution of a bottleneck the FrozenBN pass (csrc/frozen_bn.hip) re-reads the convolution's output
// and writes it again — pure HBM traffic for two FLOPs per element the convolution kernel could have applied while the
// tile was in registers.  The convolution itself is NOT re-written here: it is the composable_kernel template MIOpen
// already picks for these shapes (csrc/conv1x1_bn_ck.h), with this library's epilogue as its output operation.
// This file holds the C entry points, the argument checks and the per-shape routing table.
#include "conv1x1_bn_ck.h"

namespace {

// (C, K, stride, smallest number of output rows N*Ho*Wo) -> tile configuration.  Filled from measurement on an MI355X
// (profiles/conv1x1_bn_opbench.txt: the fused launch against MIOpen's convolution + the FrozenBN launch, device time, at
// the R-50 backbone's shapes for 2 and for 1 image of 800 x 1344).  Listed: the fused launch is at least 5 % faster at
// both row counts; min_rows is the smaller of the two.  A shape that is not listed, or has fewer rows than measured,
// keeps the two-launch path — among the backbone's, 1024 -> 256, 1024 -> 512 / 2 and 2048 -> 512 (res4 / res5, K loops of
// 64 - 128 tiles over 2100 - 8400 rows), where neither tile beats MIOpen's choice at 2 images.
// In the comments: us of the pair -> us fused, 2 images | 1 image.
struct Route { int C, K, stride; int64_t min_rows; int config; };
constexpr Route kRoutes[] = {
    {64, 64, 1, 67200, kConv1x1BnTile16},      //  29.7 -> 20.5 |  35.1 -> 13.9
    {64, 256, 1, 67200, kConv1x1BnTile32},     // 111.6 -> 65.5 |  74.6 -> 33.8 with residual; 90.2 -> 49.2 | 68.6 -> 29.1 without
    {256, 64, 1, 67200, kConv1x1BnTile16},     //  59.1 -> 48.3 |  59.6 -> 30.3
    {256, 128, 2, 16800, kConv1x1BnTile16},    //  35.2 -> 30.3 |  35.2 -> 20.6
    {128, 512, 1, 16800, kConv1x1BnTile32},    //  74.9 -> 48.7 |  64.9 -> 30.5
    {256, 512, 2, 16800, kConv1x1BnTile16},    // 100.4 -> 83.6 |  93.9 -> 48.1
    {512, 128, 1, 16800, kConv1x1BnTile16},    //  55.6 -> 52.5 |  55.3 -> 34.8
    {512, 256, 2, 4200, kConv1x1BnTile16},     //  37.9 -> 34.6 |  42.1 -> 25.3
    {256, 1024, 1, 4200, kConv1x1BnTile16},    //  64.0 -> 49.0 |  70.2 -> 30.5
    {512, 1024, 2, 4200, kConv1x1BnTile16},    //  96.4 -> 85.2 | 117.7 -> 51.5
    {512, 2048, 1, 1050, kConv1x1BnTile16},    //  58.0 -> 52.3 |  55.7 -> 34.8
    {1024, 2048, 2, 1050, kConv1x1BnTile16},   // 104.7 -> 95.2 |  94.8 -> 61.0
};

int route(int C, int K, int stride, int64_t rows) {
  for (const Route& r : kRoutes)
    if (r.C == C && r.K == K && r.stride == stride && rows >= r.min_rows) return r.config;
  return 0;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// shape limits of the entry points (the instance's own IsSupportedArgument comes on top)
bool shape_ok(int N, int C, int H, int W, int K, int stride) {
  if (N < 1 || C < 4 || K < 4 || H < 1 || W < 1 || (stride != 1 && stride != 2)) return false;
  if (C % 4 || K % 4) return false;
  const int64_t Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
  const int64_t lim = 0x7fffffff;
  return static_cast<int64_t>(N) * H * W * C < lim && N * Ho * Wo * K < lim && static_cast<int64_t>(K) * C < lim;
}

int dispatch(const Conv1x1BnArgs& a, int config, bool check_only) {
  if (a.stride != 1) return conv1x1_bn_s2(a, config, check_only);
  return config == kConv1x1BnTile32 ? conv1x1_bn_t32_s1(a, check_only) : conv1x1_bn_t16_s1(a, check_only);
}

}  // namespace

// -> the tile configuration (1 | 2) that serves the shape, 0 = not served.  config 0 asks the routing table (0 then also
// means "the two-launch path is at least as fast"), 1 | 2 ask for that tile.  Needs a current HIP device.
DETOPS_API int detops_conv1x1_frozen_bn_act_supported(int N, int C, int H, int W, int K, int stride, int residual,
                                                      int config) {
#ifdef DETOPS_HAVE_CK
  if (config < 0 || config > kConv1x1BnTile16 || !shape_ok(N, C, H, W, K, stride) || (residual && stride != 1)) return 0;
  const int64_t rows = static_cast<int64_t>(N) * ((H - 1) / stride + 1) * ((W - 1) / stride + 1);
  if (config == 0) config = route(C, K, stride, rows);
  if (config == 0) return 0;
  static const float kDummy[4] = {0.f, 0.f, 0.f, 0.f};   // IsSupportedArgument reads no memory
  const Conv1x1BnArgs a{kDummy, kDummy, kDummy, kDummy, residual ? kDummy : nullptr, nullptr, N, C, H, W, K, stride, 0, nullptr};
  return dispatch(a, config, true) == 0 ? config : 0;
#else
  return 0;
#endif
}

DETOPS_API int detops_conv1x1_frozen_bn_act_forward_nhwc_f32(const float* x, const float* w, const float* scale,
                                                             const float* bias, const float* residual, float* y, int N,
                                                             int C, int H, int W, int K, int stride, int relu, int config,
                                                             detops_stream_t stream) {
  if (N < 0 || C < 0 || H < 0 || W < 0 || K < 0) return DETOPS_EINVAL;
  if (!x || !w || !scale || !bias || !y) return DETOPS_EINVAL;
  if (config < 0 || config > kConv1x1BnTile16 || !shape_ok(N, C, H, W, K, stride) || (residual && stride != 1))
    return DETOPS_EUNSUPPORTED;
  if (!aligned16(x) || !aligned16(w) || !aligned16(scale) || !aligned16(bias) || !aligned16(residual) || !aligned16(y))
    return DETOPS_EUNSUPPORTED;
  if (config == 0) config = route(C, K, stride, static_cast<int64_t>(N) * ((H - 1) / stride + 1) * ((W - 1) / stride + 1));
  if (config == 0) return DETOPS_EUNSUPPORTED;
  const Conv1x1BnArgs a{x, w, scale, bias, residual, y, N, C, H, W, K, stride, relu ? 1 : 0, as_stream(stream)};
  return dispatch(a, config, false);
}
