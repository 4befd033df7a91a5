// conv1x1_bn_t32_s1.hip — 1x1 convolution + FrozenBN epilogue (csrc/conv1x1_bn_ck.h): the 64 x 128 tile (32x32x2 fp32 MFMA),
// stride 1, with and without residual.
#define DETOPS_CONV1X1_BN_INSTANTIATE
#include "conv1x1_bn_ck.h"

int conv1x1_bn_t32_s1(const Conv1x1BnArgs& a, bool check_only) {
#ifdef DETOPS_HAVE_CK
  using namespace conv1x1_bn;
  constexpr auto kSpec = ConvolutionForwardSpecialization::Filter1x1Stride1Pad0;
  return a.res ? run<Tile32<true, kSpec>, true>(a, check_only) : run<Tile32<false, kSpec>, false>(a, check_only);
#else
  return DETOPS_EUNSUPPORTED;
#endif
}
