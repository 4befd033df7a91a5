// conv1x1_bn_s2.hip — 1x1 convolution + FrozenBN epilogue (csrc/conv1x1_bn_ck.h): the strided form (a bottleneck's first
// convolution and its projection shortcut; neither takes a residual), both tiles.
#define DETOPS_CONV1X1_BN_INSTANTIATE
#include "conv1x1_bn_ck.h"

int conv1x1_bn_s2(const Conv1x1BnArgs& a, int config, bool check_only) {
#ifdef DETOPS_HAVE_CK
  using namespace conv1x1_bn;
  constexpr auto kSpec = ConvolutionForwardSpecialization::Filter1x1Pad0;
  if (a.res) return DETOPS_EUNSUPPORTED;
  return config == kConv1x1BnTile32 ? run<Tile32<false, kSpec>, false>(a, check_only)
                                    : run<Tile16<false, kSpec>, false>(a, check_only);
#else
  return DETOPS_EUNSUPPORTED;
#endif
}
