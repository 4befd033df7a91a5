"""Keypoint-head feature extractor (reference roi_heads/keypoint_head/roi_keypoint_feature_extractors.py:10-49)."""
from torch import nn

from maskrcnn_benchmark.layers import Conv2d
from maskrcnn_benchmark.layers.misc import conv_bias_act
from maskrcnn_benchmark.modeling import registry
from maskrcnn_benchmark.modeling.poolers import make_pooler


@registry.ROI_KEYPOINT_FEATURE_EXTRACTORS.register("KeypointRCNNFeatureExtractor")
class KeypointRCNNFeatureExtractor(nn.Module):
    """multi-level ROIAlign (14 x 14) followed by CONV_LAYERS 3 x 3 conv + relu (`conv_fcn1` ... `conv_fcnN`)."""

    def __init__(self, cfg, in_channels):
        super(KeypointRCNNFeatureExtractor, self).__init__()
        self.pooler = make_pooler(cfg, "ROI_KEYPOINT_HEAD")
        self.blocks = []
        nxt = in_channels
        for i, width in enumerate(cfg.MODEL.ROI_KEYPOINT_HEAD.CONV_LAYERS, 1):
            conv = Conv2d(nxt, width, 3, stride=1, padding=1)
            nn.init.kaiming_normal_(conv.weight, mode="fan_out", nonlinearity="relu")
            nn.init.constant_(conv.bias, 0)
            name = "conv_fcn{}".format(i)
            self.add_module(name, conv)
            self.blocks.append(name)
            nxt = width
        self.out_channels = nxt

    def forward(self, x, proposals):
        x = self.pooler(x, proposals)
        for name in self.blocks:
            x = conv_bias_act(getattr(self, name), x, relu=True)
        return x


def make_roi_keypoint_feature_extractor(cfg, in_channels):
    return registry.ROI_KEYPOINT_FEATURE_EXTRACTORS[cfg.MODEL.ROI_KEYPOINT_HEAD.FEATURE_EXTRACTOR](cfg, in_channels)
