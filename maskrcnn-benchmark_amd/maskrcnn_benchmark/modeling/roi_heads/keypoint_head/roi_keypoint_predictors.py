"""Keypoint predictor (reference roi_heads/keypoint_head/roi_keypoint_predictors.py:8-36): a 4 x 4 stride-2 transposed
convolution to one logit map per keypoint (14 -> 28), then x2 bilinear upsampling (align_corners=False) to 56 x 56.  On a
channels-last input both keep the layout: the loss reads the logits through their strides."""
from torch import nn

from maskrcnn_benchmark.layers import ConvTranspose2d, interpolate
from maskrcnn_benchmark.layers.misc import conv_bias_act
from maskrcnn_benchmark.modeling import registry


@registry.ROI_KEYPOINT_PREDICTOR.register("KeypointRCNNPredictor")
class KeypointRCNNPredictor(nn.Module):
    def __init__(self, cfg, in_channels):
        super(KeypointRCNNPredictor, self).__init__()
        num_keypoints = cfg.MODEL.ROI_KEYPOINT_HEAD.NUM_CLASSES
        self.kps_score_lowres = ConvTranspose2d(in_channels, num_keypoints, 4, stride=2, padding=1)
        nn.init.kaiming_normal_(self.kps_score_lowres.weight, mode="fan_out", nonlinearity="relu")
        nn.init.constant_(self.kps_score_lowres.bias, 0)
        self.up_scale = 2
        self.out_channels = num_keypoints

    def forward(self, x):
        x = conv_bias_act(self.kps_score_lowres, x)
        return interpolate(x, scale_factor=self.up_scale, mode="bilinear", align_corners=False)


def make_roi_keypoint_predictor(cfg, in_channels):
    return registry.ROI_KEYPOINT_PREDICTOR[cfg.MODEL.ROI_KEYPOINT_HEAD.PREDICTOR](cfg, in_channels)
