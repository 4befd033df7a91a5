"""RPN head + module (reference modeling/rpn/rpn.py:14-208)."""
import os

import torch
import torch.nn.functional as F
from torch import nn

from maskrcnn_benchmark.layers.misc import conv_bias_act

from maskrcnn_benchmark.modeling import registry
from maskrcnn_benchmark.modeling.box_coder import BoxCoder

from .anchor_generator import make_anchor_generator
from .inference import make_rpn_postprocessor
from .loss import RPNLossComputation, make_rpn_loss_evaluator

# A/B switch of the sparse RPN-head backward: "0" the dense library backward (the previous behaviour), "1" (default) sparse
# where the static shape test says it pays, "force" sparse wherever the kernels serve the tensors (tests)
_SPARSE_BWD = os.environ.get("DETOPS_RPN_SPARSE_BWD", "1")
# The dense backward costs ~4 * 9 C^2 FLOP per pyramid pixel at the library's matrix-core rate, the sparse one the same per
# gradient ROW on plain FMA kernels an order of magnitude below that rate: it pays while rows * 16 <= pixels.
_SPARSE_PIXELS_PER_ROW = 16


class RPNHeadConvRegressor(nn.Module):
    """classification + regression heads without the shared 3x3 conv (reference :14-45)."""

    def __init__(self, cfg, in_channels, num_anchors):
        super(RPNHeadConvRegressor, self).__init__()
        self.cls_logits = nn.Conv2d(in_channels, num_anchors, kernel_size=1, stride=1)
        self.bbox_pred = nn.Conv2d(in_channels, num_anchors * 4, kernel_size=1, stride=1)
        for m in (self.cls_logits, self.bbox_pred):
            nn.init.normal_(m.weight, std=0.01)
            nn.init.constant_(m.bias, 0)

    def forward(self, x):
        assert isinstance(x, (list, tuple))
        return [self.cls_logits(y) for y in x], [self.bbox_pred(y) for y in x]


@registry.RPN_HEADS.register("SingleConvRPNHead")
class RPNHead(nn.Module):
    """3x3 conv + relu shared trunk, then 1x1 objectness (A) and 1x1 box deltas (4A) per level."""

    def __init__(self, cfg, in_channels, num_anchors):
        super(RPNHead, self).__init__()
        self.conv = nn.Conv2d(in_channels, in_channels, kernel_size=3, stride=1, padding=1)
        self.cls_logits = nn.Conv2d(in_channels, num_anchors, kernel_size=1, stride=1)
        self.bbox_pred = nn.Conv2d(in_channels, num_anchors * 4, kernel_size=1, stride=1)
        for m in (self.conv, self.cls_logits, self.bbox_pred):
            nn.init.normal_(m.weight, std=0.01)
            nn.init.constant_(m.bias, 0)

    def _sparse_ok(self, x, rows):
        if _SPARSE_BWD == "0" or not rows or not torch.is_grad_enabled() or torch.is_autocast_enabled():
            return False
        from maskrcnn_benchmark import _C
        # (the weights are read here, at forward time: HalfWeights swaps `module.weight` per step)
        params = (self.conv.weight, self.conv.bias, self.cls_logits.weight, self.cls_logits.bias, self.bbox_pred.weight,
                  self.bbox_pred.bias)
        if len(x) == 0 or not all(torch.is_tensor(p) for p in params) or not _C.rpn_head_sparse_supported(x, params):
            return False
        pixels = sum(int(f.shape[0]) * int(f.shape[2]) * int(f.shape[3]) for f in x)
        return _SPARSE_BWD == "force" or rows * _SPARSE_PIXELS_PER_ROW <= pixels

    def forward(self, x, sparse_rows=None):
        """`sparse_rows`: the caller's promise that at most this many anchors of the batch receive a non-zero gradient (the
        sampled RPN loss): the head then runs as one autograd node with the sparse backward where that pays.  Default:
        the dense per-level composition."""
        if sparse_rows is not None and self._sparse_ok(x, sparse_rows):
            from maskrcnn_benchmark import _C
            return _C.rpn_head_sparse(list(x), self.conv.weight, self.conv.bias, self.cls_logits.weight, self.cls_logits.bias,
                                      self.bbox_pred.weight, self.bbox_pred.bias, sparse_rows)
        logits, bbox_reg = [], []
        for feature in x:
            t = conv_bias_act(self.conv, feature, relu=True)      # channels-last: conv, then ONE fused bias + ReLU pass
            # the proposal / loss kernels read the A and 4A-channel outputs in NCHW; under a channels-last pyramid these two
            # small tensors are the only ones converted (a no-op for NCHW features)
            logits.append(conv_bias_act(self.cls_logits, t).contiguous())
            bbox_reg.append(conv_bias_act(self.bbox_pred, t).contiguous())
        return logits, bbox_reg


class RPNModule(nn.Module):
    """features -> proposals (+ RPN losses in training)."""

    def __init__(self, cfg, in_channels):
        super(RPNModule, self).__init__()
        self.cfg = cfg.clone()
        anchor_generator = make_anchor_generator(cfg)
        head = registry.RPN_HEADS[cfg.MODEL.RPN.RPN_HEAD](cfg, in_channels,
                                                          anchor_generator.num_anchors_per_location()[0])
        rpn_box_coder = BoxCoder(weights=(1.0, 1.0, 1.0, 1.0))
        self.anchor_generator = anchor_generator
        self.head = head
        self.box_selector_train = make_rpn_postprocessor(cfg, rpn_box_coder, is_train=True)
        self.box_selector_test = make_rpn_postprocessor(cfg, rpn_box_coder, is_train=False)
        self.loss_evaluator = make_rpn_loss_evaluator(cfg, rpn_box_coder)

    def _sparse_rows(self, features):
        """Upper bound on the anchors of the batch with a non-zero loss gradient, or None when there is no such bound: the
        sampled RPN loss evaluates <= BATCH_SIZE_PER_IMAGE anchors per image and nothing else backpropagates into the head
        (the proposals are taken under no_grad)."""
        if type(self.loss_evaluator) is not RPNLossComputation or type(self.head) is not RPNHead or len(features) == 0:
            return None
        A = self.anchor_generator.num_anchors_per_location()[0]
        per_image = A * sum(int(f.shape[2]) * int(f.shape[3]) for f in features)
        return int(features[0].shape[0]) * min(int(self.loss_evaluator.fg_bg_sampler.batch_size_per_image), per_image)

    def forward(self, images, features, targets=None):
        rows = self._sparse_rows(features) if self.training and targets is not None else None
        objectness, rpn_box_regression = self.head(features) if rows is None else self.head(features, sparse_rows=rows)
        anchors = self.anchor_generator(images, features)
        if self.training:
            return self._forward_train(anchors, objectness, rpn_box_regression, targets)
        return self._forward_test(anchors, objectness, rpn_box_regression)

    def _forward_train(self, anchors, objectness, rpn_box_regression, targets):
        if self.cfg.MODEL.RPN_ONLY:
            boxes = anchors  # proposals are not consumed; only the loss matters
        else:
            with torch.no_grad():  # end-to-end models do not backprop through the proposals
                boxes = self.box_selector_train(anchors, objectness, rpn_box_regression, targets)
        loss_objectness, loss_rpn_box_reg = self.loss_evaluator(anchors, objectness, rpn_box_regression, targets)
        return boxes, {"loss_objectness": loss_objectness, "loss_rpn_box_reg": loss_rpn_box_reg}

    def _forward_test(self, anchors, objectness, rpn_box_regression):
        boxes = self.box_selector_test(anchors, objectness, rpn_box_regression)
        if self.cfg.MODEL.RPN_ONLY:
            boxes = [b[b.get_field("objectness").sort(descending=True)[1]] for b in boxes]
        return boxes, {}


def build_rpn(cfg, in_channels):
    if cfg.MODEL.RETINANET_ON:
        from .retinanet.retinanet import build_retinanet
        return build_retinanet(cfg, in_channels)
    return RPNModule(cfg, in_channels)
