"""ROIKeypointHead (reference roi_heads/keypoint_head/keypoint_head.py:9-50).

Training runs on the box head's positive slots, the way the mask head does (mask_head.py): the first `slots_per_image` slots
of every image (positives first; the counts come from the one asynchronous read-back the box head starts, or the fixed quota
under DETOPS_MASK_SLOTS=fixed / a captured graph), with the slots that are not keypoint ROIs masked out of the loss
(loss.py explains why that set equals the reference's re-matched and re-sampled one)."""
import torch

from ..mask_head.mask_head import keep_only_positive_boxes, slots_per_image
from .inference import make_roi_keypoint_post_processor
from .loss import make_roi_keypoint_loss_evaluator
from .roi_keypoint_feature_extractors import make_roi_keypoint_feature_extractor
from .roi_keypoint_predictors import make_roi_keypoint_predictor


class ROIKeypointHead(torch.nn.Module):
    def __init__(self, cfg, in_channels):
        super(ROIKeypointHead, self).__init__()
        if cfg.MODEL.ROI_KEYPOINT_HEAD.SHARE_BOX_FEATURE_EXTRACTOR:
            raise ValueError("MODEL.ROI_KEYPOINT_HEAD.SHARE_BOX_FEATURE_EXTRACTOR=True shares the box head's C4 feature "
                             "extractor; C4 keypoint models are not built here (set it to False, as the FPN configs do)")
        self.cfg = cfg.clone()
        self.feature_extractor = make_roi_keypoint_feature_extractor(cfg, in_channels)
        self.predictor = make_roi_keypoint_predictor(cfg, self.feature_extractor.out_channels)
        self.post_processor = make_roi_keypoint_post_processor(cfg)
        self.loss_evaluator = make_roi_keypoint_loss_evaluator(cfg)
        H = cfg.MODEL.ROI_HEADS
        self.max_positives = int(H.BATCH_SIZE_PER_IMAGE * H.POSITIVE_FRACTION)
        self.last_slots = None      # slot counts of the last training forward (one per image)

    def forward(self, features, proposals, targets=None):
        if self.training:
            all_proposals = proposals
            fixed = all(p.has_field("valid") for p in proposals)
            slots = slots_per_image(proposals, self.max_positives) if fixed else None
            self.last_slots = slots
            proposals, _ = keep_only_positive_boxes(proposals, slots)
        x = self.feature_extractor(features, proposals)
        kp_logits = self.predictor(x)
        if not self.training:
            return x, self.post_processor(kp_logits, proposals), {}
        loss_kp = self.loss_evaluator(proposals, kp_logits, targets)
        return x, all_proposals, dict(loss_kp=loss_kp)


def build_roi_keypoint_head(cfg, in_channels):
    return ROIKeypointHead(cfg, in_channels)
