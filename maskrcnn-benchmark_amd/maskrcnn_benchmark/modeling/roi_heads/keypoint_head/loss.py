"""Keypoint loss and keypoint targets (reference roi_heads/keypoint_head/loss.py:55-183).

Which ROIs.  The reference matches and samples the box head's sampled proposals a second time (`subsample`, loss.py:79-143).
With the matcher thresholds of the box head (FG = BG = 0.5: no between-threshold band) the re-match gives back the box head's
`matched_idxs`, and its positive quota (BATCH_SIZE_PER_IMAGE * POSITIVE_FRACTION) is never smaller than the number of
candidates, which are the box head's positives already capped at that quota; its random stream only picks negatives, which
`subsample` then drops.  So the reference's keypoint ROIs are exactly the box head's positive slots whose matched ground
truth has at least one labelled (v > 0) keypoint inside its own box.  Here the keypoint head takes the box head's
positives-first slots (mask_head.keep_only_positive_boxes: the slot counts and the one asynchronous read-back are the mask
head's) and the slots that do not qualify are masked out of the loss instead of being compacted with `nonzero`.

The loss.  Mean softmax cross-entropy over the valid (ROI, keypoint) rows of the M x M logits; 0 without valid rows
(loss.py:160-163).  The reference selects the valid rows with a second `nonzero`; on the device one kernel here forms the
value, the gradient and the normaliser (csrc/keypoint.hip) — no host wait.  The torch formulation below is the CPU path and
the yardstick of the kernels.
"""
import torch

from maskrcnn_benchmark import _C
from maskrcnn_benchmark.structures.keypoint import keypoints_to_heat_map


def within_box(points, boxes):
    """points [n, K, 2], boxes [n, 4] xyxy -> [n, K] bool, edges inclusive"""
    x, y = points[..., 0], points[..., 1]
    return (x >= boxes[:, 0, None]) & (x <= boxes[:, 2, None]) & (y >= boxes[:, 1, None]) & (y <= boxes[:, 3, None])


def keypoint_slots(matched, labels, gt_boxes, gt_keypoints):
    """-> [P] bool: the slot is a keypoint ROI of the reference (loss.py:93-100): positive, and its matched ground truth has
    a labelled (v > 0) keypoint inside its own box"""
    G = gt_keypoints.shape[0]
    if G == 0:
        return torch.zeros_like(labels, dtype=torch.bool)
    g = matched.clamp(min=0, max=G - 1)
    kp = gt_keypoints[g]
    gt_ok = (within_box(kp[..., :2], gt_boxes[g]) & (kp[..., 2] > 0)).any(dim=1)
    return (labels > 0) & (matched >= 0) & (matched < G) & gt_ok


def keypoint_targets_torch(boxes, matched, labels, gt_boxes, gt_keypoints, heatmap_size):
    """the torch formulation of `_C.keypoint_targets` (same arguments and results)"""
    P, K = boxes.shape[0], gt_keypoints.shape[1]
    if P == 0 or gt_keypoints.shape[0] == 0:
        z = torch.zeros((P, K), dtype=torch.int64, device=boxes.device)
        return z, z.bool()
    slot_ok = keypoint_slots(matched, labels, gt_boxes, gt_keypoints)
    heat, valid = keypoints_to_heat_map(gt_keypoints[matched.clamp(min=0)], boxes, heatmap_size)
    valid = valid.bool() & slot_ok[:, None]
    return heat * valid, valid


def keypoint_loss_torch(logits, heatmaps, valid):
    """the torch formulation of `_C.keypoint_loss`: mean cross-entropy of the valid rows, 0 without any"""
    P, K, H, W = logits.shape
    x = logits.reshape(P * K, H * W).float()
    v = valid.reshape(-1)
    per_row = torch.logsumexp(x, dim=1) - x.gather(1, heatmaps.reshape(-1, 1)).squeeze(1)
    per_row = torch.where(v, per_row, torch.zeros_like(per_row))
    return per_row.sum() / v.sum().clamp(min=1).to(per_row.dtype)


class KeypointRCNNLossComputation(object):
    def __init__(self, discretization_size):
        self.discretization_size = discretization_size

    def batch(self, proposals, targets, num_keypoints):
        """-> (boxes [P, 4], matched [P] (rows of the batch's concatenated ground truth), labels [P], gt_boxes [G, 4],
        gt_keypoints [G, K, 3]) of the keypoint head's slots, image after image"""
        dev = proposals[0].bbox.device
        boxes = torch.cat([p.convert("xyxy").bbox for p in proposals], dim=0)
        labels = torch.cat([p.get_field("labels") for p in proposals], dim=0)
        matched, base = [], 0
        for p, t in zip(proposals, targets):
            m = p.get_field("matched_idxs")
            matched.append(torch.where(m >= 0, m + base, m))
            base += len(t)
        matched = torch.cat(matched, dim=0)
        gt_boxes = torch.cat([t.convert("xyxy").bbox for t in targets], dim=0).to(dev)
        # explicit K: an image without instances holds a 1-D empty keypoint tensor (Keypoints keeps it as given)
        gt_kps = torch.cat([t.get_field("keypoints").keypoints.reshape(len(t), num_keypoints, 3) for t in targets],
                           dim=0).to(dev)
        return boxes, matched, labels, gt_boxes, gt_kps

    def targets(self, proposals, targets, num_keypoints=17):
        """-> (heatmaps [P, K] int64, valid [P, K] bool) of the keypoint head's slots, image after image"""
        boxes, matched, labels, gt_boxes, gt_kps = self.batch(proposals, targets, num_keypoints)
        if _C.on_device(boxes):
            return _C.keypoint_targets(boxes, matched, labels, gt_boxes, gt_kps, self.discretization_size)
        return keypoint_targets_torch(boxes, matched, labels, gt_boxes, gt_kps, self.discretization_size)

    def __call__(self, proposals, keypoint_logits, targets):
        """proposals: the keypoint head's positives-first slots (fields labels, matched_idxs); keypoint_logits [sum P, K, M, M]"""
        if keypoint_logits.shape[0] == 0:
            return keypoint_logits.sum() * 0
        heatmaps, valid = self.targets(proposals, targets, keypoint_logits.shape[1])
        logits = keypoint_logits.float()     # autocast: half logits are cast first (as the mask loss does)
        if _C.on_device(logits):
            return _C.keypoint_loss(logits, heatmaps, valid)
        return keypoint_loss_torch(logits, heatmaps, valid)


def make_roi_keypoint_loss_evaluator(cfg):
    return KeypointRCNNLossComputation(cfg.MODEL.ROI_KEYPOINT_HEAD.RESOLUTION)
