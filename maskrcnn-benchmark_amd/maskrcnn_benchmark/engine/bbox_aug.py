"""Test-time box augmentation (reference engine/bbox_aug.py): the detector runs over every image of a batch at several
scales and mirrored, and the detections of all passes are merged, NMS'd per class and limited once.

The reference transforms every PIL image on the host for every pass, maps each pass's BoxList back with transpose /
resize, concatenates them per image and runs filter_results' Python loop over the classes.  Here the raw bytes of the
batch go to the device once (data/collate_batch.py: RawImageBatch.on), every pass is one image_batch launch with its own
geometry records (RawImageBatch.prepare), and the merge of all passes of all images is one pair of HIP launches
(csrc/bbox_aug.hip through _C.bbox_aug_merge) that leaves one compact NMS segment per (image, class) — followed by ONE
segmented NMS call for the batch and the k-th-value limit of PostProcessor.filter_results."""
import torch

from maskrcnn_benchmark import _C
from maskrcnn_benchmark._bbox_aug_torch import group_records
from maskrcnn_benchmark.data.collate_batch import RawImageBatch
from maskrcnn_benchmark.structures.bounding_box import BoxList

NMS_SEGMENT_MAX = 65536      # boxes per segment the segmented NMS serves


def augmentation_passes(cfg):
    """[(min_size, max_size, flip)] in the reference's order (engine/bbox_aug.py:26-51): the identity pass, its flip, then
    every scale followed by its flip"""
    aug = cfg.TEST.BBOX_AUG
    out = [(cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST, False)]
    if aug.H_FLIP:
        out.append((cfg.INPUT.MIN_SIZE_TEST, cfg.INPUT.MAX_SIZE_TEST, True))
    for scale in aug.SCALES:
        out.append((scale, aug.MAX_SIZE, False))
        if aug.SCALE_H_FLIP:
            out.append((scale, aug.MAX_SIZE, True))
    return out


def merge_detections(boxes, scores, row_offset, group_geom, group_ratio, sizes, T, score_thresh, nms_thresh,
                     detections_per_img):
    """boxes [R, 4C], scores [R, C]: the unfiltered rows of every (image, pass) group, image-major (row_offset, group_geom,
    group_ratio: _C.bbox_aug_merge); sizes: per image the (w, h) of its first pass -> [BoxList] with `scores` and `labels`,
    class-major, candidate order inside a class (the convention of PostProcessor.filter_results)."""
    N, C = len(sizes), scores.shape[1]
    cand_boxes, cand_scores, seg_offsets, longest = _C.bbox_aug_merge(boxes, scores, row_offset, group_geom, group_ratio, N, T,
                                                                      score_thresh)
    if longest > NMS_SEGMENT_MAX:
        raise RuntimeError("bbox_aug: %d candidates of one class in one image, the segmented NMS serves %d"
                           % (longest, NMS_SEGMENT_MAX))
    dev = scores.device
    if cand_scores.numel():
        keep, _ = _C.nms_batched_mask(cand_boxes, cand_scores, seg_offsets, longest, nms_thresh)
        sel = keep.nonzero().squeeze(1)
    else:
        sel = torch.zeros((0,), dtype=torch.int64, device=dev)
    # the segment of a kept candidate: image * (C - 1) + (class - 1); candidates are segment-major already
    seg = torch.searchsorted(seg_offsets[1:].long(), sel, right=True)
    image = torch.div(seg, max(C - 1, 1), rounding_mode="floor")
    labels = seg - image * (C - 1) + 1
    per_image = torch.bincount(image, minlength=N).tolist() if N else []
    det_boxes, det_scores = cand_boxes[sel], cand_scores[sel]
    results = []
    for size, b, s, l in zip(sizes, det_boxes.split(per_image), det_scores.split(per_image), labels.split(per_image)):
        if 0 < detections_per_img < s.numel():
            # the reference thresholds at the k-th value (box_head/inference.py:139-146): ties at the threshold all stay
            thr = s.topk(detections_per_img).values[-1]
            top = (s >= thr).nonzero().squeeze(1)
            b, s, l = b[top], s[top], l[top]
        out = BoxList(b, size, mode="xyxy")
        out.add_field("scores", s)
        out.add_field("labels", l)
        results.append(out)
    return results


def im_detect_bbox_aug(model, images, device, cfg):
    """images: the RawImageBatch of a test loader under TEST.BBOX_AUG -> [BoxList] in the frame of the identity pass"""
    if not isinstance(images, RawImageBatch):
        raise ValueError("bbox_aug: every pass is prepared from the raw uint8 images of the batch (RawImageBatch, the deferred "
                         "input path), got %s" % type(images).__name__)
    if cfg.MODEL.RETINANET_ON or cfg.MODEL.RPN_ONLY or not cfg.TEST.BBOX_AUG.ENABLED:
        raise ValueError("bbox_aug merges the box head's per-class boxes: it needs a model with ROI heads that was built with "
                         "TEST.BBOX_AUG.ENABLED")
    C = cfg.MODEL.ROI_BOX_HEAD.NUM_CLASSES
    heads = cfg.MODEL.ROI_HEADS
    raw = images.on(device)
    passes = augmentation_passes(cfg)
    N, T = len(raw), len(passes)
    outputs = []                                      # [pass][image]: BoxList [n*C, 4] with scores [n*C], unfiltered
    for min_size, max_size, flip in passes:
        outputs.append(model(raw.prepare(min_size, max_size, flip)))
    groups = [outputs[t][i] for i in range(N) for t in range(T)]          # image-major
    rows = [len(g) // C for g in groups]
    row_offset = torch.tensor([0] + rows, dtype=torch.int64).cumsum(0).to(torch.int32)
    group_geom, group_ratio = group_records([[outputs[t][i].size for t in range(T)] for i in range(N)],
                                            [flip for _, _, flip in passes])
    dev = torch.device(device)
    if groups:
        boxes = torch.cat([g.bbox.reshape(-1, 4 * C) for g in groups])
        scores = torch.cat([g.get_field("scores").reshape(-1, C) for g in groups])
    else:
        boxes, scores = torch.zeros((0, 4 * C), device=dev), torch.zeros((0, C), device=dev)
    return merge_detections(boxes, scores, row_offset, group_geom, group_ratio, [outputs[0][i].size for i in range(N)], T,
                            heads.SCORE_THRESH, heads.NMS, heads.DETECTIONS_PER_IMG)
