"""Keypoint evaluation: COCO-style AP / AR under object keypoint similarity (OKS), as a streaming evaluator, and the way
back from `keypoints.json`.

Per batch the OKS matrix of every (image, category) problem is computed where the tensors live (on the device:
csrc/eval_oks.hip through maskrcnn_benchmark._C.eval_oks; CPU tensors: _eval_cpu.eval_oks), matched by the same
_C.eval_match as boxes and masks, and only the match records are kept; coco_style.accumulate turns them into precision and
recall once, on the host.

The rules (include/detops.h, "Keypoint evaluation (OKS)") are a restatement of pycocotools.cocoeval — computeOks, the
keypoint branches of _prepare, evaluateImg and setKpParams, and loadRes for keypoint results — written from knowledge of
that code.  It has NOT been checked against pycocotools, which is not available where this project is built and tested;
tests/oks_refs.py is the literal, loop-by-loop form everything here is pinned to.  The sum of an OKS runs in keypoint
order, so its last bits are this library's choice.

These are names of their own: the generic entry points (`evaluate`, `COCOStyleEvaluator`, `load_results`,
`evaluate_result_files`, `inference(iou_types=...)`) still refuse "keypoints"; `inference(keypoint_oks=True)` and
tools/evaluate_keypoints.py are the way in.
"""
import os

import numpy as np
import torch

from maskrcnn_benchmark import _C, _eval_cpu
from maskrcnn_benchmark.structures.keypoint import PersonKeypoints

from . import coco_style
from .coco_results import _group_entries, _scored_boxlist
from .coco_style import _feed, _num_classes

IOU_THRS, REC_THRS = coco_style.IOU_THRS, coco_style.REC_THRS
AREA_RNGS = np.array([[0, 1e10], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]], dtype=np.float64)      # all, medium, large
MAX_DETS = (20,)
STAT_NAMES = tuple(row[0] for row in coco_style.STAT_ROWS["keypoints"])
COCO_PERSON_SIGMAS = _eval_cpu.COCO_PERSON_SIGMAS


def _keypoint_tensor(boxlist, K, dev):
    """the [n, K, 3] fp32 tensor of a BoxList's `keypoints` field (a Keypoints or a tensor), on `dev`"""
    kp = boxlist.get_field("keypoints")
    kp = kp.keypoints if hasattr(kp, "keypoints") else kp
    kp = torch.as_tensor(kp, dtype=torch.float32).to(dev)
    if kp.numel() == 0:
        return kp.reshape(0, K, 3)
    if kp.dim() != 3 or kp.shape[1] != K or kp.shape[2] != 3 or kp.shape[0] != len(boxlist):
        raise ValueError("keypoints of shape %s for %d instances of K = %d keypoints" % (tuple(kp.shape), len(boxlist), K))
    return kp


def _keypoints_of(boxlists, K, dev):
    """the keypoints of a batch's BoxLists, one after the other: fp32 [n, K, 3]; an empty BoxList needs no field"""
    f32 = dict(dtype=torch.float32, device=dev)
    parts = [_keypoint_tensor(x, K, dev) if len(x) else torch.zeros((0, K, 3), **f32) for x in boxlists]
    return torch.cat(parts) if parts else torch.zeros((0, K, 3), **f32)


class KeypointOKSEvaluator(coco_style.COCOStyleEvaluator):
    """evaluator = KeypointOKSEvaluator(num_classes, sigmas); evaluator.update(predictions, targets) per batch;
    evaluator.summarize() -> {"keypoints": the 10 numbers AP, AP50, AP75, APm, APl, AR, AR50, AR75, ARm, ARl}.
    A COCOStyleEvaluator in what it keeps (the match records) and how it accumulates them; its own are the similarity, the
    area ranges, the cut to 20 detections and the ten statistics.

    sigmas: the per-keypoint constants, fp64 [K] (default: the 17 of the COCO person table).  Labels are the contiguous
    ones (1 .. num_classes - 1).  At most 20 detections per (image, category) are matched.

    update(predictions, targets): two lists of BoxList (one per image), on the device or the CPU.  Predictions carry
    `scores`, `labels` and `keypoints` [n, K, 3] (a Keypoints or a tensor; the third column is not read); targets carry
    `labels`, `keypoints` (third column: the visibility flag) and may carry `iscrowd`, `area` and `masks`."""

    iou_types = ("keypoints",)

    def __init__(self, num_classes=2, sigmas=None):
        self.num_classes = int(num_classes)
        self.sigmas = np.asarray(COCO_PERSON_SIGMAS if sigmas is None else sigmas, dtype=np.float64).reshape(-1)
        if self.sigmas.size < 1 or not (self.sigmas > 0).all():
            raise ValueError("KeypointOKSEvaluator: sigmas must be K >= 1 positive numbers")
        self.iou_thrs, self.rec_thrs, self.area_rngs, self.max_dets = IOU_THRS, REC_THRS, AREA_RNGS, MAX_DETS
        self.records = {"keypoints": []}
        self.num_images = self.num_detections = self.num_groundtruths = 0
        self.eval = {}

    # ------------------------------------------------------------------ per batch: its part of COCOStyleEvaluator.update
    def _check_fields(self, predictions, targets):
        for pred, tgt in zip(predictions, targets):
            if len(tgt) and not tgt.has_field("keypoints"):
                raise ValueError("keypoint evaluation needs ground-truth keypoints")
            if len(pred) and not pred.has_field("keypoints"):
                raise ValueError("keypoint evaluation needs predictions with a `keypoints` field")

    def _similarity(self, iou_type, b, pr, offs, gt_area, dt_pack, gt_pack):
        K, dev = self.sigmas.size, b.gt_box.device
        do, go = pr["dt_order"], pr["gt_order"]
        dt_kp, gt_kp = _keypoints_of(b.preds, K, dev), _keypoints_of(b.tgts, K, dev)
        oks, dt_area = _C.eval_oks(dt_kp[do], gt_kp[go], b.gt_box[go], gt_area[go], self.sigmas, *offs, pr["total_pairs"])
        # no visible keypoint and no crowd: ignored in every range and not matched again (area -1 lies outside every range)
        unlabelled = ((gt_kp[:, :, 2] > 0).sum(dim=1) == 0) & ~b.gt_ignore
        return oks, dt_area, torch.where(unlabelled, torch.full_like(gt_area, -1.0), gt_area)


def summarize(ev, iou_thrs=IOU_THRS):
    """-> the 10 numbers (STAT_NAMES): the mean of the cells greater than -1, or -1 when there are none"""
    return coco_style.summarize(ev, iou_thrs, coco_style.STAT_ROWS["keypoints"])


# ------------------------------------------------------------------------------------------------ keypoints.json
def load_keypoint_results(path_or_list, dataset, device=None):
    """A `keypoints.json` result file (a path, or its list of entries) -> a list of BoxList in dataset order, what
    KeypointOKSEvaluator.update takes: the inverse of coco_results.keypoint_entries, with the id and label maps of
    load_results (coco_results._group_entries; the file's order is kept inside an image).
    `keypoints` is the flat list of 3 K numbers and becomes a PersonKeypoints field [n, K, 3]; the box is the keypoints'
    extents (min x, min y, max x, max y), as pycocotools' loadRes makes it.  ValueError: an unknown image id or category id,
    a keypoint list whose length is no multiple of 3 or differs inside the file."""
    entries, per_image, labels_of = _group_entries(path_or_list, dataset)
    K = None
    for e in entries:
        n = len(e.get("keypoints", ()))
        if n == 0 or n % 3 or (K is not None and n != 3 * K):
            raise ValueError("result files: %d keypoint numbers (image %r): expected the same multiple of 3 in every entry"
                             % (n, e["image_id"]))
        K = n // 3
    device = torch.device("cpu" if device is None else device)
    K = 17 if K is None else K
    out = []
    for index, es in enumerate(per_image):
        info = dataset.get_img_info(index)
        W, H = int(info["width"]), int(info["height"])
        kp = torch.tensor([e["keypoints"] for e in es], dtype=torch.float32).reshape(-1, K, 3)
        if len(es):
            lo, hi = kp[:, :, :2].min(dim=1)[0], kp[:, :, :2].max(dim=1)[0]
            boxes = torch.cat([lo, hi], dim=1)
        else:
            boxes = torch.zeros((0, 4), dtype=torch.float32)
        boxlist = _scored_boxlist(boxes, (W, H), "xyxy", es, labels_of)
        boxlist.add_field("keypoints", PersonKeypoints(kp, (W, H)))
        out.append(boxlist.to(device))
    return out


def evaluate_keypoint_file(dataset, path_or_list, output_folder=None, batch=8, device="cpu", sigmas=None, expected_results=(),
                           expected_results_sigma_tol=4):
    """Score a saved `keypoints.json` (a path, or its list of entries) against `dataset`'s ground truth: one
    KeypointOKSEvaluator fed `batch` images at a time on `device` -> the COCOResults of finish_coco, which also logs the
    table and, with `output_folder`, writes coco_results.pth / coco_results.txt."""
    from . import finish_coco

    device = torch.device(device)
    predictions = load_keypoint_results(path_or_list, dataset, device)
    evaluator = _feed(KeypointOKSEvaluator(_num_classes(dataset, 2), sigmas), predictions, dataset, batch, device)
    if output_folder:
        os.makedirs(output_folder, exist_ok=True)
    return finish_coco(evaluator, output_folder, expected_results, expected_results_sigma_tol)
