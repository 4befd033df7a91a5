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
from collections import OrderedDict

import numpy as np
import torch

from maskrcnn_benchmark import _C, _eval_cpu
from maskrcnn_benchmark.structures.bounding_box import BoxList
from maskrcnn_benchmark.structures.keypoint import PersonKeypoints

from . import coco_style

IOU_THRS, REC_THRS = coco_style.IOU_THRS, coco_style.REC_THRS
AREA_RNGS = np.array([[0, 1e10], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]], dtype=np.float64)      # all, medium, large
MAX_DETS = (20,)
STAT_NAMES = ("AP", "AP50", "AP75", "APm", "APl", "AR", "AR50", "AR75", "ARm", "ARl")
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


class KeypointOKSEvaluator(coco_style.COCOStyleEvaluator):
    """evaluator = KeypointOKSEvaluator(num_classes, sigmas); evaluator.update(predictions, targets) per batch;
    evaluator.summarize() -> {"keypoints": the 10 numbers AP, AP50, AP75, APm, APl, AR, AR50, AR75, ARm, ARl}.
    A COCOStyleEvaluator in what it keeps (the match records) and how it accumulates them; its own are the similarity, the
    area ranges, the cut to 20 detections and the ten statistics.

    sigmas: the per-keypoint constants, fp64 [K] (default: the 17 of the COCO person table).  Labels are the contiguous
    ones (1 .. num_classes - 1).  At most 20 detections per (image, category) are matched."""

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

    # ------------------------------------------------------------------ per batch
    def update(self, predictions, targets):
        """predictions, targets: two lists of BoxList (one per image), on the device or the CPU.  Predictions carry
        `scores`, `labels` and `keypoints` [n, K, 3] (a Keypoints or a tensor; the third column is not read); targets carry
        `labels`, `keypoints` (third column: the visibility flag) and may carry `iscrowd`, `area` and `masks`."""
        assert len(predictions) == len(targets), "one prediction per target"
        K = self.sigmas.size
        dev = targets[0].bbox.device if targets else torch.device("cpu")
        preds, tgts = [], []
        for pred, tgt in zip(predictions, targets):
            tgt = tgt.convert("xyxy")
            if tuple(pred.size) != tuple(tgt.size):
                pred = pred.resize(tgt.size)
            if len(tgt) and not tgt.has_field("keypoints"):
                raise ValueError("keypoint evaluation needs ground-truth keypoints")
            if len(pred) and not pred.has_field("keypoints"):
                raise ValueError("keypoint evaluation needs predictions with a `keypoints` field")
            preds.append(pred.to(dev))
            tgts.append(tgt)
        n_dt, n_gt = [len(p) for p in preds], [len(t) for t in tgts]
        i64 = dict(dtype=torch.int64, device=dev)
        img = torch.arange(len(preds), **i64) + self.num_images
        dt_img, gt_img = img.repeat_interleave(torch.tensor(n_dt, **i64)), img.repeat_interleave(torch.tensor(n_gt, **i64))
        cat = lambda ts, **kw: torch.cat(ts) if ts else torch.zeros((0,), **kw)  # noqa: E731
        f32 = dict(dtype=torch.float32, device=dev)
        dt_kp = cat([_keypoint_tensor(p, K, dev) if len(p) else torch.zeros((0, K, 3), **f32) for p in preds], **f32).reshape(-1, K, 3)
        gt_kp = cat([_keypoint_tensor(t, K, dev) if len(t) else torch.zeros((0, K, 3), **f32) for t in tgts], **f32).reshape(-1, K, 3)
        gt_box = cat([t.bbox for t in tgts]).reshape(-1, 4)
        dt_label = cat([p.get_field("labels").to(**i64) for p in preds], **i64)
        gt_label = cat([t.get_field("labels").to(**i64) for t in tgts], **i64)
        dt_score = cat([p.get_field("scores").reshape(-1) for p in preds], device=dev)
        gt_crowd = cat([(t.get_field("iscrowd").to(dev) != 0) if t.has_field("iscrowd") else torch.zeros((len(t),), dtype=torch.bool, device=dev)
                        for t in tgts], dtype=torch.bool, device=dev)
        for name, lab in (("prediction", dt_label), ("target", gt_label)):
            if lab.numel() and (int(lab.min()) < 0 or int(lab.max()) >= self.num_classes):
                raise ValueError("%s labels must lie in [0, %d), got %d .. %d" % (name, self.num_classes, int(lab.min()), int(lab.max())))
        self.num_images += len(preds)
        self.num_detections += sum(n_dt)
        self.num_groundtruths += sum(n_gt)
        pr = coco_style.build_problems(dt_img, dt_label, dt_score, gt_img, gt_label, self.num_classes, max_dets=MAX_DETS[-1])
        do, go = pr["dt_order"], pr["gt_order"]
        gt_pack = coco_style._pack_masks(coco_style.groundtruth_planes(tgts, dev)) if coco_style.needs_mask_area(tgts) else None
        gt_area = coco_style.groundtruth_area(tgts, gt_box, gt_pack)
        offs = (pr["dt_offset"], pr["gt_offset"], pr["iou_offset"])
        oks, dt_area = _C.eval_oks(dt_kp[do], gt_kp[go], gt_box[go], gt_area[go], self.sigmas, *offs, pr["total_pairs"])
        # no visible keypoint and no crowd: ignored in every range and not matched again (area -1 lies outside every range)
        unlabelled = ((gt_kp[:, :, 2] > 0).sum(dim=1) == 0) & ~gt_crowd
        match_area = torch.where(unlabelled, torch.full_like(gt_area, -1.0), gt_area)
        dtm, dti, gti = _C.eval_match(_C.EVAL_COCO_BBOX, oks, *offs, pr["counts_host"], gt_crowd[go], torch.from_numpy(self.iou_thrs),
                                      dt_area=dt_area, gt_area=match_area[go], area_rngs=torch.from_numpy(self.area_rngs))
        self._keep("keypoints", pr, dt_score[do].to(torch.float64).cpu().numpy(), dtm.cpu().numpy(), dti.cpu().numpy(),
                   gti.cpu().numpy())

    # ------------------------------------------------------------------ once per evaluation
    def summarize(self):
        self.accumulate()
        self.stats = OrderedDict([("keypoints", summarize(self.eval["keypoints"], self.iou_thrs))])
        return self.stats


def summarize(ev, iou_thrs=IOU_THRS):
    """-> the 10 numbers (STAT_NAMES): the mean of the cells greater than -1, or -1 when there are none"""
    def stat(ap, thr=None, area=0):
        s = ev["precision"] if ap else ev["recall"]
        if thr is not None:
            s = s[np.nonzero(np.isclose(iou_thrs, thr))[0]]
        s = s[:, :, :, area, 0] if ap else s[:, :, area, 0]
        s = s[s > -1]
        return float(np.mean(s)) if s.size else -1.0

    return np.array([stat(1), stat(1, 0.5), stat(1, 0.75), stat(1, area=1), stat(1, area=2),
                     stat(0), stat(0, 0.5), stat(0, 0.75), stat(0, area=1), stat(0, area=2)])


# ------------------------------------------------------------------------------------------------ keypoints.json
def load_keypoint_results(path_or_list, dataset, device=None):
    """A `keypoints.json` result file (a path, or its list of entries) -> a list of BoxList in dataset order, what
    KeypointOKSEvaluator.update takes: the inverse of coco_results.keypoint_entries, with the id and label maps of
    load_results (entries grouped by `image_id` through the inverse of `id_to_img_map`, the file's order kept inside an
    image; labels through `json_category_id_to_contiguous_id`; a dataset without these maps uses the index and the label).
    `keypoints` is the flat list of 3 K numbers and becomes a PersonKeypoints field [n, K, 3]; the box is the keypoints'
    extents (min x, min y, max x, max y), as pycocotools' loadRes makes it.  ValueError: an unknown image id or category id,
    a keypoint list whose length is no multiple of 3 or differs inside the file."""
    from .coco_results import _read_entries

    entries = _read_entries(path_or_list)
    ids = getattr(dataset, "id_to_img_map", None)
    index_of = {v: k for k, v in ids.items()} if ids is not None else None
    labels_of = getattr(dataset, "json_category_id_to_contiguous_id", None)
    if labels_of is None and getattr(dataset, "contiguous_category_id_to_json_id", None) is not None:
        labels_of = {v: k for k, v in dataset.contiguous_category_id_to_json_id.items()}
    per_image = [[] for _ in range(len(dataset))]
    K = None
    for e in entries:
        image_id = e["image_id"]
        index = index_of.get(image_id) if index_of is not None else (image_id if isinstance(image_id, int) else None)
        if index is None or not 0 <= index < len(per_image):
            raise ValueError("result files: image_id %r is not in the dataset" % (image_id,))
        if labels_of is not None and e["category_id"] not in labels_of:
            raise ValueError("result files: category_id %r is not in the dataset" % (e["category_id"],))
        n = len(e.get("keypoints", ()))
        if n == 0 or n % 3 or (K is not None and n != 3 * K):
            raise ValueError("result files: %d keypoint numbers (image %r): expected the same multiple of 3 in every entry"
                             % (n, image_id))
        K = n // 3
        per_image[index].append(e)
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
        boxlist = BoxList(boxes, (W, H), mode="xyxy")
        boxlist.add_field("scores", torch.tensor([e["score"] for e in es], dtype=torch.float32))
        cats = [e["category_id"] for e in es]
        boxlist.add_field("labels", torch.tensor(cats if labels_of is None else [labels_of[c] for c in cats], dtype=torch.int64))
        boxlist.add_field("keypoints", PersonKeypoints(kp, (W, H)))
        out.append(boxlist.to(device))
    return out


def evaluate_keypoint_file(dataset, path_or_list, output_folder=None, batch=8, device="cpu", sigmas=None, expected_results=(),
                           expected_results_sigma_tol=4):
    """Score a saved `keypoints.json` (a path, or its list of entries) against `dataset`'s ground truth: one
    KeypointOKSEvaluator fed `batch` images at a time on `device` -> the COCOResults of finish_coco, which also logs the
    table and, with `output_folder`, writes coco_results.pth / coco_results.txt."""
    from . import _groundtruth, finish_coco

    device = torch.device(device)
    predictions = load_keypoint_results(path_or_list, dataset, device)
    evaluator = KeypointOKSEvaluator(getattr(dataset, "num_classes", None) or 2, sigmas)
    for i in range(0, len(predictions), batch):
        preds = predictions[i:i + batch]
        evaluator.update(preds, [_groundtruth(dataset, j).to(device) for j in range(i, i + len(preds))])
    if output_folder:
        os.makedirs(output_folder, exist_ok=True)
    return finish_coco(evaluator, output_folder, expected_results, expected_results_sigma_tol)
