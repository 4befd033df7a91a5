"""Cityscapes instance-level AP (reference data/datasets/evaluation/cityscapes/{cityscapes_eval,eval_instances}.py) as a
streaming evaluator.

Per batch the predictions are brought to the original image size, their masks pasted and the ground-truth planes made where
the tensors live, and ALL the pixel counts of an image come from one call (`_C.window_counts`: csrc/cityscapes_eval.hip on
the device, _eval_cpu.window_counts for CPU tensors) where the reference crops, multiplies, sums and calls `.item()` once
per instance and per pair.  Only records are kept: per instance (image, label, boxArea, pixelCount, score), per recorded
pair the two intersections.  The AP is the reference's loops (evaluateBoxMatches / evaluateMaskMatches / computeAverages),
restated once for both kinds and evaluated on the host in fp64; tests/golden/cityscapes_reference.npz holds what the
reference's own functions returned.

The definitions (include/detops.h, "Cityscapes evaluation"; README.md, "Cityscapes"):
  boxes are `bbox.long()` of the xyxy boxes at the original image size; boxArea = (xmax - xmin) * (ymax - ymin); pixelCount
  is the plane's sum over rows ymin:ymax and columns xmin:xmax, THE MAXIMA EXCLUSIVE; a prediction with masks and
  pixelCount 0 is dropped; a pair takes part iff isOverlapping (strict on all four sides), maskIntersection is counted
  inside the UNION box; pairs are formed ACROSS classes and both sides are grouped by their own label afterwards.
This library's choices, where the reference slips or leaves a case open:
  1. a prediction keeps its own mask after others were dropped (the reference's zip pairs instance k with mask k);
  2. windows are clamped to the image (the reference lets a negative minimum wrap around as a Python index);
  3. the ground truth is the dataset's original-size target (`get_groundtruth`), not the transformed target resized back.
Without a `mask` field in the predictions, or without "segm" in `iou_types`, no plane is made and the pixel counts are 0.
An (overlap, class) whose curve has no entry at all, every prediction being ignored, gets AP 0 (the reference indexes an
empty array there).

`matches.json` is not written and the per-pair dicts are not kept; `boxResult.json` / `maskResult.json` are.
`evaluate` still refuses the "cityscapes" style: `inference()`, CityscapesEvaluator and do_cityscapes_evaluation are the
way in.
"""
import json
import logging
import os
from collections import OrderedDict

import numpy as np
import torch

from maskrcnn_benchmark import _C

from . import coco_style
from .coco_style import _feed

OVERLAPS = np.arange(0.5, 1.0, 0.05)          # the reference's very fp64 values: 0.6000000000000001, 0.7500000000000002, ...
MIN_REGION_SIZES = np.array([100])


def _prediction_planes(pred):
    """the `mask` field of one image's predictions -> [n, H, W] bool / uint8 planes on the predictions' device: dense
    planes [n, 1, H, W] as they are, probabilities [n, 1, M, M] pasted with Masker(threshold=0.5)"""
    from maskrcnn_benchmark.modeling.roi_heads.mask_head.inference import Masker

    W, H = pred.size
    masks = pred.get_field("mask").to(pred.bbox.device)
    if masks.dim() != 4 or masks.shape[1] != 1 or masks.shape[0] != len(pred):
        raise ValueError("prediction masks must be [n, 1, H, W] planes or [n, 1, M, M] probabilities, got %s" % (tuple(masks.shape),))
    if masks.dtype in (torch.bool, torch.uint8):
        if tuple(masks.shape[-2:]) != (H, W):
            raise ValueError("dense prediction masks of size %s for an image of %s" % (tuple(masks.shape[-2:]), (H, W)))
        return masks[:, 0]
    return Masker(threshold=0.5).forward_single_image(masks.float(), pred)[:, 0]


def host_pair_box(dt_box, gt_box):
    """boxIntersection of every pair that isOverlapping, 0 elsewhere: int64 numpy [D, G] from int boxes [D, 4], [G, 4]"""
    dt_box, gt_box = np.asarray(dt_box, np.int64).reshape(-1, 4), np.asarray(gt_box, np.int64).reshape(-1, 4)
    lo = np.maximum(dt_box[:, None, :2], gt_box[None, :, :2])
    hi = np.minimum(dt_box[:, None, 2:], gt_box[None, :, 2:])
    overlapping = ((dt_box[:, None, :2] < gt_box[None, :, 2:]) & (gt_box[None, :, :2] < dt_box[:, None, 2:])).all(axis=2)
    return np.where(overlapping, (hi - lo).prod(axis=2), 0)


class CityscapesEvaluator(object):
    """evaluator = CityscapesEvaluator(dataset.CLASSES, ("bbox", "segm")); evaluator.update(predictions, targets) per
    batch; evaluator.summarize() -> {"bbox": {"averages": the reference's avgDict, "ap": [1, classes, 10]}, "segm": ...}.

    classes: the label names, "__background__" first (the reference's args.instLabels; the background's row is nan).
    update(predictions, targets): two lists of BoxList (one per image) on the device or the CPU.  Predictions carry
    `labels`, `scores` and, for segm, `mask` ([n, 1, M, M] probabilities or [n, 1, H, W] bool / uint8 planes); one of another
    size than its target is resized to it.  Targets are the original-size ground truth with `labels` and `masks` (either
    SegmentationMask mode; polygons are rasterised where the target lives)."""

    def __init__(self, classes, iou_types=("bbox", "segm")):
        self.classes = list(classes)
        assert self.classes and self.classes[0] == "__background__", "the class names start with __background__"
        self.iou_types = tuple(iou_types)
        for t in self.iou_types:
            if t not in ("bbox", "segm"):
                raise ValueError("the Cityscapes evaluation serves the IoU types bbox and segm, not %r" % (t,))
        self.overlaps, self.min_region_sizes = OVERLAPS, MIN_REGION_SIZES
        self.images = []           # per image: the records (numpy) of its ground truths, predictions and recorded pairs
        self.num_images = self.num_detections = self.num_groundtruths = 0
        self.results = None

    # ------------------------------------------------------------------ per batch
    def update(self, predictions, targets):
        assert len(predictions) == len(targets), "one prediction per target"
        for pred, tgt in zip(predictions, targets):
            self._update_image(pred, tgt)

    def _update_image(self, pred, tgt):
        dev = tgt.bbox.device
        tgt = tgt.convert("xyxy")
        if tuple(pred.size) != tuple(tgt.size):
            pred = pred.resize(tgt.size)
        pred = pred.convert("xyxy").to(dev)
        W, H = tgt.size
        D, G = len(pred), len(tgt)
        dt_box = pred.bbox.reshape(-1, 4).long().to(torch.int32)             # truncation, as bbox.long()
        gt_box = tgt.bbox.reshape(-1, 4).long().to(torch.int32)
        labels = lambda b: b.get_field("labels").reshape(-1).cpu().numpy().astype(np.int64) if len(b) else np.zeros((0,), np.int64)  # noqa: E731
        dt_label, gt_label = labels(pred), labels(tgt)
        for name, lab in (("prediction", dt_label), ("target", gt_label)):
            if lab.size and (lab.min() < 0 or lab.max() >= len(self.classes)):
                raise ValueError("%s labels must lie in [0, %d), got %d .. %d" % (name, len(self.classes), lab.min(), lab.max()))
        score = pred.get_field("scores").reshape(-1).cpu().numpy().astype(np.float64) if D else np.zeros((0,), np.float64)
        with_masks = "segm" in self.iou_types and D > 0 and pred.has_field("mask")
        if with_masks:
            dt_planes = _prediction_planes(pred)
            gt_planes = coco_style._planes_of_target(tgt).to(dev) if G and tgt.has_field("masks") else torch.zeros((G, H, W), dtype=torch.uint8, device=dev)
            counts = _C.window_counts(dt_planes, dt_box, gt_planes, gt_box)
            dt_count, gt_count, pair_box, pair_mask = (c.cpu().numpy().astype(np.int64) for c in counts)
        else:
            dt_count, gt_count = np.zeros((D,), np.int64), np.zeros((G,), np.int64)
            if G and "segm" in self.iou_types and tgt.has_field("masks"):
                # the ground truths' own counts (an image without predictions still has its ground truth filtered by size)
                none = torch.zeros((0, H, W), dtype=torch.uint8, device=dev)
                gt_count = _C.window_counts(none, dt_box[:0], coco_style._planes_of_target(tgt).to(dev), gt_box)[1].cpu().numpy().astype(np.int64)
            pair_box = host_pair_box(dt_box.cpu().numpy(), gt_box.cpu().numpy())
            pair_mask = np.zeros_like(pair_box)
        dt_box_h, gt_box_h = dt_box.cpu().numpy().astype(np.int64), gt_box.cpu().numpy().astype(np.int64)
        area = lambda b: (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])  # noqa: E731
        keep = dt_count > 0 if with_masks else np.ones((D,), bool)          # a prediction without pixels is dropped
        d, g = np.nonzero((pair_box > 0) & keep[:, None])
        self.images.append({
            "gt_label": gt_label, "gt_box_area": area(gt_box_h), "gt_pixel_count": gt_count,
            "dt_index": np.nonzero(keep)[0], "dt_label": dt_label[keep], "dt_box_area": area(dt_box_h)[keep],
            "dt_pixel_count": dt_count[keep], "dt_score": score[keep],
            # recorded pairs in the reference's order (ground truth outer, prediction inner): prediction, ground truth, the two
            "pairs": np.stack([d, g, pair_box[d, g], pair_mask[d, g]], axis=1)[np.lexsort((d, g))].reshape(-1, 4)})
        self.num_images += 1
        self.num_detections += D
        self.num_groundtruths += G

    # ------------------------------------------------------------------ once per evaluation
    def matches(self):
        """the records as the reference's `matches`: per image {"groundTruth": {name: [gt]}, "prediction": {name: [pred]}},
        every gt with "matchedPred" and every pred with "matchedGt" (copies that carry the pair's two intersections)"""
        out = []
        for i, im in enumerate(self.images):
            gts = [{"labelID": int(l), "instID": k, "boxArea": int(a), "pixelCount": int(c), "matchedPred": []}
                   for k, (l, a, c) in enumerate(zip(im["gt_label"], im["gt_box_area"], im["gt_pixel_count"]))]
            preds = [{"imgName": i, "predID": int(k), "labelID": int(l), "boxArea": int(a), "pixelCount": int(c), "confidence": float(s),
                      "matchedGt": []}
                     for k, l, a, c, s in zip(im["dt_index"], im["dt_label"], im["dt_box_area"], im["dt_pixel_count"], im["dt_score"])]
            by_id = {p["predID"]: p for p in preds}
            for d, g, box, mask in im["pairs"]:
                gt, pred = gts[int(g)], by_id[int(d)]
                both = {"boxIntersection": int(box), "maskIntersection": int(mask)}
                gt["matchedPred"].append(dict({k: v for k, v in pred.items() if k != "matchedGt"}, **both))
                pred["matchedGt"].append(dict({k: v for k, v in gt.items() if k != "matchedPred"}, **both))
            out.append({"groundTruth": {name: [x for x in gts if self.classes[x["labelID"]] == name] for name in self.classes},
                        "prediction": {name: [x for x in preds if self.classes[x["labelID"]] == name] for name in self.classes}})
        return out

    def summarize(self):
        matches = self.matches()
        self.results = OrderedDict()
        for iou_type in self.iou_types:
            size, inter = ("boxArea", "boxIntersection") if iou_type == "bbox" else ("pixelCount", "maskIntersection")
            ap = evaluate_matches(matches, self.classes, size, inter, self.overlaps, self.min_region_sizes)
            self.results[iou_type] = {"averages": compute_averages(ap, self.classes, self.overlaps, self.min_region_sizes), "ap": ap}
        return self.results


def average_precision(y_true, y_score, hard_fns):
    """the reference's curve: scores ascending, the thresholds np.unique finds, the cumulative sum read at the FIRST index of
    every tie group (so the order inside a tie changes nothing), the artificial point (recall 0, precision 1) appended, and
    precision dotted with the step widths np.convolve(recall', [-0.5, 0, 0.5], "valid") makes"""
    y_true, y_score = np.asarray(y_true, np.float64), np.asarray(y_score, np.float64)
    order = np.argsort(y_score)
    score_sorted, true_sorted = y_score[order], y_true[order]
    cumsum = np.cumsum(true_sorted)
    _, first = np.unique(score_sorted, return_index=True)
    n, n_true = len(score_sorted), (cumsum[-1] if len(cumsum) else 0.0)
    cumsum = np.append(cumsum, 0)                       # index -1 reads this zero
    precision, recall = np.zeros(len(first) + 1), np.zeros(len(first) + 1)
    for k, idx in enumerate(first):
        below = cumsum[idx - 1]
        tp = n_true - below
        fp = n - idx - tp
        fn = below + hard_fns
        precision[k] = float(tp) / (tp + fp)
        recall[k] = float(tp) / (tp + fn)
    precision[-1], recall[-1] = 1.0, 0.0
    padded = np.append(np.append(recall[0], recall), 0.0)
    return np.dot(precision, np.convolve(padded, [-0.5, 0, 0.5], "valid"))


def evaluate_matches(matches, classes, size, inter, overlaps=OVERLAPS, min_region_sizes=MIN_REGION_SIZES):
    """evaluateBoxMatches (size "boxArea", inter "boxIntersection") and evaluateMaskMatches ("pixelCount",
    "maskIntersection") of the reference in one: -> ap [region sizes, classes, overlaps] fp64, nan for a class without
    ground truth, 0 for one with ground truth and no prediction.  Neither side's label is looked at when a match list is
    walked: a prediction of another class matches a ground truth."""
    ap = np.zeros((len(min_region_sizes), len(classes), len(overlaps)), np.float64)

    def iou(a, b, both):
        union = a[size] + b[size] - both[inter]
        return float(both[inter]) / union if union else 0.0          # 0 / 0 (no masks at all): the reference divides by zero

    for di, min_region in enumerate(min_region_sizes):
        for oi, threshold in enumerate(overlaps):
            for li, name in enumerate(classes):
                y_true, y_score, hard_fns, have_gt, have_pred = [], [], 0, False, False
                for img in matches:
                    preds = img["prediction"][name]
                    gts = [gt for gt in img["groundTruth"][name] if gt[size] >= min_region]
                    have_gt, have_pred = have_gt or bool(gts), have_pred or bool(preds)
                    true, scores = [], []
                    for gt in gts:
                        best = None                       # the highest score matched so far; every other match is a false positive
                        for pred in gt["matchedPred"]:
                            if iou(gt, pred, pred) > threshold:
                                if best is None:
                                    best = pred["confidence"]
                                else:
                                    true.append(0)
                                    scores.append(min(best, pred["confidence"]))
                                    best = max(best, pred["confidence"])
                        if best is None:
                            hard_fns += 1
                        else:
                            true.append(1)
                            scores.append(best)
                    for pred in preds:
                        if any(iou(gt, pred, gt) > threshold for gt in pred["matchedGt"]):
                            continue
                        ignored = sum(gt[inter] for gt in pred["matchedGt"] if gt[size] < min_region)      # small ground truths only
                        proportion = float(ignored) / pred[size] if pred[size] > 0 else 0
                        if proportion <= threshold:
                            true.append(0)
                            scores.append(pred["confidence"])
                    y_true += true
                    y_score += scores
                if have_gt and have_pred:
                    ap[di, li, oi] = average_precision(y_true, y_score, hard_fns)
                else:
                    ap[di, li, oi] = 0.0 if have_gt else float("nan")
    return ap


def compute_averages(ap, classes, overlaps=OVERLAPS, min_region_sizes=MIN_REGION_SIZES):
    """computeAverages: np.nanmean over the classes (the background's row is always nan), the 50% / 75% columns found with
    np.isclose -> the reference's avgDict"""
    import warnings

    d = int(np.argmin(min_region_sizes))
    o50, o75 = np.where(np.isclose(overlaps, 0.5))[0], np.where(np.isclose(overlaps, 0.75))[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)          # "Mean of empty slice": no class has ground truth
        avg = {"allAp": np.nanmean(ap[d]), "allAp50%": np.nanmean(ap[d][:, o50]), "allAp75%": np.nanmean(ap[d][:, o75]), "classes": {}}
    for li, name in enumerate(classes):
        avg["classes"][name] = {"ap": np.average(ap[d, li, :]), "ap50%": np.average(ap[d, li, o50]), "ap75%": np.average(ap[d, li, o75])}
    return avg


def format_results(avg, classes):
    """the reference's printResults with colorized = False and csv = False"""
    row = lambda what, a, b, c: "{:<15}".format(what) + ":" + "".join("{:>15.3f}".format(v) for v in (a, b, c))  # noqa: E731
    lines = ["", "#" * 65, "{:<15}".format("what") + ":" + "".join("{:>15}".format(h) for h in ("AP", "AP_50%", "AP_75%")), "#" * 65]
    lines += [row(name, avg["classes"][name]["ap"], avg["classes"][name]["ap50%"], avg["classes"][name]["ap75%"]) for name in classes]
    lines += ["-" * 65, row("average", avg["allAp"], avg["allAp50%"], avg["allAp75%"]), ""]
    return "\n".join(lines) + "\n"


def _jsonable(v):
    if isinstance(v, dict):
        return {k: _jsonable(x) for k, x in v.items()}
    return float(v)


def finish_cityscapes(evaluator, output_folder=None, expected_results=(), expected_results_sigma_tol=4):
    """summarize, log the reference's table (without its colour codes), and with an output folder write
    evaluationResults/boxResult.json / maskResult.json in the layout of prepareJSONDataForResults (nan is written as NaN,
    as json.dump does) -> summarize()'s dict.  matches.json is not written."""
    logger = logging.getLogger("maskrcnn_benchmark.inference")
    results = evaluator.summarize()
    text = ""
    for iou_type, title, fname in (("bbox", "BBox", "boxResult.json"), ("segm", "Mask", "maskResult.json")):
        if iou_type not in results:
            continue
        res = results[iou_type]
        text += "\n%s\n" % title + format_results(res["averages"], evaluator.classes)
        if output_folder:
            folder = os.path.join(output_folder, "evaluationResults")
            os.makedirs(folder, exist_ok=True)
            with open(os.path.join(folder, fname), "w") as f:
                json.dump({"averages": _jsonable(res["averages"]), "overlaps": evaluator.overlaps.tolist(),
                           "minRegionSizes": evaluator.min_region_sizes.tolist(), "instLabels": list(evaluator.classes),
                           "resultApMatrix": res["ap"].tolist()}, f, indent=4)
    logger.info(text)
    if expected_results:
        logger.warning("expected results are not checked for the Cityscapes evaluation (the reference does not either)")
    return results


def do_cityscapes_evaluation(dataset, predictions, box_only=False, output_folder=None, iou_types=("bbox", "segm"),
                             expected_results=(), expected_results_sigma_tol=4, batch=8, device=None):
    """The reference's entry for stored predictions (one BoxList per image, in dataset order), `batch` images at a time on
    `device` (None: where the predictions live) -> {"bbox": ..., "segm": ...} of finish_cityscapes"""
    if box_only:
        raise NotImplementedError("box_only is not part of the Cityscapes evaluation (the reference ignores the flag)")
    logger = logging.getLogger("maskrcnn_benchmark.inference")
    logger.info("CityScapes evaluation on [%s]:" % (dataset,))
    evaluator = _feed(CityscapesEvaluator(dataset.CLASSES, iou_types), predictions, dataset, batch, device)
    return finish_cityscapes(evaluator, output_folder, expected_results, expected_results_sigma_tol)
