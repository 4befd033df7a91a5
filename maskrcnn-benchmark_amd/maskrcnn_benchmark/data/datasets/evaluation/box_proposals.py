"""Proposal recall (`box_only`): the average recall of RPN proposals at 100 and 1000 proposals per image, over all ground
truths and over small, medium and large ones — the reference's evaluate_box_proposals
(data/datasets/evaluation/coco/coco_eval.py) as a streaming evaluator.

Per batch the proposals are put in objectness order and matched against the ground truth where the tensors live: for all
(limit, area range) pairs in one launch on the device (csrc/eval_proposals.hip through
maskrcnn_benchmark._C.eval_proposal_overlaps), or by the reference's loop in numpy for CPU tensors and images beyond the
kernel's caps (_eval_cpu.eval_proposal_overlaps).  Only the matched IoU of every ground truth is kept; recall and its
average are the reference's own torch expressions, evaluated once on the host.

The rules are stated in include/detops.h ("Proposal recall").  Unlike the COCO-style AP rules they are checked against the
original: the reference's function is plain torch, and tests/golden/box_proposals_reference.npz holds what it returned for
every limit and area range (tests/golden/make_golden_box_proposals.py).

Ground truth, as the test loader hands it out (`get_groundtruth`): crowds (`iscrowd` != 0) do not count; the area is the
`area` field, else the mask's pixel count, else the box area (coco_style.groundtruth_area), compared in fp32 with both ends
of the range inclusive.  The reference compares an fp32 tensor when the json areas are floats and an int64 tensor when they
are all integers; the two differ only for areas above 2^24.

`evaluate`, `coco_evaluation` and `check_scope` still refuse `box_only`, like `keypoints`: `inference(box_only=True)`,
BoxProposalEvaluator and evaluate_box_proposals are the way in.
"""
import logging
import os
from collections import OrderedDict

import torch

from maskrcnn_benchmark import _C

from . import coco_style
from .coco_style import _feed

# the reference's table: name -> [lo, hi] of the area, both inclusive
AREA_RANGES = OrderedDict([
    ("all", (0 ** 2, 1e5 ** 2)), ("small", (0 ** 2, 32 ** 2)), ("medium", (32 ** 2, 96 ** 2)), ("large", (96 ** 2, 1e5 ** 2)),
    ("96-128", (96 ** 2, 128 ** 2)), ("128-256", (128 ** 2, 256 ** 2)), ("256-512", (256 ** 2, 512 ** 2)),
    ("512-inf", (512 ** 2, 1e5 ** 2))])
AREA_SUFFIX = {"all": "", "small": "s", "medium": "m", "large": "l"}      # AR@100, ARs@100, ... (COCOResults.METRICS)
LIMITS = (100, 1000)


def default_thresholds():
    return torch.arange(0.5, 0.95 + 1e-5, 0.05, dtype=torch.float32)


class BoxProposalEvaluator(object):
    """evaluator = BoxProposalEvaluator(); evaluator.update(predictions, targets) per batch; evaluator.summarize() ->
    {(limit, area): {"ar", "recalls", "thresholds", "gt_overlaps", "num_pos"}}, the reference's dict per pair.

    limits: proposals per image that take part (None: all); areas: names of AREA_RANGES; thresholds: an fp32 tensor of IoU
    thresholds (default 0.5 : 0.05 : 0.95).
    update(predictions, targets): two lists of BoxList (one per image), on the device or the CPU.  Predictions carry
    `objectness`; one of another size than its target is resized to it (the reference resizes to the image's size), then
    they are sorted by objectness, descending and stable.  Targets may carry `iscrowd`, `area` and `masks`.
    An image without (valid) ground truth contributes nothing; one with valid ground truth and no proposals adds to num_pos
    only.  With num_pos == 0 the reference fails inside torch.cat; here `ar` is -1 and `recalls` is all -1 (this library's
    choice)."""

    def __init__(self, limits=LIMITS, areas=("all", "small", "medium", "large"), thresholds=None):
        self.limits, self.areas = tuple(limits), tuple(areas)
        for area in self.areas:
            assert area in AREA_RANGES, "Unknown area range: {}".format(area)
        if not self.limits or not self.areas:
            raise ValueError("BoxProposalEvaluator: at least one limit and one area range")
        self.thresholds = thresholds
        self.batches = []         # per batch (overlaps [L, A, G] on the batch's device, valid ground truths per range [A])
        self.num_images = self.num_detections = self.num_groundtruths = 0
        self.results = None

    # ------------------------------------------------------------------ per batch
    def update(self, predictions, targets):
        assert len(predictions) == len(targets), "one prediction per target"
        dev = targets[0].bbox.device if targets else torch.device("cpu")
        preds, tgts = [], []
        for pred, tgt in zip(predictions, targets):
            if len(pred) and not pred.has_field("objectness"):
                raise ValueError("proposal recall needs predictions with an `objectness` field: the model is not RPN-only")
            tgt = tgt.convert("xyxy")
            if tuple(pred.size) != tuple(tgt.size):
                pred = pred.resize(tgt.size)
            preds.append(pred.convert("xyxy").to(dev))
            tgts.append(tgt)
        n_dt, n_gt = [len(p) for p in preds], [len(t) for t in tgts]
        self.num_images += len(preds)
        self.num_detections += sum(n_dt)
        self.num_groundtruths += sum(n_gt)
        if sum(n_gt) == 0:
            return
        f32 = dict(dtype=torch.float32, device=dev)
        dt_box = torch.cat([p.bbox for p in preds]).reshape(-1, 4)
        gt_box = torch.cat([t.bbox for t in tgts]).reshape(-1, 4)
        score = torch.cat([p.get_field("objectness").reshape(-1).to(**f32) if len(p) else torch.zeros((0,), **f32) for p in preds])
        image = torch.arange(len(preds), device=dev).repeat_interleave(torch.tensor(n_dt, device=dev), output_size=sum(n_dt))
        by_score = torch.sort(score, descending=True, stable=True)[1]
        order = by_score[torch.sort(image[by_score], stable=True)[1]]          # objectness order inside every image
        offsets = lambda counts: torch.tensor([0] + counts, dtype=torch.int64).cumsum(0).to(torch.int32).to(dev)  # noqa: E731
        crowd = torch.cat([(t.get_field("iscrowd").to(dev) != 0) if t.has_field("iscrowd")
                           else torch.zeros((len(t),), dtype=torch.bool, device=dev) for t in tgts])
        gt_pack = None
        if coco_style.needs_mask_area(tgts):
            gt_pack = coco_style._pack_masks(coco_style.groundtruth_planes(tgts, dev))
        area = coco_style.groundtruth_area(tgts, gt_box, gt_pack).to(torch.float32)
        valid = torch.stack([(area >= AREA_RANGES[a][0]) & (area <= AREA_RANGES[a][1]) & ~crowd for a in self.areas])
        overlaps = _C.eval_proposal_overlaps(dt_box[order], gt_box, offsets(n_dt), offsets(n_gt), valid, self.limits,
                                             max_dt=max(n_dt), max_gt=max(n_gt))
        if any(g and not d for d, g in zip(n_dt, n_gt)):
            # an image without proposals counts in num_pos and adds nothing to the overlaps (the reference skips it there)
            bare = torch.tensor([not d for d, g in zip(n_dt, n_gt) for _ in range(g)]).to(dev)
            overlaps = torch.where(bare, torch.full_like(overlaps, -1), overlaps)
        self.batches.append((overlaps, valid.sum(dim=1)))

    # ------------------------------------------------------------------ once per evaluation
    def num_pos(self):
        """{area: the number of valid ground truths seen}"""
        total = torch.zeros((len(self.areas),), dtype=torch.int64)
        for _, count in self.batches:
            total += count.cpu()
        return OrderedDict(zip(self.areas, (int(v) for v in total)))

    def summarize(self):
        num_pos = self.num_pos()
        thresholds = default_thresholds() if self.thresholds is None else self.thresholds
        overlaps = [o.cpu() for o, _ in self.batches]
        self.results = OrderedDict()
        for li, limit in enumerate(self.limits):
            for ai, area in enumerate(self.areas):
                parts = [o[li, ai] for o in overlaps]
                gt_overlaps = torch.cat([p[p >= 0] for p in parts]) if parts else torch.zeros((0,), dtype=torch.float32)
                gt_overlaps, _ = torch.sort(gt_overlaps)
                recalls = torch.zeros_like(thresholds)
                if num_pos[area] == 0:
                    recalls = recalls - 1
                else:
                    for i, t in enumerate(thresholds):
                        recalls[i] = (gt_overlaps >= t).float().sum() / float(num_pos[area])
                ar = recalls.mean()
                self.results[(limit, area)] = {"ar": ar, "recalls": recalls, "thresholds": thresholds,
                                               "gt_overlaps": gt_overlaps, "num_pos": num_pos[area]}
        return self.results


def evaluate_box_proposals(predictions, dataset, thresholds=None, area="all", limit=None, batch=8):
    """The reference's function: predictions (one BoxList with `objectness` per image, in dataset order) against the
    dataset's ground truth -> {"ar", "recalls", "thresholds", "gt_overlaps" (sorted), "num_pos"}"""
    evaluator = _feed(BoxProposalEvaluator((limit,), (area,), thresholds), predictions, dataset, batch)
    return evaluator.summarize()[(limit, area)]


def finish_box_proposals(evaluator, output_folder=None, expected_results=(), expected_results_sigma_tol=4):
    """summarize, fill the `box_proposal` row (AR@100 ... ARl@1000), log it, check the expected results, save
    box_proposals.pth / box_proposals.txt -> COCOResults"""
    from . import COCOResults, check_expected_results

    logger = logging.getLogger("maskrcnn_benchmark.inference")
    logger.info("Evaluating bbox proposals")
    results = COCOResults("box_proposal")
    for (limit, area), stats in evaluator.summarize().items():
        key = "AR{}@{}".format(AREA_SUFFIX.get(area, "[%s]" % area), "all" if limit is None or limit <= 0 else "%d" % limit)
        results.results["box_proposal"][key] = stats["ar"].item()
    logger.info(results)
    check_expected_results(results, expected_results, expected_results_sigma_tol)
    if output_folder:
        os.makedirs(output_folder, exist_ok=True)
        torch.save(results, os.path.join(output_folder, "box_proposals.pth"))
        with open(os.path.join(output_folder, "box_proposals.txt"), "w") as f:
            f.write(repr(results))
    return results


def do_box_proposal_evaluation(dataset, predictions, output_folder=None, expected_results=(), expected_results_sigma_tol=4,
                               batch=8, device=None):
    """Score stored proposals (one BoxList with `objectness` per image, in dataset order) at the reference's limits and area
    ranges, `batch` images at a time on `device` (None: where the predictions live) -> the COCOResults of
    finish_box_proposals"""
    evaluator = _feed(BoxProposalEvaluator(), predictions, dataset, batch, device)
    return finish_box_proposals(evaluator, output_folder, expected_results, expected_results_sigma_tol)
