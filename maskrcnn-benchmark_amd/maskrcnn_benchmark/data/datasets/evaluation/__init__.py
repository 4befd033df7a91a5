"""Detection evaluation (reference data/datasets/evaluation/): `evaluate` dispatches on the dataset as the reference's
does; COCO-shaped datasets go to the streaming COCO-style evaluator (coco_style.py), VOC-shaped ones to voc.py.

Keypoints are scored under names of their own (keypoint_oks.py: KeypointOKSEvaluator, load_keypoint_results,
evaluate_keypoint_file; `inference(keypoint_oks=True)`; tools/evaluate_keypoints.py).  `evaluate`, `check_scope` and
COCOStyleEvaluator still refuse the `keypoints` IoU type: routing the generic names to OKS is a later change.

The average recall of RPN proposals (`box_only`) has names of its own too (box_proposals.py: BoxProposalEvaluator,
evaluate_box_proposals, do_box_proposal_evaluation; `inference(box_only=True)`); `evaluate`, `coco_evaluation` and
`check_scope` still refuse `box_only`.

The Cityscapes instance-level AP has names of its own as well (cityscapes.py: CityscapesEvaluator, do_cityscapes_evaluation,
finish_cityscapes; `inference()` routes a dataset whose `evaluation_style` is "cityscapes" there); `evaluate` still refuses
that style.

Not built, and raising NotImplementedError: `box_only`, the `keypoints` IoU type and the "cityscapes" style through the
generic entry points.
"""
import logging
import os
from collections import OrderedDict

import torch

from .box_proposals import (BoxProposalEvaluator, do_box_proposal_evaluation, evaluate_box_proposals,  # noqa: F401
                            finish_box_proposals)
from .cityscapes import CityscapesEvaluator, do_cityscapes_evaluation, finish_cityscapes  # noqa: F401
from .coco_style import STAT_NAMES, STAT_ROWS, COCOStyleEvaluator, _feed, _num_classes  # noqa: F401
from .keypoint_oks import KeypointOKSEvaluator, evaluate_keypoint_file, load_keypoint_results  # noqa: F401
from .voc import do_voc_evaluation, eval_detection_voc  # noqa: F401


def dataset_style(dataset):
    """"coco" | "voc" | "cityscapes" | None: the dataset's `evaluation_style` attribute; the synthetic COCO-shaped dataset is "coco" """
    from maskrcnn_benchmark.data.synthetic import SyntheticCOCODataset

    style = getattr(dataset, "evaluation_style", None)
    if style is None and isinstance(dataset, SyntheticCOCODataset):
        style = "coco"
    return style


def evaluate(dataset, predictions, output_folder, **kwargs):
    """dataset: the dataset the predictions (a list of BoxList, one per image, in dataset order) were made on;
    output_folder: where result files go (None: nowhere) -> the evaluation's result"""
    args = dict(dataset=dataset, predictions=predictions, output_folder=output_folder, **kwargs)
    style = dataset_style(dataset)
    if style == "coco":
        return coco_evaluation(**args)
    if style == "voc":
        return voc_evaluation(**args)
    if style == "cityscapes":
        raise NotImplementedError("the Cityscapes evaluation is not served by the generic entry points: it runs through "
                                  "inference(), CityscapesEvaluator and do_cityscapes_evaluation")
    raise NotImplementedError("Unsupported dataset type {}.".format(dataset.__class__.__name__))


def check_scope(box_only, iou_types):
    if box_only:
        raise NotImplementedError("box_only (the AR of RPN proposals) is not served by the generic entry points: it runs "
                                  "through inference(box_only=True), BoxProposalEvaluator and evaluate_box_proposals")
    if "keypoints" in iou_types:
        raise NotImplementedError("the keypoints IoU type is not served by the generic entry points: OKS runs through "
                                  "inference(keypoint_oks=True), KeypointOKSEvaluator and tools/evaluate_keypoints.py")


def coco_evaluation(dataset, predictions, output_folder, box_only=False, iou_types=("bbox",), expected_results=(),
                    expected_results_sigma_tol=4, batch=8):
    check_scope(box_only, iou_types)
    evaluator = _feed(COCOStyleEvaluator(iou_types, _num_classes(dataset, 81)), predictions, dataset, batch)
    return finish_coco(evaluator, output_folder, expected_results, expected_results_sigma_tol)


def finish_coco(evaluator, output_folder=None, expected_results=(), expected_results_sigma_tol=4):
    """summarize, log the table, check the expected results, save coco_results.pth -> COCOResults.  evaluator: a
    COCOStyleEvaluator, a KeypointOKSEvaluator, or a sequence of them (their tables in that order)"""
    logger = logging.getLogger("maskrcnn_benchmark.inference")
    evaluators = list(evaluator) if isinstance(evaluator, (list, tuple)) else [evaluator]
    stats = OrderedDict()
    for e in evaluators:
        stats.update(e.summarize())
    results = COCOResults(*stats)
    for e in evaluators:
        results.update(e)
    logger.info(results)
    logger.info(format_stats(stats))
    check_expected_results(results, expected_results, expected_results_sigma_tol)
    if output_folder:
        torch.save(results, os.path.join(output_folder, "coco_results.pth"))
        with open(os.path.join(output_folder, "coco_results.txt"), "w") as f:
            f.write(repr(results) + format_stats(stats))
    return results


def format_stats(stats):
    """{iou type: its statistics, in the order of coco_style.STAT_ROWS (12 numbers; keypoints: 10)} -> the table as text"""
    text = "\n"
    for iou_type, s in stats.items():
        text += "%s\n" % iou_type
        text += "".join("  %-6s %8.4f\n" % (row[0], v) for row, v in zip(STAT_ROWS[iou_type], s))
    return text


def voc_evaluation(dataset, predictions, output_folder, box_only=False, **_):
    logger = logging.getLogger("maskrcnn_benchmark.inference")
    if box_only:
        logger.warning("voc evaluation doesn't support box_only, ignored.")
    logger.info("performing voc evaluation, ignored iou_types.")
    return do_voc_evaluation(dataset=dataset, predictions=predictions, output_folder=output_folder, logger=logger)


_AP_NAMES = ("AP", "AP50", "AP75", "APs", "APm", "APl")


class COCOResults(object):
    """The headline numbers per task, under the reference's names (its COCOResults): `results[task][metric]`, -1 until
    filled; printed as a 'Task:' line, the metric names and the values to four decimals."""

    METRICS = {
        "bbox": list(_AP_NAMES),
        "segm": list(_AP_NAMES),
        "box_proposal": ["AR%s@%d" % (size, limit) for limit in (100, 1000) for size in ("", "s", "m", "l")],
        "keypoints": [name for name in _AP_NAMES if name != "APs"],
    }

    def __init__(self, *iou_types):
        unknown = [t for t in iou_types if t not in self.METRICS]
        assert not unknown, unknown
        self.results = OrderedDict()
        for task in iou_types:
            self.results[task] = OrderedDict.fromkeys(self.METRICS[task], -1)

    def update(self, evaluator):
        """evaluator: a summarized COCOStyleEvaluator or KeypointOKSEvaluator (the reference takes a pycocotools COCOeval),
        or None.  The keypoints row takes the first five of the ten keypoint statistics: AP, AP50, AP75, APm, APl."""
        if evaluator is None:
            return
        assert isinstance(evaluator, COCOStyleEvaluator)
        for task, stats in evaluator.stats.items():
            self.results[task].update(zip(self.METRICS[task], (float(v) for v in stats)))

    def __repr__(self):
        lines = [""]
        for task, metrics in self.results.items():
            lines += ["Task: %s" % task, ", ".join(metrics), ", ".join("%.4f" % v for v in metrics.values())]
        return "\n".join(lines) + "\n"


def check_expected_results(results, expected_results, sigma_tol):
    """expected_results: [(task, metric, (mean, std))].  A value strictly inside mean -+ sigma_tol * std is logged as PASS
    (info), any other as FAIL (error), in the reference's wording; nothing is raised."""
    logger = logging.getLogger("maskrcnn_benchmark.inference")
    for task, metric, (mean, std) in expected_results or ():
        value = results.results[task][metric]
        half = sigma_tol * std
        inside = mean - half < value < mean + half
        text = "%s > %s sanity check (actual vs. expected): %.3f vs. mean=%.4f, std=%s, range=(%.4f, %.4f)" % (
            task, metric, value, mean, "{:.4}".format(std), mean - half, mean + half)
        logger.log(logging.INFO if inside else logging.ERROR, ("PASS: " if inside else "FAIL: ") + text)
