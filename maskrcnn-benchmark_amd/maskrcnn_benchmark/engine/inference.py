"""Inference and evaluation loop (reference engine/inference.py) as a streaming evaluation: per batch, loader ->
model(images.to(device)) -> targets to the device -> evaluator.update; the predictions are matched against the ground truth
where they were made and only the match records are kept (data/datasets/evaluation/coco_style.py).  With an output folder the
detections themselves are written as COCO result files (data/datasets/evaluation/coco_results.py: bbox.json, segm.json,
keypoints.json), batch by batch next to the evaluator; `evaluate=False` writes them and matches nothing.  Keypoints are
scored on request (`keypoint_oks=True`: data/datasets/evaluation/keypoint_oks.py).  The proposals of an RPN-only model
are scored by their average recall (`box_only=True`: data/datasets/evaluation/box_proposals.py).  A dataset whose
`evaluation_style` is "cityscapes" feeds the Cityscapes evaluator the same way (data/datasets/evaluation/cityscapes.py).
Single process only.
Datasets that are not COCO-shaped keep the reference's flow: the predictions are collected and handed to `evaluate`."""
import logging
import os
import time

import torch

from maskrcnn_benchmark.data.datasets.evaluation import (BoxProposalEvaluator, CityscapesEvaluator, COCOStyleEvaluator,
                                                         check_scope, dataset_style, finish_box_proposals, finish_cityscapes,
                                                         finish_coco)
from maskrcnn_benchmark.data.datasets.evaluation import evaluate as evaluate_predictions
from maskrcnn_benchmark.data.datasets.evaluation.coco_results import COCOResultsWriter
from maskrcnn_benchmark.data.datasets.evaluation.coco_style import _num_classes
from maskrcnn_benchmark.data.datasets.evaluation.keypoint_oks import KeypointOKSEvaluator
from maskrcnn_benchmark.utils.comm import get_world_size


def _built_with(model):
    """the config a detector was built from: the copy its ROI heads keep (a wrapper's `.module` is looked through); None
    for a model without ROI heads"""
    for _ in range(4):
        heads = getattr(model, "roi_heads", None)
        if heads is not None:
            return getattr(heads, "cfg", None)
        model = getattr(model, "module", None)
        if model is None:
            break
    return None


def inference(model, data_loader, dataset_name, iou_types=("bbox",), box_only=False, bbox_aug=None, device="cuda",
              expected_results=(), expected_results_sigma_tol=4, output_folder=None, cfg=None, evaluate=True,
              keypoint_oks=False):
    """bbox_aug: test-time box augmentation (engine/bbox_aug.py) with the passes of `cfg.TEST.BBOX_AUG`; model and loader
    were built from that `cfg` (the reference reads its global cfg there; left out, it is the copy the ROI heads keep).
    None, the default and what tools/test_net.py gets: as the model was built, i.e. TEST.BBOX_AUG.ENABLED of its config.
    An explicit value that contradicts the model is an error, not a choice: a model built with BBOX_AUG hands back unfiltered
    per-class boxes and one built without it hands back detections.  Under box augmentation only the bbox table is made,
    which is logged.
    evaluate=False (COCO-shaped datasets, `output_folder` required): results only.  The model runs and the result files of
    `iou_types` are written; no evaluator is built, the evaluator's scope is not checked ("keypoints" is allowed: OKS is not
    needed to write keypoints.json) and the targets are neither moved nor matched: the way to run a test set without
    annotations.  -> {iou type: path of its file}.
    keypoint_oks=True (COCO-shaped datasets, a model with a keypoint head, not under box augmentation): the loop also feeds a
    KeypointOKSEvaluator next to the evaluator of `iou_types`, the writer also writes keypoints.json, and the returned
    COCOResults has a `keypoints` row.  "keypoints" in `iou_types` is still refused: OKS has names of its own.
    box_only=True (an RPN-only model, MODEL.RPN_ONLY: its output is the proposals with their `objectness`): on a COCO-shaped
    dataset the loop feeds a BoxProposalEvaluator instead of the evaluator of `iou_types`, and the returned COCOResults has the
    one row `box_proposal` (AR@100 ... ARl@1000), saved as box_proposals.pth / box_proposals.txt; no result files are written
    for proposals.  Not together with keypoint_oks, evaluate=False or box augmentation.  ValueError: the model's output has
    no `objectness`, i.e. the model is not RPN-only.
    A dataset whose `evaluation_style` is "cityscapes" (data/datasets/cityscapes.py): the loop feeds a CityscapesEvaluator with
    the dataset's CLASSES and `iou_types` ("bbox", "segm"), and the result is its summarize(): {iou type: {"averages": the
    reference's avgDict, "ap": [1, classes, 10]}}; with an output folder evaluationResults/boxResult.json / maskResult.json
    are written, no COCO result files.  Refused for such a dataset: keypoint_oks, box_only, evaluate=False, and box
    augmentation together with "segm" (the mask head is not run under it)."""
    if not evaluate and not output_folder:
        raise ValueError("inference(evaluate=False) writes result files only: it needs output_folder=")
    if get_world_size() > 1:
        raise NotImplementedError("evaluation is single-process only: run tools/test_net.py without a distributed launcher "
                                  "(world size %d)" % get_world_size())
    logger = logging.getLogger("maskrcnn_benchmark.inference")
    requested_iou_types = tuple(iou_types)
    built_with = _built_with(model)
    built_aug = None if built_with is None else bool(built_with.TEST.BBOX_AUG.ENABLED)
    if bbox_aug is None:
        bbox_aug = bool(built_aug)
        if bbox_aug:
            logger.info("the model was built with TEST.BBOX_AUG.ENABLED: evaluating with test-time box augmentation")
    elif built_aug is not None and bool(bbox_aug) != built_aug:
        raise ValueError("inference(bbox_aug=%s), but the model was built with TEST.BBOX_AUG.ENABLED %s: the box head's output "
                         "(unfiltered per-class boxes or detections) is fixed when the model is built" % (bool(bbox_aug), built_aug))
    if bbox_aug:
        from .bbox_aug import im_detect_bbox_aug

        cfg = built_with if cfg is None else cfg
        if cfg is None:
            raise ValueError("inference(bbox_aug=True) needs cfg=: the config the model and the loader were built from")
        if tuple(iou_types) != ("bbox",):
            logger.info("TEST.BBOX_AUG: the mask and keypoint heads are not run under box augmentation; evaluating bbox only "
                        "(not %s)", ", ".join(t for t in iou_types if t != "bbox"))
            iou_types = ("bbox",)
    device = torch.device(device)
    dataset = data_loader.dataset
    logger.info("Start evaluation on {} dataset({} images).".format(dataset_name, len(dataset)))
    cityscapes = dataset_style(dataset) == "cityscapes"
    streaming = dataset_style(dataset) == "coco" or cityscapes
    evaluators, writer = [], None
    if cityscapes:
        if keypoint_oks or box_only or not evaluate:
            raise NotImplementedError("inference() on a Cityscapes dataset scores bbox and segm AP only: not keypoint_oks, "
                                      "box_only or evaluate=False")
        if bbox_aug and "segm" in requested_iou_types:
            raise NotImplementedError("inference() on a Cityscapes dataset: segm is not scored under box augmentation (the "
                                      "mask head is not run); ask for iou_types=('bbox',)")
    if keypoint_oks and (not streaming or box_only or bbox_aug):
        raise NotImplementedError("inference(keypoint_oks=True): keypoints are scored for COCO-shaped datasets and detections "
                                  "only (not box_only proposals, not under box augmentation)")
    if not evaluate and (not streaming or box_only):
        raise NotImplementedError("inference(evaluate=False): result files are written for COCO-shaped datasets and detections "
                                  "only (not box_only proposals)")
    if box_only and bbox_aug:
        raise NotImplementedError("inference(box_only=True): proposals are not scored under box augmentation")
    if cityscapes:
        evaluators = [CityscapesEvaluator(dataset.CLASSES, iou_types)]
    elif streaming and evaluate and box_only:
        evaluators = [BoxProposalEvaluator()]
    elif streaming and evaluate:
        check_scope(False, iou_types)
        evaluators = [COCOStyleEvaluator(iou_types, _num_classes(dataset, 81))]
        if keypoint_oks:
            evaluators.append(KeypointOKSEvaluator(_num_classes(dataset, 2)))
    if streaming and output_folder and not box_only and not cityscapes:
        writer = COCOResultsWriter(dataset, tuple(iou_types) + (("keypoints",) if keypoint_oks and "keypoints" not in iou_types else ()))
    model.eval()
    predictions = {}
    start = time.time()
    model_time = 0.0
    for images, targets, image_ids in data_loader:
        with torch.no_grad():
            t0 = time.time()
            output = im_detect_bbox_aug(model, images, device, cfg) if bbox_aug else model(images.to(device))
            if not bbox_aug and not box_only and any(o.has_field("scores") and not o.has_field("labels") for o in output):
                # a model whose config could not be found (a wrapper without `.module`) and that was built with BBOX_AUG
                raise ValueError("the model returned boxes without `labels`: it was built with TEST.BBOX_AUG.ENABLED and is "
                                 "evaluated with inference(bbox_aug=True, cfg=...)")
            if box_only and any(len(o) and not o.has_field("objectness") for o in output):
                raise ValueError("inference(box_only=True): the model returned boxes without `objectness`: it is not RPN-only "
                                 "(MODEL.RPN_ONLY); detections are evaluated with box_only=False")
            if device.type != "cpu":
                torch.cuda.synchronize()
            model_time += time.time() - t0
            if writer is not None:
                writer.update(output, image_ids)
            if evaluators:
                targets = [t.to(device) for t in targets]
                for evaluator in evaluators:
                    evaluator.update(output, targets)
            elif not streaming:
                predictions.update({i: o.to("cpu") for i, o in zip(image_ids, output)})
    total = time.time() - start
    n = max(len(dataset), 1)
    logger.info("Total run time: {:.1f} s ({:.4f} s / img, matching and result files included)".format(total, total / n))
    logger.info("Model inference time: {:.1f} s ({:.4f} s / img)".format(model_time, model_time / n))
    if output_folder:
        os.makedirs(output_folder, exist_ok=True)
    paths = {}
    if writer is not None:
        paths = writer.save(output_folder)
        for t, path in paths.items():
            logger.info("Wrote {} {} results of {} images to {}".format(len(writer.results[t]), t, writer.num_images, path))
    if not evaluate:
        return paths
    if streaming:
        logger.info("Matched {} detections against {} ground truths of {} images".format(
            evaluators[0].num_detections, evaluators[0].num_groundtruths, evaluators[0].num_images))
        if cityscapes:
            return finish_cityscapes(evaluators[0], output_folder, expected_results, expected_results_sigma_tol)
        if box_only:
            return finish_box_proposals(evaluators[0], output_folder, expected_results, expected_results_sigma_tol)
        return finish_coco(evaluators, output_folder, expected_results, expected_results_sigma_tol)
    predictions = [predictions[i] for i in sorted(predictions)]
    if output_folder:
        torch.save(predictions, os.path.join(output_folder, "predictions.pth"))
    return evaluate_predictions(dataset=dataset, predictions=predictions, output_folder=output_folder, box_only=box_only,
                                iou_types=iou_types, expected_results=expected_results,
                                expected_results_sigma_tol=expected_results_sigma_tol)
