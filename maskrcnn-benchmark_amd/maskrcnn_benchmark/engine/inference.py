"""Inference and evaluation loop (reference engine/inference.py) as a streaming evaluation: per batch, loader ->
model(images.to(device)) -> targets to the device -> evaluator.update; the predictions are matched against the ground truth
where they were made and only the match records are kept (data/datasets/evaluation/coco_style.py).  Single process only.
Datasets that are not COCO-shaped keep the reference's flow: the predictions are collected and handed to `evaluate`."""
import logging
import os
import time

import torch

from maskrcnn_benchmark.data.datasets.evaluation import COCOStyleEvaluator, check_scope, dataset_style, evaluate, finish_coco
from maskrcnn_benchmark.utils.comm import get_world_size


def inference(model, data_loader, dataset_name, iou_types=("bbox",), box_only=False, bbox_aug=False, device="cuda",
              expected_results=(), expected_results_sigma_tol=4, output_folder=None):
    if get_world_size() > 1:
        raise NotImplementedError("evaluation is single-process only: run tools/test_net.py without a distributed launcher "
                                  "(world size %d)" % get_world_size())
    if bbox_aug:
        raise NotImplementedError("test-time box augmentation (bbox_aug) is not built")
    device = torch.device(device)
    logger = logging.getLogger("maskrcnn_benchmark.inference")
    dataset = data_loader.dataset
    logger.info("Start evaluation on {} dataset({} images).".format(dataset_name, len(dataset)))
    streaming = dataset_style(dataset) == "coco"
    evaluator = None
    if streaming:
        check_scope(box_only, iou_types)
        evaluator = COCOStyleEvaluator(iou_types, getattr(dataset, "num_classes", None) or 81)
    model.eval()
    predictions = {}
    start = time.time()
    model_time = 0.0
    for images, targets, image_ids in data_loader:
        with torch.no_grad():
            t0 = time.time()
            output = model(images.to(device))
            if device.type != "cpu":
                torch.cuda.synchronize()
            model_time += time.time() - t0
            if streaming:
                evaluator.update(output, [t.to(device) for t in targets])
            else:
                predictions.update({i: o.to("cpu") for i, o in zip(image_ids, output)})
    total = time.time() - start
    n = max(len(dataset), 1)
    logger.info("Total run time: {:.1f} s ({:.4f} s / img, matching included)".format(total, total / n))
    logger.info("Model inference time: {:.1f} s ({:.4f} s / img)".format(model_time, model_time / n))
    if output_folder:
        os.makedirs(output_folder, exist_ok=True)
    if streaming:
        logger.info("Matched {} detections against {} ground truths of {} images".format(
            evaluator.num_detections, evaluator.num_groundtruths, evaluator.num_images))
        return finish_coco(evaluator, output_folder, expected_results, expected_results_sigma_tol)
    predictions = [predictions[i] for i in sorted(predictions)]
    if output_folder:
        torch.save(predictions, os.path.join(output_folder, "predictions.pth"))
    return evaluate(dataset=dataset, predictions=predictions, output_folder=output_folder, box_only=box_only,
                    iou_types=iou_types, expected_results=expected_results,
                    expected_results_sigma_tol=expected_results_sigma_tol)
