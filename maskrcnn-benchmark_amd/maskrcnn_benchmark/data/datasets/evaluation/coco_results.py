"""COCO result files (reference data/datasets/evaluation/coco/coco_eval.py:70-186): the detections of a run in the COCO
results format, `bbox.json`, `segm.json` and `keypoints.json` — what the COCO servers accept and what any other tool,
pycocotools among them, reads.

`prepare_for_coco_detection`, `prepare_for_coco_segmentation` and `prepare_for_coco_keypoint` have the reference's names
and signatures, (predictions, dataset) -> list of dict; `COCOResultsWriter` is the same per image, fed batch by batch by
the inference loop.  Per image, as in the reference: resize to the image's original size (`get_img_info`), boxes in xywh,
`image_id` through `id_to_img_map`, `category_id` through `contiguous_category_id_to_json_id`, images without detections
skipped.  A dataset without those maps (the synthetic one) uses the index as the image id and the label as the category id.

Masks are dense planes of the image's ORIGINAL size or M x M floating-point probabilities; anything else raises (planes
pasted at the network's input size cannot be pasted again).  Probabilities are pasted at the original size with
Masker(0.5, padding=1)'s parameters: device tensors by `_C.paste_masks_rle` (planes never stored), CPU tensors by
`paste_masks_torch`; dense planes are run-length coded by torch operators where they live.  Either way the runs go to
`_C.rle_strings` (include/detops.h, "Compressed RLE strings"), so one image leaves the device as boxes, scores, labels,
keypoints, the strings' bytes and their offsets.

Not built: reading result files back, decoding compressed strings, `box_only` proposals, OKS."""
import json
import os

import torch

from maskrcnn_benchmark import _C
from maskrcnn_benchmark.modeling.roi_heads.mask_head.inference import paste_masks_torch

IOU_TYPES = ("bbox", "segm", "keypoints")
MASK_THRESHOLD, MASK_PADDING = 0.5, 1      # the reference's Masker(threshold=0.5, padding=1)


def _image_id(dataset, index):
    ids = getattr(dataset, "id_to_img_map", None)
    return int(index) if ids is None else ids[index]


def _category_ids(dataset, labels):
    table = getattr(dataset, "contiguous_category_id_to_json_id", None)
    return list(labels) if table is None else [table[i] for i in labels]


def _original(dataset, index, prediction):
    """the prediction in the frame of the image as it is on disk -> (BoxList, width, height)"""
    info = dataset.get_img_info(index)
    width, height = info["width"], info["height"]
    return prediction.resize((width, height)), width, height


def plane_runs(planes):
    """bool / uint8 [n, H, W] -> (counts int32 [total], run_offset int64 [n + 1]) on the planes' device: `rle_encode` of
    every plane (column-major runs starting with a 0-run), back to back, without a Python loop over the planes"""
    n, H, W = planes.shape
    dev = planes.device
    if n == 0:
        return torch.empty((0,), dtype=torch.int32, device=dev), torch.zeros((1,), dtype=torch.int64, device=dev)
    flat = planes.transpose(1, 2).reshape(n, H * W).to(torch.int8)
    before = torch.cat([flat.new_zeros((n, 1)), flat[:, :-1]], dim=1)
    row, pos = torch.nonzero(flat != before, as_tuple=True)          # row-major: plane after plane, positions ascending
    edges = torch.bincount(row, minlength=n)
    edge_start = torch.cumsum(edges, 0) - edges
    start = torch.cumsum(edges + 2, 0) - (edges + 2)                 # a plane's bounds: 0, its edges, H * W
    bounds = torch.zeros((int(pos.numel()) + 2 * n,), dtype=torch.int64, device=dev)
    bounds[start + edges + 1] = H * W
    bounds[start[row] + 1 + torch.arange(pos.numel(), device=dev) - edge_start[row]] = pos
    keep = torch.ones((bounds.numel() - 1,), dtype=torch.bool, device=dev)
    keep[start[1:] - 1] = False                                      # the difference across two planes
    counts = (bounds[1:] - bounds[:-1])[keep].to(torch.int32)
    run_offset = torch.cat([edges.new_zeros(1), torch.cumsum(edges + 1, 0)])
    return counts, run_offset


def mask_strings(masks, boxes, height, width):
    """the masks of one image, [n, 1, H, W] planes of the image's size or [n, 1, M, M] floating-point probabilities with
    their xyxy `boxes` in the image -> a list of n compressed `counts` strings; ValueError for anything else"""
    if masks.dim() == 3:
        masks = masks[:, None]
    if list(masks.shape[-2:]) == [height, width]:
        counts, run_offset = plane_runs(masks[:, 0] != 0)
    elif masks.shape[-1] != masks.shape[-2] or not masks.is_floating_point():
        # e.g. POSTPROCESS_MASKS planes pasted at the network's input size: they cannot be pasted again as probabilities
        raise ValueError("result files: masks of shape %s and dtype %s are neither planes of the image's original size "
                         "%d x %d nor M x M probability maps" % (tuple(masks.shape), masks.dtype, height, width))
    elif masks.is_cuda:
        counts, run_offset = _C.paste_masks_rle(masks, boxes, [(height, width)], MASK_THRESHOLD, MASK_PADDING,
                                                counts=[masks.shape[0]])
    else:
        counts, run_offset = plane_runs(paste_masks_torch(masks, boxes, height, width, MASK_THRESHOLD, MASK_PADDING)[:, 0])
    return _C.rle_string_list(*_C.rle_strings(counts, run_offset))


def detection_entries(dataset, index, prediction):
    if len(prediction) == 0:
        return []
    original_id = _image_id(dataset, index)
    prediction, _, _ = _original(dataset, index, prediction)
    prediction = prediction.convert("xywh")
    boxes = prediction.bbox.tolist()
    scores = prediction.get_field("scores").tolist()
    labels = _category_ids(dataset, prediction.get_field("labels").tolist())
    return [{"image_id": original_id, "category_id": labels[k], "bbox": box, "score": scores[k]}
            for k, box in enumerate(boxes)]


def segmentation_entries(dataset, index, prediction):
    if len(prediction) == 0:
        return []
    original_id = _image_id(dataset, index)
    prediction, width, height = _original(dataset, index, prediction)
    strings = mask_strings(prediction.get_field("mask"), prediction.convert("xyxy").bbox, height, width)
    scores = prediction.get_field("scores").tolist()
    labels = _category_ids(dataset, prediction.get_field("labels").tolist())
    return [{"image_id": original_id, "category_id": labels[k],
             "segmentation": {"size": [height, width], "counts": s}, "score": scores[k]}
            for k, s in enumerate(strings)]


def keypoint_entries(dataset, index, prediction):
    if len(prediction.bbox) == 0:
        return []
    original_id = _image_id(dataset, index)
    prediction, width, height = _original(dataset, index, prediction)
    scores = prediction.get_field("scores").tolist()
    labels = _category_ids(dataset, prediction.get_field("labels").tolist())
    keypoints = prediction.get_field("keypoints").resize((width, height))
    keypoints = keypoints.keypoints.reshape(keypoints.keypoints.shape[0], -1).tolist()
    return [{"image_id": original_id, "category_id": labels[k], "keypoints": keypoint, "score": scores[k]}
            for k, keypoint in enumerate(keypoints)]


_ENTRIES = {"bbox": detection_entries, "segm": segmentation_entries, "keypoints": keypoint_entries}


def _prepare(iou_type, predictions, dataset):
    results = []
    for index, prediction in enumerate(predictions):
        results.extend(_ENTRIES[iou_type](dataset, index, prediction))
    return results


def prepare_for_coco_detection(predictions, dataset):
    return _prepare("bbox", predictions, dataset)


def prepare_for_coco_segmentation(predictions, dataset):
    return _prepare("segm", predictions, dataset)


def prepare_for_coco_keypoint(predictions, dataset):
    return _prepare("keypoints", predictions, dataset)


class COCOResultsWriter(object):
    """The result files of a run, image by image: `update(predictions, image_indices)` per batch (BoxLists on any device and
    their indices in `dataset`), `save(folder)` at the end -> <folder>/<iou_type>.json for each of `iou_types`."""

    def __init__(self, dataset, iou_types):
        unknown = [t for t in iou_types if t not in IOU_TYPES]
        if unknown:
            raise ValueError("COCOResultsWriter: unknown iou types %s (of %s)" % (unknown, list(IOU_TYPES)))
        self.dataset = dataset
        self.iou_types = tuple(iou_types)
        self.results = {t: [] for t in self.iou_types}
        self.num_images = 0

    def update(self, predictions, image_indices):
        if len(predictions) != len(image_indices):
            raise ValueError("COCOResultsWriter.update: %d predictions for %d image indices"
                             % (len(predictions), len(image_indices)))
        for prediction, index in zip(predictions, image_indices):
            for t in self.iou_types:
                self.results[t].extend(_ENTRIES[t](self.dataset, int(index), prediction))
            self.num_images += 1

    def save(self, folder):
        """-> {iou_type: path}"""
        os.makedirs(folder, exist_ok=True)
        paths = {}
        for t in self.iou_types:
            paths[t] = os.path.join(folder, t + ".json")
            with open(paths[t], "w") as f:
                json.dump(self.results[t], f)
        return paths
